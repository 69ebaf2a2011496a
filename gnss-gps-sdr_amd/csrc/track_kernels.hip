// track_kernels.hip -- the tracking channels of include/gpsacq.h ("THE CHANNEL MODEL") on the 1-bit stream: track_channel.hpp's
// loop around a popcount correlator.
//
// Each epoch's samples are cut into 32-sample words of the window; lane l takes words l, l + 64, ...  Per word it builds five
// 32-bit masks (cos, -sin, early, prompt, late chips) one sample at a time from the NCO words and takes six popcounts against the
// sample word.  The six counts of ones are packed in pairs (each fits 16 bits: each count <= n <= max_epoch <= 65535) and summed
// over the wave with xor shuffles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_channel.hpp"

namespace acq {

__device__ __forceinline__ uint32_t load_word(const uint8_t* b, size_t n_bytes, uint64_t wi) {
    const size_t off = (size_t)wi * 4;
    if (off + 4 <= n_bytes) return *reinterpret_cast<const uint32_t*>(b + off);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (off + k < n_bytes) v |= (uint32_t)b[off + k] << (8 * k);
    return v;
}

struct BitsCorr {
    const uint8_t* bits;
    size_t n_bytes;
    __device__ __forceinline__ void operator()(const gpsacq_track_chan& st, const uint32_t* chips, uint64_t o, uint64_t n, int lane,
                                               int32_t (&sums)[6]) const {
        const uint64_t w0 = o >> 5, w1 = (o + n - 1) >> 5;
        uint32_t ones[6] = {0, 0, 0, 0, 0, 0};  // IE QE IP QP IL QL: samples whose product is -1
        for (uint64_t wi = w0 + lane; wi <= w1; wi += 64) {
            const uint32_t x = load_word(bits, n_bytes, wi);
            const int j0 = (int)((int64_t)(wi * 32) - (int64_t)o);  // epoch sample index of bit 0 of this word (> -32, < max_epoch)
            uint32_t cm = 0, sm = 0, em = 0, pm = 0, lm = 0, valid = 0;
#pragma unroll 8
            for (int b = 0; b < 32; ++b) {
                const int k = j0 + b;
                const bool ok = k >= 0 && k < (int)n;
                const NcoBits nb = nco_bits(st, chips, ok ? (uint32_t)k : 0u);
                cm |= nb.cb << b;
                sm |= nb.sb << b;
                em |= nb.ce << b;
                pm |= nb.cp << b;
                lm |= nb.cl << b;
                valid |= (ok ? 1u : 0u) << b;
            }
            ones[0] += __popc((x ^ em ^ cm) & valid);
            ones[1] += __popc((x ^ em ^ sm) & valid);
            ones[2] += __popc((x ^ pm ^ cm) & valid);
            ones[3] += __popc((x ^ pm ^ sm) & valid);
            ones[4] += __popc((x ^ lm ^ cm) & valid);
            ones[5] += __popc((x ^ lm ^ sm) & valid);
        }
        uint32_t pk[3] = {ones[0] | ones[1] << 16, ones[2] | ones[3] << 16, ones[4] | ones[5] << 16};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < 3; ++q) pk[q] += (uint32_t)__shfl_xor((int)pk[q], m, 64);
        const int32_t nn = (int32_t)n;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            sums[2 * q] = nn - 2 * (int32_t)(pk[q] & 0xFFFF);
            sums[2 * q + 1] = nn - 2 * (int32_t)(pk[q] >> 16);
        }
    }
};

__global__ __launch_bounds__(64 * TRACK_WAVES) void k_track(TrackArgs a) { run_channel(a, BitsCorr{a.bits, a.n_bytes}); }

void launch_track(const TrackArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_track, dim3((unsigned)((a.n_chans + TRACK_WAVES - 1) / TRACK_WAVES)), dim3(64 * TRACK_WAVES), 0, s, a);
}

}  // namespace acq
