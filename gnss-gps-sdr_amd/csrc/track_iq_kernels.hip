// track_iq_kernels.hip -- tracking channels on an 8-bit IQ capture kept at full amplitude (include/gpsacq.h, "Tracking channels on
// an 8-bit IQ capture", multi-bit mode): track_channel.hpp's loop around a dot-product correlator.  No reference counterpart: the
// reference's channels are 1-bit ("Homemade GPS Receiver"); its rtl-sdr / HackRF flow (README.md:83-115) quantises to 1 bit
// before anything runs.
//
// Each epoch's samples are cut into 16-byte groups of the window (8 samples: I0 Q0 I1 Q1 ...), lane l takes groups l, l + 64, ...
// A dword holds two samples; against a weight dword (h C, -h S, h C', -h S') a 4 x int8 dot product (v_dot4_i32_i8) gives two
// samples of I_X = sum h (v_i C - v_q S), against (h S, h C, ...) two samples of Q_X = sum h (v_i S + v_q C).  Weights are +1, -1
// or 0 (a sample outside the epoch).  GPSACQ_IQ_U8 bytes are XORed with 0x80 first (byte ^ 0x80 read as int8 = byte - 128); the
// removed mean is a correction -dc * sum(weights) that costs two more dot products per dword and only when it is not zero.
// load_group, dot4 and the weight bytes live in iq_groups.hpp, which the snapshot kernels on an IQ capture share.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iq_groups.hpp"
#include "track_channel.hpp"

namespace acq {

struct IqCorr {
    const uint8_t* iq;
    size_t iq_bytes;
    uint32_t flip;
    int32_t dc_i, dc_q;
    __device__ __forceinline__ void operator()(const gpsacq_track_chan& st, const uint32_t* chips, uint64_t o, uint64_t n, int lane,
                                               int32_t (&acc)[6]) const {
        const bool dc = dc_i != 0 || dc_q != 0;
        const uint64_t g0 = o >> 3, g1 = (o + n - 1) >> 3;
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = 0;     // IE QE IP QP IL QL before the mean correction
        int sc[3] = {0, 0, 0}, ss[3] = {0, 0, 0};  // sum h C, sum -h S per E, P, L (only with a mean to remove)
        for (uint64_t gi = g0 + lane; gi <= g1; gi += 64) {
            const uint4 raw = load_group(iq, iq_bytes, gi);
            const uint32_t x[4] = {raw.x ^ flip, raw.y ^ flip, raw.z ^ flip, raw.w ^ flip};
            const int j0 = (int)((int64_t)(gi * 8) - (int64_t)o);  // epoch sample index of the group's first sample (> -8, < max_epoch)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t wi[3] = {0, 0, 0}, wq[3] = {0, 0, 0};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = j0 + 2 * d + h;
                    const bool ok = k >= 0 && k < (int)n;
                    const NcoBits nb = nco_bits(st, chips, ok ? (uint32_t)k : 0u);
                    const uint32_t chip[3] = {nb.ce, nb.cp, nb.cl};
                    const uint32_t keep = ok ? 0xFFFFu : 0u;
#pragma unroll
                    for (int X = 0; X < 3; ++X) {
                        const uint32_t bc = chip[X] ^ nb.cb, bs = chip[X] ^ nb.sb;  // 1: h C = -1, h S = -1
                        uint32_t pi, pq;  // bytes +1 (0x01) / -1 (0xFF): (h C, -h S) for the I arm, (h S, h C) for the Q arm
                        weight_bytes(bc, bs, keep, pi, pq);
                        wi[X] |= pi << (16 * h);
                        wq[X] |= pq << (16 * h);
                    }
                }
#pragma unroll
                for (int X = 0; X < 3; ++X) {
                    acc[2 * X] = dot4(x[d], wi[X], acc[2 * X]);
                    acc[2 * X + 1] = dot4(x[d], wq[X], acc[2 * X + 1]);
                    if (dc) {
                        sc[X] = dot4(wi[X], 0x00010001u, sc[X]);
                        ss[X] = dot4(wi[X], 0x01000100u, ss[X]);
                    }
                }
            }
        }
        if (dc) {
            // I_X = sum h ((a_i - dc_i) C - (a_q - dc_q) S),  Q_X = sum h ((a_i - dc_i) S + (a_q - dc_q) C);  ss holds sum -h S
#pragma unroll
            for (int X = 0; X < 3; ++X) {
                acc[2 * X] -= dc_i * sc[X] + dc_q * ss[X];
                acc[2 * X + 1] += dc_i * ss[X] - dc_q * sc[X];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += __shfl_xor(acc[q], m, 64);
    }
};

__global__ __launch_bounds__(64 * TRACK_WAVES) void k_track_iq(TrackIqArgs a) {
    run_channel(a, IqCorr{a.iq, 2 * (size_t)a.n_samples, a.flip, a.dc_i, a.dc_q});
}

void launch_track_iq(const TrackIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_track_iq, dim3((unsigned)((a.n_chans + TRACK_WAVES - 1) / TRACK_WAVES)), dim3(64 * TRACK_WAVES), 0, s, a);
}

}  // namespace acq
