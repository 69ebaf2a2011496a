// track_kernels.hip -- the tracking channels of include/gpsacq.h ("THE CHANNEL MODEL"), one wave64 per channel.
//
// What the reference's FPGA does per channel ("Homemade GPS Receiver", "Hardware / software split" and after): 1-bit samples
// XOR a 1-bit carrier and early / prompt / late codes half a chip apart, integrate-and-dump on the code epoch; and what its
// embedded CPU does at 1 kHz: the Costas and early-minus-late PI loops with 64-bit integrators and power-of-two gains.  Here the
// host's AGC (c/channel.cpp:265-288) and code-aided carrier reset (:199-206), and an FLL pull-in, run in the same epoch loop.
//
// Layout: TRACK_WAVES independent channels per workgroup, no barrier in the epoch loop.  Each epoch's samples are cut into
// 32-sample words of the window; lane l takes words l, l + 64, ...  Per word it builds five 32-bit masks (cos, -sin, early,
// prompt, late chips) one sample at a time from the NCO words and takes six popcounts against the sample word.  The six counts
// of ones are packed in pairs (each fits 16 bits: each count <= n <= max_epoch <= 65535) and summed over the wave with xor shuffles; every lane then runs
// the same integer loop update, and lane 0 writes the outputs with plain stores.  All arithmetic is integer: the result does not
// depend on the order of the sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_launch.hpp"

namespace acq {

static constexpr uint64_t kFull = 1023ull << 32;  // one code period, chips * 2^32

__device__ __forceinline__ uint32_t load_word(const uint8_t* b, size_t n_bytes, uint64_t wi) {
    const size_t off = (size_t)wi * 4;
    if (off + 4 <= n_bytes) return *reinterpret_cast<const uint32_t*>(b + off);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (off + k < n_bytes) v |= (uint32_t)b[off + k] << (8 * k);
    return v;
}

__device__ __forceinline__ bool outside(uint64_t v, uint64_t nom, int64_t win) {
    const int64_t d = (int64_t)(v - nom);
    return d > win || d < -win;
}

__global__ __launch_bounds__(64 * TRACK_WAVES) void k_track(TrackArgs a) {
    __shared__ uint32_t s_chips[TRACK_WAVES][32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * TRACK_WAVES + wv;
    const bool live = c < a.n_chans;
    gpsacq_track_chan st = live ? a.chans[c] : gpsacq_track_chan{};
    if (live && lane < 32) s_chips[wv][lane] = a.chips[(st.prn - 1) * 32 + lane];
    __syncthreads();  // the only barrier: the chip table is in place
    if (!live) return;
    const uint32_t* chips = s_chips[wv];
    const gpsacq_track_params& p = a.prm;
    const uint64_t win_end = a.first_sample + 8ull * a.n_bytes;
    const uint64_t lo_nom = (uint64_t)st.lo_nom, ca_nom = (uint64_t)st.ca_nom;
    uint64_t lo_int = (uint64_t)st.lo_int, ca_int = (uint64_t)st.ca_int;
    int t = 0;
    for (; t < a.max_epochs && st.status == GPSACQ_TRACK_OK; ++t) {
        const uint64_t n = (kFull - st.ca_pos + st.ca_rate - 1) / st.ca_rate;
        if (n < (uint64_t)p.min_epoch || n > (uint64_t)p.max_epoch) {
            st.status = GPSACQ_TRACK_LOST;
            break;
        }
        if (st.next_sample + n > win_end) break;
        const uint64_t o = st.next_sample - a.first_sample;  // window-relative start
        const uint64_t w0 = o >> 5, w1 = (o + n - 1) >> 5;
        uint32_t ones[6] = {0, 0, 0, 0, 0, 0};  // IE QE IP QP IL QL: samples whose product is -1
        for (uint64_t wi = w0 + lane; wi <= w1; wi += 64) {
            const uint32_t x = load_word(a.bits, a.n_bytes, wi);
            const int j0 = (int)((int64_t)(wi * 32) - (int64_t)o);  // epoch sample index of bit 0 of this word (> -32, < max_epoch)
            uint32_t cm = 0, sm = 0, em = 0, pm = 0, lm = 0, valid = 0;
#pragma unroll 8
            for (int b = 0; b < 32; ++b) {
                const int k = j0 + b;
                const bool ok = k >= 0 && k < (int)n;
                const uint32_t kk = ok ? (uint32_t)k : 0u;
                const uint32_t ph = st.lo_phase + kk * st.lo_rate;
                const uint64_t P = st.ca_pos + (uint64_t)kk * st.ca_rate;
                const int ip = (int)(P >> 32), f = (int)((uint32_t)P >> 31);
                int ie = ip + f, il = ip - 1 + f;
                ie = ie == 1023 ? 0 : ie;
                il = il < 0 ? 1022 : il;
                const uint32_t ce = (chips[ie >> 5] >> (ie & 31)) & 1u;
                const uint32_t cp = (chips[ip >> 5] >> (ip & 31)) & 1u;
                const uint32_t cl = (chips[il >> 5] >> (il & 31)) & 1u;
                cm |= (((ph >> 31) ^ (ph >> 30)) & 1u) << b;
                sm |= ((~ph >> 31) & 1u) << b;
                em |= ce << b;
                pm |= cp << b;
                lm |= cl << b;
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
        const int32_t IE = nn - 2 * (int32_t)(pk[0] & 0xFFFF), QE = nn - 2 * (int32_t)(pk[0] >> 16);
        const int32_t IP = nn - 2 * (int32_t)(pk[1] & 0xFFFF), QP = nn - 2 * (int32_t)(pk[1] >> 16);
        const int32_t IL = nn - 2 * (int32_t)(pk[2] & 0xFFFF), QL = nn - 2 * (int32_t)(pk[2] >> 16);
        if (lane == 0) {
            const size_t r = (size_t)c * a.max_epochs + t;
            if (a.prompt) {
                a.prompt[2 * r] = IP;
                a.prompt[2 * r + 1] = QP;
            }
            if (a.records) {
                gpsacq_track_record rec;
                rec.sample = st.next_sample;
                rec.ie = IE, rec.qe = QE, rec.ip = IP, rec.qp = QP, rec.il = IL, rec.ql = QL;
                rec.lo_rate = st.lo_rate, rec.ca_rate = st.ca_rate;
                a.records[r] = rec;
            }
        }
        // the NCOs past the epoch
        st.lo_phase += (uint32_t)n * st.lo_rate;
        st.ca_pos = st.ca_pos + n * st.ca_rate - kFull;
        st.next_sample += n;
        st.epoch += 1;
        const int k = st.epoch;
        // AGC
        if (p.agc_period > 0 && k % p.agc_period == 0) {
            st.pwr[st.pwr_pos] = (int64_t)IP * IP + (int64_t)QP * QP;
            st.pwr_pos = (st.pwr_pos + 1) & 7;
            int64_t S = 0;
            for (int i = 0; i < 8; ++i) S += st.pwr[i];
            if (st.gain_adj) {
                if (S < 8 * p.agc_lo) st.gain_adj = 0;
            } else if (S > 8 * p.agc_hi) {
                st.gain_adj = -1;
            }
        }
        // carrier: FLL pull-in, then Costas
        if (st.fll_left > 0) {
            const int64_t dot = (int64_t)st.prev_ip * IP + (int64_t)st.prev_qp * QP;
            const int64_t cross = (int64_t)st.prev_ip * QP - (int64_t)st.prev_qp * IP;
            const int64_t e = dot > 0 ? cross : (dot < 0 ? -cross : 0);
            lo_int += (uint64_t)e << p.fll_k;
            st.lo_rate = (uint32_t)(lo_int >> 32);
            st.fll_left -= 1;
        } else {
            const int64_t e = (int64_t)IP * QP;
            lo_int += (uint64_t)e << (p.lo_ki + st.gain_adj);
            st.lo_rate = (uint32_t)((lo_int + ((uint64_t)e << (p.lo_kp + st.gain_adj))) >> 32);
        }
        st.prev_ip = IP;
        st.prev_qp = QP;
        // code: early-minus-late power
        {
            const int64_t e = ((int64_t)IE * IE + (int64_t)QE * QE) - ((int64_t)IL * IL + (int64_t)QL * QL);
            ca_int += (uint64_t)e << p.ca_ki;
            st.ca_rate = (uint32_t)((ca_int + ((uint64_t)e << p.ca_kp)) >> 32);
        }
        // code-aided carrier reset
        if (k == p.aid_epoch) {
            lo_int = lo_nom + (ca_int - ca_nom) * 1540ull;
            st.lo_rate = (uint32_t)(lo_int >> 32);
        }
        if (outside(lo_int, lo_nom, p.lo_window) || outside((uint64_t)st.lo_rate << 32, lo_nom, p.lo_window) ||
            outside(ca_int, ca_nom, p.ca_window) || outside((uint64_t)st.ca_rate << 32, ca_nom, p.ca_window))
            st.status = GPSACQ_TRACK_LOST;
    }
    st.lo_int = (int64_t)lo_int;
    st.ca_int = (int64_t)ca_int;
    if (lane == 0) {
        a.chans[c] = st;
        a.n_epochs[c] = t;
    }
}

void launch_track(const TrackArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_track, dim3((unsigned)((a.n_chans + TRACK_WAVES - 1) / TRACK_WAVES)), dim3(64 * TRACK_WAVES), 0, s, a);
}

}  // namespace acq
