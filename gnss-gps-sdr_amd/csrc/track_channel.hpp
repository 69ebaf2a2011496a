// track_channel.hpp -- the tracking channel of include/gpsacq.h ("THE CHANNEL MODEL"), stated once for every kernel that runs it:
// one wave64 per channel, TRACK_WAVES independent channels per workgroup, no barrier in the epoch loop.
//
// What the reference's FPGA does per channel ("Homemade GPS Receiver", "Hardware / software split" and after): samples times a
// 1-bit carrier and early / prompt / late codes half a chip apart, integrate-and-dump on the code epoch; and what its embedded CPU
// does at 1 kHz: the Costas and early-minus-late PI loops with 64-bit integrators and power-of-two gains.  Here the host's AGC
// (c/channel.cpp:265-288) and code-aided carrier reset (:199-206), and an FLL pull-in, run in the same epoch loop.
//
// run_channel() is the epoch loop; how an epoch's samples become the six sums IE QE IP QP IL QL is the correlator's business
// (track_kernels.hip: 1-bit samples, popcounts; track_iq_kernels.hip: 8-bit complex samples, dot products), a template parameter,
// so nothing here asks which kernel it serves.  Every lane runs the same integer loop update and lane 0 writes the outputs with
// plain stores.  All arithmetic is integer: the result does not depend on the order of the sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_launch.hpp"

namespace acq {

static constexpr uint64_t kFull = 1023ull << 32;  // one code period, chips * 2^32

__device__ __forceinline__ bool outside(uint64_t v, uint64_t nom, int64_t win) {
    const int64_t d = (int64_t)(v - nom);
    return d > win || d < -win;
}

// the NCOs at sample kk of the epoch: the carrier's two sign bits (1: cos, -sin negative) and the early / prompt / late chips
struct NcoBits {
    uint32_t cb, sb, ce, cp, cl;
};
__device__ __forceinline__ NcoBits nco_bits(const gpsacq_track_chan& st, const uint32_t* chips, uint32_t kk) {
    const uint32_t ph = st.lo_phase + kk * st.lo_rate;
    const uint64_t P = st.ca_pos + (uint64_t)kk * st.ca_rate;
    const int ip = (int)(P >> 32), f = (int)((uint32_t)P >> 31);
    int ie = ip + f, il = ip - 1 + f;
    ie = ie == 1023 ? 0 : ie;
    il = il < 0 ? 1022 : il;
    NcoBits b;
    b.cb = ((ph >> 31) ^ (ph >> 30)) & 1u;
    b.sb = (~ph >> 31) & 1u;
    b.ce = (chips[ie >> 5] >> (ie & 31)) & 1u;
    b.cp = (chips[ip >> 5] >> (ip & 31)) & 1u;
    b.cl = (chips[il >> 5] >> (il & 31)) & 1u;
    return b;
}

// corr(st, chips, o, n, lane, sums): the epoch of n samples that starts at sample o of the window, NCOs as in st, chip words in
// LDS; leaves IE QE IP QP IL QL, summed over the wave, in sums[0..5] of every lane.
template <class Corr> __device__ __forceinline__ void run_channel(const TrackCommon& a, const Corr& corr) {
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
    const uint64_t win_end = a.first_sample + a.n_samples;
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
        int32_t sums[6];
        corr(st, chips, o, n, lane, sums);
        const int32_t IE = sums[0], QE = sums[1], IP = sums[2], QP = sums[3], IL = sums[4], QL = sums[5];
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

}  // namespace acq
