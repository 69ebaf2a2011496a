// capture_groups.hpp -- the group loop of the kernels that go back to an 8-bit IQ capture at a search peak, once:
// snapshot_iq_kernels.hip (k_refine_iq, k_fine_dop_iq) includes it, nothing else does.  It is capture_words.hpp's word loop with a
// 16-byte group (8 samples) where that has a 32-sample word, and iq_groups.hpp's dot products where that has popcounts:
// the IqCaptureArgs overload of window_of() is steps 1 to 3 of the text with the carrier word of gpsacq_track_start_iq8; segment_sums() walks one segment,
// lane l the groups l, l + 64, ... -- per group the mask of the samples before and after the segment, the carrier phase of sample
// 0, capture_words.hpp's code_window (the ONE 32-chip window that holds every chip of the group: 8 samples advance by fewer than
// 8 chips, early lies at most one chip past late's start plus that), then per dword the weight bytes of two samples and two dot
// products per replica.  "Snapshot chain on an 8-bit IQ capture" of include/gpsacq.h is the text.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "capture_words.hpp"
#include "iq_groups.hpp"
#include "snapshot_iq_launch.hpp"

namespace acq {

// steps 1 to 3 of "Fine code phases", PER TASK, as "Snapshot chain on an 8-bit IQ capture" changes them: the carrier word is
// gpsacq_track_start_iq8's, a hit needs |f| < fs / 2, the window starts at sample block * (stride / 2) of n_samples.  base_hz is
// f - lo_dop, what the fine Doppler takes off the replica's frequency.  Every lane of the workgroup decides the same
__device__ __forceinline__ Window window_of(const gpsacq_peak& pk, const IqCaptureArgs& c, size_t t, double snr_min, int blocks, double& base_hz) {
#pragma clang fp contract(off)  // the NCO words are the host's to the bit
    Window w = {false, (int32_t)(t % 32), 0, 0, 0, (uint64_t)c.n_samples, 0, 0};
    int32_t block = (int32_t)t;
    if (c.tasks) block = c.tasks[t].block, w.prn = c.tasks[t].prn;
    double lo_dop, ca_f;
    peak_dopplers(pk, c.fs, c.step_hz, lo_dop, ca_f);
    const double f = lo_dop - c.mix_hz + c.fc_lo;
    base_hz = f - lo_dop;
    w.hit = (double)pk.snr >= snr_min && pk.ca_shift >= 0 && pk.ca_shift < c.spm && block >= 0 && w.prn >= 0 && w.prn < GPSACQ_NUM_SATS &&
            fabs(f) < c.fs / 2 && ca_f >= 0 && ca_f < c.fs;
    if (!w.hit) return w;
    w.o = (uint64_t)block * (uint64_t)(c.stride / 2);  // stride <= 2^31: no overflow
    w.lo_rate = (uint32_t)(int64_t)llround(f / c.fs * 4294967296.0);
    w.ca_rate = (uint32_t)(ca_f / c.fs * 4294967296.0);
    window_segments(w, c.spm, blocks);
    return w;
}

// The sums of the segment [a0, a1) (capture samples) of a window that starts at sample o with the prompt position P0, over the
// wave, in every lane.  NX = 3: acc = IE QE IP QP IL QL with early and late D from prompt; NX = 1: acc = IP QP (D must be 0).
template <int NX>
__device__ __forceinline__ void segment_sums(const IqCaptureArgs& c, uint64_t a0, uint64_t a1, uint64_t o, uint64_t P0, uint32_t D, uint32_t lo_rate,
                                             uint32_t ca_rate, const uint32_t* s_chips, int lane, int32_t (&acc)[2 * NX]) {
    const bool dc = c.dc_i != 0 || c.dc_q != 0;
    const size_t iq_bytes = 2 * c.n_samples;
#pragma unroll
    for (int q = 0; q < 2 * NX; ++q) acc[q] = 0;  // before the mean correction
    int sc[NX], ss[NX];                            // sum h C, sum -h S per replica (only with a mean to remove)
#pragma unroll
    for (int X = 0; X < NX; ++X) sc[X] = ss[X] = 0;
    const uint64_t g1 = (a1 - 1) >> 3;
    for (uint64_t gi = (a0 >> 3) + lane; gi <= g1; gi += 64) {
        const uint4 raw = load_group(c.iq, iq_bytes, gi);
        const uint32_t x[4] = {raw.x ^ c.flip, raw.y ^ c.flip, raw.z ^ c.flip, raw.w ^ c.flip};
        const uint64_t gs = gi << 3;
        const uint32_t b_lo = gs < a0 ? (uint32_t)(a0 - gs) : 0u;      // 0 .. 7
        const uint32_t b_hi = gs + 8 > a1 ? (uint32_t)(a1 - gs) : 8u;  // 1 .. 8
        const CodeWindow cw = code_window(gs + b_lo - o, b_lo, P0, D, ca_rate, s_chips);
        uint32_t ph = (uint32_t)(gs - o) * lo_rate;  // modulo 2^32 also where the group starts before the window
        uint64_t rel = cw.rel;                       // rel - D >= 0 and rel + D + 7 ca_rate < 10 * 2^32: every shift below is < 32
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t wi[NX], wq[NX];
#pragma unroll
            for (int X = 0; X < NX; ++X) wi[X] = wq[X] = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t k = 2 * d + h;
                const uint32_t keep = k >= b_lo && k < b_hi ? 0xFFFFu : 0u;
                const uint32_t cb = ((ph >> 31) ^ (ph >> 30)) & 1u, sb = (~ph >> 31) & 1u;  // the carrier bits of THE CHANNEL MODEL
                uint32_t chip[NX];
                if constexpr (NX == 3) {
                    chip[0] = (cw.win >> (uint32_t)((rel + D) >> 32)) & 1u;
                    chip[1] = (cw.win >> (uint32_t)(rel >> 32)) & 1u;
                    chip[2] = (cw.win >> (uint32_t)((rel - D) >> 32)) & 1u;
                } else {
                    chip[0] = (cw.win >> (uint32_t)(rel >> 32)) & 1u;
                }
#pragma unroll
                for (int X = 0; X < NX; ++X) {
                    uint32_t pi, pq;
                    weight_bytes(chip[X] ^ cb, chip[X] ^ sb, keep, pi, pq);
                    wi[X] |= pi << (16 * h);
                    wq[X] |= pq << (16 * h);
                }
                ph += lo_rate;
                rel += ca_rate;
            }
#pragma unroll
            for (int X = 0; X < NX; ++X) {
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
        for (int X = 0; X < NX; ++X) {
            acc[2 * X] -= c.dc_i * sc[X] + c.dc_q * ss[X];
            acc[2 * X + 1] += c.dc_i * ss[X] - c.dc_q * sc[X];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int q = 0; q < 2 * NX; ++q) acc[q] += __shfl_xor(acc[q], m, 64);
}

}  // namespace acq
