// snapshot_records.hpp -- what the 1-bit and the 8-bit IQ member of a snapshot kernel pair do alike once their sums are taken, ONCE:
// the records of include/gpsacq.h from integer sums, flags and the output peak.  The pairs are k_refine / k_refine_iq (fine_record),
// k_fine_dop / k_fine_dop_iq (dopfine_record), k_aided / k_aided_iq (aided_record) and k_aided_coh / k_aided_coh_iq
// (aided_coh_record); the four aided kernels also share window_at and aided_prologue, steps 1 and 2 of "Aided acquisition".  How a
// kernel comes by its sums (words and popcounts, or groups and dot products), by its winner (a packed key, or a (power, tag) pair)
// and by its floor (2 spm segments, or the measured sum) stays in the kernel.  `Args` is the kernel's argument block: its `c` is a
// BitCaptureArgs or an IqCaptureArgs, which both have spm, fs, step_hz and peaks.
// Every file that includes this is built with -ffp-contract=off (Makefile) and every double expression keeps the order of the
// text, one IEEE operation each: the records are the host reference's to the bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture_words.hpp"
#include "nav_device.hpp"

namespace acq {

// "Fine code phases", 5. estimate, 6. usable.  D: early's and late's distance from prompt, P0: the prompt position of window
// sample 0, both chips * 2^32
__device__ __forceinline__ gpsacq_fine fine_record(uint64_t segments, uint64_t fit, int min_segments, uint32_t lo_rate, uint32_t ca_rate, uint32_t D,
                                                   uint64_t P0, uint64_t early, uint64_t prompt, uint64_t late) {
    gpsacq_fine r = {0, (int32_t)segments, lo_rate, ca_rate, early, prompt, late, 0.0, 0.0};
    if (segments < fit) r.flags |= GPSACQ_FINE_SHORT;
    if (segments < (uint64_t)min_segments) r.flags |= GPSACQ_FINE_FEW;
    if (r.early + r.late == 0) {
        r.flags |= GPSACQ_FINE_NO_POWER;
    } else {
        const double d = (double)D / 4294967296.0, aE = sqrt((double)r.early), aL = sqrt((double)r.late);
        r.offset_chips = (1.0 - d) * (aE - aL) / (aE + aL);
        double pos = (double)P0 / 4294967296.0 + r.offset_chips;
        if (pos < 0.0) pos += 1023.0;
        else if (pos >= 1023.0) pos -= 1023.0;
        r.tx_frac = pos / 1.023e6;
        if (!(r.tx_frac < 1e-3)) r.tx_frac = 0.0;
    }
    return r;
}

// "Cold snapshot fixes", the fine Doppler's estimate and flags.  T = spm / fs, one segment; base_hz is window_of's.
// nco_hz: the replica's carrier frequency lo_rate * fs / 2^32, which THE CALLER converts because the two captures differ on
// purpose: k_fine_dop reads lo_rate unsigned (a real capture's fc + lo_dop may pass fs / 2), k_fine_dop_iq reads it as int32 (complex
// baseband: the frequency has a sign)
__device__ __forceinline__ gpsacq_dopfine dopfine_record(uint64_t segments, uint64_t fit, const gpsacq_dopfine_params& p, uint32_t lo_rate,
                                                         uint32_t ca_rate, uint64_t re, uint64_t im, uint64_t mag, uint64_t power, double nco_hz,
                                                         double base_hz, double T) {
    gpsacq_dopfine r = {0, (int32_t)segments, lo_rate, ca_rate, (int64_t)re, (int64_t)im, mag, power, 0.0, 0.0, 0.0};
    if (segments < fit) r.flags |= GPSACQ_DOPFINE_SHORT;
    if (segments < (uint64_t)p.min_segments) r.flags |= GPSACQ_DOPFINE_FEW;
    if (r.mag == 0 || (r.re == 0 && r.im == 0)) {
        r.flags |= GPSACQ_DOPFINE_NO_POWER;
    } else {
        r.df_hz = atan2((double)r.im, (double)r.re) / ((4.0 * PI) * T);
        r.coherence = hypot((double)r.re, (double)r.im) / (double)r.mag;
        r.doppler_hz = (nco_hz - base_hz) + r.df_hz;
    }
    if (r.coherence < p.coherence_min) r.flags |= GPSACQ_DOPFINE_WEAK;
    return r;
}

// ---- the aided searches ------------------------------------------------------------------------------------------------------
// the window of Doppler hypothesis lo_shift: steps 1 to 3 of the capture's section on a peak that is a hit by itself
template <class Args> __device__ __forceinline__ Window window_at(const Args& a, size_t t, int64_t lo_shift) {
    Window w = {false, 0, 0, 0, 0, 0, 0, 0};
    if (lo_shift < -(int64_t)a.kmax || lo_shift > (int64_t)a.kmax) return w;
    const gpsacq_peak pk = {1.0f, (int32_t)lo_shift, 0, 0.0f};
    double base_hz;
    return window_of(pk, a.c, t, 0.0, a.p.blocks, base_hz);
}

// the record of a task that is not searched, one per record type
__device__ __forceinline__ void blank_record(gpsacq_aided& r, int flag) { r = gpsacq_aided{flag, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0}; }
__device__ __forceinline__ void blank_record(gpsacq_aided_coh& r, int flag) {
    r = gpsacq_aided_coh{flag, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0};
}

// 1. kept, 2. no aid, for the whole workgroup (every lane decides the same).  True: the task is searched, win is the window of
// the first valid Doppler hypothesis d_first and pk_out the zero peak.  False: the flag and zeros are written as the task's
// record, peaks_in's peak (kept) or the zero peak as its peak, and zeros over its n_powers powers (powers may be NULL)
template <class Args>
__device__ __forceinline__ bool aided_prologue(const Args& a, size_t t, const gpsacq_aid& aid, unsigned long long* powers, int n_powers,
                                               gpsacq_peak& pk_out, Window& win, int& d_first) {
    const int K = a.p.dop_half, n_dop = 2 * K + 1;
    int blank = 0;
    pk_out = gpsacq_peak{0.0f, 0, 0, 0.0f};
    if (a.c.peaks) {
        const gpsacq_peak pk = a.c.peaks[t];
        if ((double)pk.snr >= a.p.keep_snr) blank = GPSACQ_AIDED_KEPT, pk_out = pk;
    }
    win = Window{false, 0, 0, 0, 0, 0, 0, 0};
    d_first = 0;
    if (!blank) {
        if (aid.flags == 0 && aid.ca_center >= 0 && aid.ca_center < a.c.spm)
            for (int d = 0; d < n_dop && !win.hit; ++d) win = window_at(a, t, (int64_t)aid.lo_center - K + d), d_first = d;
        if (!win.hit) blank = GPSACQ_AIDED_NO_AID;
    }
    if (!blank) return true;
    if (threadIdx.x == 0) {
        blank_record(a.out[t], blank);
        a.peaks_out[t] = pk_out;
    }
    if (powers)
        for (int i = threadIdx.x; i < n_powers; i += blockDim.x) powers[i] = 0;
    return false;
}

// the first code hypothesis of a task, samples: ca_center - W modulo spm
__device__ __forceinline__ uint32_t aided_base(const gpsacq_aid& aid, int W, int spm) { return (uint32_t)(((aid.ca_center - W) % spm + spm) % spm); }

// what both aided records hold alike (R: gpsacq_aided or gpsacq_aided_coh with best, best_h, best_d and floor set): the winner's
// place on the engine's grid, the ratio, the flags, and the peak where the record is usable
template <class R, class Args>
__device__ __forceinline__ void aided_close(R& r, const Args& a, const gpsacq_aid& aid, uint32_t base, uint64_t fit, gpsacq_peak& pk_out) {
    r.lo_shift = aid.lo_center - a.p.dop_half + r.best_d;
    r.ca_shift = (int32_t)((base + (uint32_t)r.best_h) % (uint32_t)a.c.spm);
    if (r.floor) r.ratio = (double)r.best / (double)r.floor;
    if ((uint64_t)r.segments < fit) r.flags |= GPSACQ_AIDED_SHORT;
    if (r.segments < a.p.min_segments) r.flags |= GPSACQ_AIDED_FEW;
    if (r.best == 0) r.flags |= GPSACQ_AIDED_NO_POWER;
    if (r.ratio < a.p.ratio_min) r.flags |= GPSACQ_AIDED_BELOW;
    if (!(r.flags & (GPSACQ_AIDED_FEW | GPSACQ_AIDED_NO_POWER | GPSACQ_AIDED_BELOW))) pk_out = gpsacq_peak{(float)r.ratio, r.lo_shift, r.ca_shift, (float)r.best};
}

// "Aided acquisition", 5. record, 6. peak, by ONE thread: the winner (best at code hypothesis best_h, Doppler hypothesis best_d),
// the total over all hypotheses and the floor into task t's record and peak
template <class Args>
__device__ __forceinline__ void aided_record(const Args& a, size_t t, const gpsacq_aid& aid, uint32_t base, uint64_t segments, uint64_t fit, uint64_t best,
                                             int32_t best_h, int32_t best_d, uint64_t total, uint64_t floor, gpsacq_peak pk_out) {
    gpsacq_aided r = {0, (int32_t)segments, 2 * a.p.code_half + 1, 2 * a.p.dop_half + 1, best_h, best_d, 0, 0, best, total, floor, 0.0};
    aided_close(r, a, aid, base, fit, pk_out);
    a.out[t] = r;
    a.peaks_out[t] = pk_out;
}

// "Coherent aided acquisition", 6. record and peak, by ONE thread: the winner (best at h, d, fine Doppler hypothesis best_f and
// bit edge best_e of coh_ms), the non-coherent sum of its (h, d) and the floor into task t's record and peak
template <class Args>
__device__ __forceinline__ void aided_coh_record(const Args& a, size_t t, const gpsacq_aid& aid, uint32_t base, uint64_t segments, uint64_t fit, int coh_ms,
                                                 uint64_t best, int32_t best_h, int32_t best_d, int32_t best_f, int32_t best_e, uint64_t noncoh,
                                                 uint64_t floor, gpsacq_peak pk_out) {
    const int F = a.p.fine_half;
    gpsacq_aided_coh r = {0, (int32_t)segments, 2 * a.p.code_half + 1, 2 * a.p.dop_half + 1, 2 * F + 1, coh_ms, best_h, best_d, best_f, best_e, 0, 0, best, noncoh,
                          floor, 0.0, 0.0, 0.0};
    aided_close(r, a, aid, base, fit, pk_out);
    const double lo_dop = a.c.step_hz > 0 ? r.lo_shift * a.c.step_hz : r.lo_shift * a.c.fs / 40000.0;
    r.doppler_hz = lo_dop + ((double)((r.best_f - F) * a.p.fine_step) / 1024.0) * (a.c.fs / (double)a.c.spm);
    a.out[t] = r;
    a.peaks_out[t] = pk_out;
}

}  // namespace acq
