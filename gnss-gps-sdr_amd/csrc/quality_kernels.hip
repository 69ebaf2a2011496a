// quality_kernels.hip -- "Signal quality per observation" of include/gpsacq.h: the signal-to-noise-variance estimate of C/N0, the
// phase-lock ratio and the weight of every (instant, channel), from the prompt sums of the tracking records.  Integers up to the
// conversions of sig and noise; then one division, one product, one log10, one more division.
//
// k_quality_acc: one wave64 per channel, k_lock_acc's idiom (smooth_kernels.hip): forward prefix sums of |ip|, ip^2 + qp^2 and
// ip^2 - qp^2 over the epochs, chunks of 64 x SMOOTH_RUN epochs, runs per lane, one __shfl_up scan per sum, a 64-bit carry each.
// k_quality_out: one lane per (instant, channel); one bisection gives t, the three window sums are differences of the prefix sums.
// No LDS, no barrier, no atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quality_launch.hpp"

namespace acq {

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_quality_acc(QualityAccArgs a) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = a.chan[c].n;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    uint64_t* out_a = a.sum_a + (size_t)c * ((size_t)a.max_epochs + 1);
    uint64_t* out_d = a.sum_d + (size_t)c * ((size_t)a.max_epochs + 1);
    uint64_t* out_n = a.sum_n + (size_t)c * ((size_t)a.max_epochs + 1);
    constexpr int CHUNK = SMOOTH_BLOCK * SMOOTH_RUN;
    if (lane == 0) out_a[0] = 0, out_d[0] = 0, out_n[0] = 0;
    uint64_t carry_a = 0, carry_d = 0, carry_n = 0;  // the sums at the first epoch of the chunk, mod 2^64
    for (int base = 0; base < n; base += CHUNK) {
        const int t0 = base + lane * SMOOTH_RUN;
        // inclusive prefix sums inside this lane's run
        uint64_t pre_a[SMOOTH_RUN], pre_d[SMOOTH_RUN], pre_n[SMOOTH_RUN];
        uint64_t run_a = 0, run_d = 0, run_n = 0;
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j) {
            if (t0 + j < n) {
                const int64_t ip = rec[t0 + j].ip, qp = rec[t0 + j].qp;
                const uint64_t i2 = (uint64_t)(ip * ip), q2 = (uint64_t)(qp * qp);
                run_a += (uint64_t)(ip < 0 ? -ip : ip);
                run_d += i2 + q2;
                run_n += i2 - q2;
            }
            pre_a[j] = run_a, pre_d[j] = run_d, pre_n[j] = run_n;
        }
        // inclusive prefix scans of the run totals over the wave
        uint64_t incl_a = run_a, incl_d = run_d, incl_n = run_n;
#pragma unroll
        for (int off = 1; off < SMOOTH_BLOCK; off <<= 1) {
            const uint64_t va = __shfl_up((unsigned long long)incl_a, off, SMOOTH_BLOCK);
            const uint64_t vd = __shfl_up((unsigned long long)incl_d, off, SMOOTH_BLOCK);
            const uint64_t vn = __shfl_up((unsigned long long)incl_n, off, SMOOTH_BLOCK);
            if (lane >= off) incl_a += va, incl_d += vd, incl_n += vn;
        }
        // everything before this lane's run
        const uint64_t left_a = carry_a + (incl_a - run_a), left_d = carry_d + (incl_d - run_d), left_n = carry_n + (incl_n - run_n);
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j)
            if (t0 + j < n) {
                out_a[t0 + j + 1] = left_a + pre_a[j];
                out_d[t0 + j + 1] = left_d + pre_d[j];
                out_n[t0 + j + 1] = left_n + pre_n[j];
            }
        carry_a += __shfl((unsigned long long)incl_a, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
        carry_d += __shfl((unsigned long long)incl_d, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
        carry_n += __shfl((unsigned long long)incl_n, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
    }
}

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_quality_out(QualityOutArgs a) {
    const size_t i = (size_t)blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= a.n_fix) return;
    const QualityChan ch = a.chan[c];
    const uint64_t R = a.first_rx_sample + (uint64_t)i * a.rx_step;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    gpsacq_quality_info f;
    f.epochs = f.flags = 0;
    f.sig = f.noise = 0;
    f.lin = f.cn0_dbhz = f.weight = 0.0;
    if (ch.tag_valid != 0 && ch.n > 0 && R < ch.next_sample && R >= rec[0].sample) {
        // the last record whose sample is <= R: rec[lo].sample <= R < rec[hi].sample (hi == n: next_sample)
        int lo = 0, hi = ch.n;
        for (int k = 0; k < 32 && hi - lo > 1; ++k) {
            const int mid = lo + (hi - lo) / 2;
            if (rec[mid].sample <= R) lo = mid;
            else hi = mid;
        }
        const int32_t m = lo + 1 < a.par.epochs ? lo + 1 : a.par.epochs;
        const size_t hi_at = (size_t)c * ((size_t)a.max_epochs + 1) + (size_t)lo + 1, lo_at = hi_at - (size_t)m;
        const uint64_t A = a.sum_a[hi_at] - a.sum_a[lo_at];
        const uint64_t D = a.sum_d[hi_at] - a.sum_d[lo_at];
        const uint64_t N = a.sum_n[hi_at] - a.sum_n[lo_at];
        const uint64_t sig = A * A;
        const uint64_t noise = (uint64_t)m * D - sig;
        int32_t flags = (m == a.par.epochs ? GPSACQ_QUALITY_FULL : 0) | (m < a.par.min_epochs ? GPSACQ_QUALITY_SHORT : 0);
        const bool locked = D != 0 && (int64_t)(N * (uint64_t)a.par.lock_den) >= (int64_t)(D * (uint64_t)a.par.lock_num);
        if (!locked) flags |= GPSACQ_QUALITY_UNLOCKED;
        double lin = 0.0, db = 0.0;
        if (D == 0 || sig == 0) {
            flags |= GPSACQ_QUALITY_NO_POWER;
        } else if (noise == 0) {
            flags |= GPSACQ_QUALITY_SATURATED;
            lin = __builtin_inf();
            db = a.par.cn0_cap_dbhz;
        } else {
            const double snr = (double)sig / (double)noise;
            lin = snr * 1000.0;
            db = 10.0 * log10(lin);
        }
        double weight = 0.0;
        const bool gated = (flags & (GPSACQ_QUALITY_NO_POWER | GPSACQ_QUALITY_SHORT)) != 0 ||
                           ((flags & GPSACQ_QUALITY_UNLOCKED) != 0 && a.par.require_lock != 0) || lin < a.par.cn0_min_lin;
        if (!gated) {
            const double w = lin / a.par.cn0_ref_lin;
            weight = w < 1.0 ? w : 1.0;
        }
        f.epochs = m;
        f.flags = flags;
        f.sig = sig;
        f.noise = noise;
        f.lin = lin;
        f.cn0_dbhz = db;
        f.weight = weight;
    }
    const size_t idx = i * (size_t)a.n_chans + c;
    a.info[idx] = f;
    if (a.obs && a.obs[idx].valid != 0) a.obs[idx].weight = f.weight;
}

void launch_quality_acc(const QualityAccArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_quality_acc, dim3((unsigned)n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

void launch_quality_out(const QualityOutArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_quality_out, dim3((unsigned)((a.n_fix + SMOOTH_BLOCK - 1) / SMOOTH_BLOCK), (unsigned)a.n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

}  // namespace acq
