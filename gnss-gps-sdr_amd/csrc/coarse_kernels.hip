// coarse_kernels.hip -- "Coarse-time fixes: positions from code phases alone" of include/gpsacq.h, in fp64, written on
// nav_device.hpp (constants, usable(), geodetic(), blank_fix(), and through it spd_device.hpp, the Cholesky piece) and orbit_device.hpp (the one orbit evaluation).
//
// k_coarse_obs: one lane per (fix, channel), a search peak into an observation that carries only the sub-millisecond part.
// k_coarse_fix: one lane per fix, steps A, B and C of the text.  Unlike k_fix it holds NOTHING of the row in registers: twelve
// satellites x (position, velocity, time, weight) indexed by a run-time column would go to scratch, and the satellites move with
// the fifth unknown, so their states have to be evaluated again every pass anyway.  The satellite loop is ONE body (#pragma
// unroll 1) that reads the observation from `work` (the caller's obs_out or engine scratch, where step A left eph, the whole
// milliseconds N_k, f_k and the weight: 32 bytes that are cache hits after the first pass), evaluates the orbit, and adds into the
// 15 + 5 sums of the normal equations (a Sym<5> of spd_device.hpp, whose factor, solve and inverse the passes end with).  The pass that follows the last step runs the same body once more with unit weights: the
// sums are then H^T H of the dilution figures at the final state, and the observations go out with their full transmit times.
// So the orbit code is inlined twice in the kernel: the two passes of step A (one body) and the Newton body.
// No LDS, no barrier, no atomics; every loop is bounded.  Lanes diverge on the pass count and on Kepler's iteration, which is
// accepted as in newton() (a fix is 4-6 passes).
// Built with -mllvm -disable-machine-licm (Makefile), as fix_kernels.hip is and for its reason: hoisted out of the pass loop the
// fp64 constants of the inlined libm take k_coarse_fix to 256 VGPRs + 12 AGPRs with 12 scalar registers spilled, one wave per SIMD;
// left where they are used it is 206 VGPRs, 59 SGPRs, no spill, two waves per SIMD.  No scratch either way.
//
// "Coarse-time fix integrity" of include/gpsacq.h runs behind k_coarse_fix: the solve is ONE device function, coarse_solve<SKIP>,
// which k_coarse_fix instantiates with no column to skip and k_coarse_exclude (sixteen lanes per fix, lane k the candidate without
// column k, each in a work row of its own) with one.  k_coarse_exclude: 226 VGPRs, 0 AGPRs, 85 SGPRs, no scratch, no LDS, two
// waves per SIMD.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coarse_launch.hpp"
#include "nav_device.hpp"
#include "orbit_device.hpp"

namespace acq {

namespace {
// ---- time (split() and week_ms() are nav_device.hpp's) ---------------------------------------------------------------------------
// nearbyint as an int32; what is no count of milliseconds near t0 (beyond 1e6, or not finite) is 0, as in week_ms
__device__ __forceinline__ int32_t whole(double x) {
    const double n = nearbyint(x);
    return fabs(n) < 1e6 ? (int32_t)n : 0;
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_coarse_obs(CoarseObsArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_peak pk = a.peaks[i];
    gpsacq_obs o = {0, 0, 0, 0, 0.0, 0.0};
    if ((double)pk.snr >= a.snr_min && pk.ca_shift >= 0 && (double)pk.ca_shift < a.fs / 1000.0) {
        o.eph = (int32_t)(i % (size_t)a.chans);
        o.valid = 1;
        o.tx_frac = (double)pk.ca_shift / a.fs;
        o.weight = 1.0;
    }
    a.out[i] = o;
}

// Steps A, B and C for one row: `work` is the row's [sats] records, where step A leaves eph, the whole milliseconds N_k, f_k and the
// weight and the last pass the observations with their full transmit times.  SKIP: column `skip` is taken as not usable, the one
// difference between an exclusion candidate of k_coarse_exclude and the fix itself (k_coarse_fix: SKIP false, skip unread).
template <bool SKIP>
__device__ __forceinline__ void coarse_solve(const CoarseFixArgs& a, const gpsacq_obs* obs, gpsacq_obs* work, const gpsacq_coarse_prior& pr,
                                             int skip, gpsacq_fix& out, gpsacq_coarse_info& info) {
    const bool prior_ok = pr.rx_ms >= 0 && pr.rx_ms < WEEK_MS && isfinite(pr.x) && isfinite(pr.y) && isfinite(pr.z);

    // A. whole milliseconds, into work[]
    int ref = -1, n_used = 0;
    double delta = 0.0;
#pragma unroll 1
    for (int s = 0; s < a.sats; ++s) {
        const gpsacq_obs o = obs[s];
        gpsacq_obs w = {0, 0, 0, 0, 0.0, 0.0};
        if (prior_ok && (!SKIP || s != skip) && usable(o, a.eph, a.n_eph) && o.tx_frac >= 0.0 && o.tx_frac < 1e-3) {
            const NavEph& p = a.eph[o.eph];
            double tau = 75e-3, cc = 0.0;
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {  // at -75 ms, then at -tau
                double k, frac, sn, cs;
                split(-tau, k, frac);
                const gpsacq_sat_state st = sat_state(orbit_at(p, week_ms(pr.rx_ms, k), frac));
                sincos(-OMEGA_E * tau, &sn, &cs);
                const double dx = pr.x - (st.x * cs - st.y * sn), dy = pr.y - (st.x * sn + st.y * cs), dz = pr.z - st.z;
                tau = sqrt(dx * dx + dy * dy + dz * dz) / C;
                cc = st.clock_corr;
            }
            const double P = cc - tau;
            const int32_t N = whole(((ref < 0 ? 0.0 : delta) + P - o.tx_frac) * 1e3);
            if (ref < 0) {
                ref = s;
                delta = (double)N * 1e-3 + o.tx_frac - P;
            }
            w.eph = o.eph, w.valid = 1, w.tx_ms = N, w.tx_frac = o.tx_frac, w.weight = o.weight;
            n_used += 1;
        }
        work[s] = w;
    }

    // B. five unknowns
    out = blank_fix(GPSACQ_FIX_TOO_FEW, n_used);
    info = {ref, 0, 0.0, 0.0, 0.0, 0.0};
    double x = pr.x, y = pr.y, z = pr.z, b = 0.0, sc = 0.0, rms = 0.0;
    bool ok = false;
    if (n_used >= 5) {
        out.status = GPSACQ_FIX_NO_CONVERGE;
        bool last = false;  // the pass after the last step: H^T H of the dilution figures, and the observations out
#pragma unroll 1
        for (int pass = 0; pass <= FIX_PASSES; ++pass) {
            if (!last && pass == FIX_PASSES) break;
            Sym<5> n = {};
            double g[5] = {}, swrr = 0.0, sw = 0.0;
#pragma unroll 1
            for (int s = 0; s < a.sats; ++s) {
                const gpsacq_obs o = work[s];
                if (!o.valid) continue;
                const double w = last ? (o.weight > 0.0 ? 1.0 : 0.0) : o.weight;
                double k, frac, sn, cs;
                split(o.tx_frac + sc, k, frac);  // the uncorrected time T_k + s, from t0
                const int32_t ms = week_ms(pr.rx_ms, (double)o.tx_ms + k);
                const NavEph& p = a.eph[o.eph];
                const Orbit orb = orbit_at(p, ms, frac);
                const gpsacq_sat_state st = sat_state(orb);
                const gpsacq_sat_rate sr = sat_state_rate(p, orb);
                const double rho = C * (st.clock_corr - ((double)o.tx_ms * 1e-3 + o.tx_frac)) - b;
                sincos(-OMEGA_E * rho / C, &sn, &cs);
                const double dx = x - (st.x * cs - st.y * sn), dy = y - (st.x * sn + st.y * cs), dz = z - st.z;
                const double range = sqrt(dx * dx + dy * dy + dz * dz);
                const double inv = 1.0 / range;
                const double res = rho - range;
                double h[5];
                h[0] = dx * inv, h[1] = dy * inv, h[2] = dz * inv, h[3] = 1.0;
                h[4] = -(C * sr.clock_drift + h[0] * (sr.vx * cs - sr.vy * sn) + h[1] * (sr.vx * sn + sr.vy * cs) + h[2] * sr.vz);
                add_row(n, g, h, w, res);
                swrr += w * res * res;
                sw += w;
                if (last) {  // C: the observation with its full transmit time
                    gpsacq_obs v = o;
                    v.tx_ms = ms, v.tx_frac = frac;
                    work[s] = v;
                }
            }
            Sym<5> l;
            if (last) {
                if (factor(n, l)) {
                    Sym<5> m;
                    double q[5];
                    inverse_lower(l, m);
                    inverse_diagonal(m, q);
                    const double pd = sqrt(q[0] + q[1] + q[2]), cd = sqrt(q[4]);
                    if (isfinite(pd) && isfinite(cd)) info.pdop = pd, info.cdop = cd;
                }
                ok = true;
                break;
            }
            rms = sqrt(swrr / sw);
            if (!factor(n, l)) break;
            double d[5];
            solve(l, g, d);
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (!isfinite(step) || !isfinite(d[3]) || !isfinite(d[4])) break;
            x += d[0], y += d[1], z += d[2], b += d[3], sc += d[4];
            out.iterations += 1;
            if (!(fabs(sc) < 302400.0)) break;  // half a week: no correction of a prior, and the times above stay integers
            if (step < 1e-4 && fabs(d[4]) < 1e-7) last = true;  // the step just applied was the last one
        }
    }

    // C. records
    if (ok) {
        double k, frac;
        split(sc - b / C, k, frac);
        out.status = GPSACQ_FIX_OK;
        out.rx_ms = week_ms(pr.rx_ms, k);
        out.rx_frac = frac;
        out.x = x, out.y = y, out.z = z;
        out.rms = rms;
        geodetic(x, y, z, out.lat, out.lon, out.alt);
        info.coarse_s = sc;
        info.bias_m = b;
        if (n_used >= 6 && rms > a.p.rms_max_m) info.flags |= GPSACQ_COARSE_INCONSISTENT;
    } else {
        const gpsacq_obs none = {0, 0, 0, 0, 0.0, 0.0};
#pragma unroll 1
        for (int s = 0; s < a.sats; ++s) work[s] = none;
    }
}

__global__ __launch_bounds__(NAV_BLOCK) void k_coarse_fix(CoarseFixArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    const gpsacq_coarse_prior pr = a.prior[f];
    gpsacq_fix out;
    gpsacq_coarse_info info;
    coarse_solve<false>(a, a.obs + f * (size_t)a.sats, a.work + f * (size_t)a.sats, pr, -1, out, info);
    a.out[f] = out;
    a.info[f] = info;
}

// "Coarse-time fix integrity", steps TEST, EXCLUDE and EXCLUDED, behind k_coarse_fix (FULL).  Sixteen lanes per fix, four fixes
// per wave64.  Every lane of a group reads FULL's record and sums W and n_w over the caller's row (the same addresses across the
// group), so the test is made sixteen times and no lane has to tell another its outcome; a group whose row needs no exclusion
// writes its raim record from lane 0 and returns.  Otherwise lane k solves the row without column k where k is a candidate, in
// a work row of its own (the whole milliseconds of a candidate that drops the reference column are not FULL's), the smallest
// (T_k, k) and the count meet in a butterfly of width 16, and the winning lane writes the three records and copies its row out.
__global__ __launch_bounds__(NAV_BLOCK) void k_coarse_exclude(CoarseRaimArgs a) {
    const size_t lane = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    const size_t f = lane / COARSE_GROUP;
    const int k = (int)(lane % COARSE_GROUP);
    if (f >= a.fix.n_fix) return;
    const int sats = a.fix.sats;
    const gpsacq_obs* obs = a.fix.obs + f * (size_t)sats;
    gpsacq_fix_raim raim;
    raim.status = GPSACQ_RAIM_NONE;
    raim.dof = 0, raim.excluded = -1, raim.n_candidates = 0;
    raim.stat_full = raim.stat = raim.threshold = 0.0;
    const int full_status = a.fix.out[f].status, full_steps = a.fix.out[f].iterations;
    const double full_rms = a.fix.out[f].rms;
    if (full_status != GPSACQ_FIX_OK) {  // the same for the sixteen lanes of a group, as every return before the butterfly
        if (k == 0) a.raim[f] = raim;
        return;
    }

    // TEST.  FULL is GPSACQ_FIX_OK, so the prior named an instant and the usable columns are those step A took
    double W = 0.0, wk = 0.0;
    int n_w = 0;
    bool cand = false;
#pragma unroll 1
    for (int s = 0; s < sats; ++s) {
        const gpsacq_obs o = obs[s];
        if (!usable(o, a.fix.eph, a.fix.n_eph) || !(o.tx_frac >= 0.0 && o.tx_frac < 1e-3)) continue;
        W += o.weight;
        if (!(o.weight > 0.0)) continue;
        n_w += 1;
        if (s == k) cand = true, wk = o.weight;
    }
    const double sigma2 = a.r.sigma_m * a.r.sigma_m;
    const int d = n_w - 5;
    const double T = full_rms * full_rms * W / sigma2;
    raim.dof = d;
    raim.stat_full = raim.stat = T;
    // d <= GPSACQ_FIX_MAX_SATS - 5; selects over the table, not an index: thr = threshold[d - 1], thr2 = threshold[d - 2]
    double thr = a.r.threshold[0], thr2 = a.r.threshold[0];
#pragma unroll
    for (int j = 1; j < GPSACQ_RAIM_MAX_DOF; ++j) {
        thr = d == j + 1 ? a.r.threshold[j] : thr;
        thr2 = d - 1 == j + 1 ? a.r.threshold[j] : thr2;
    }
    bool go = false;
    if (d < 1) {
        raim.status = GPSACQ_RAIM_UNCHECKED;
    } else {
        raim.threshold = thr;
        raim.status = T <= thr ? GPSACQ_RAIM_PASS : GPSACQ_RAIM_FAILED;
        go = !(T <= thr) && a.r.exclude && d >= 2;
    }
    if (!go) {
        if (k == 0) a.raim[f] = raim;
        return;
    }

    // EXCLUDE
    gpsacq_obs* work = a.cand + (f * (size_t)sats + (size_t)k) * (size_t)sats;  // k < sats wherever it is written
    gpsacq_fix out;
    gpsacq_coarse_info info;
    double best = INFINITY;
    int count = 0;
    if (cand) {
        const gpsacq_coarse_prior pr = a.fix.prior[f];
        coarse_solve<true>(a.fix, obs, work, pr, k, out, info);
        if (out.status == GPSACQ_FIX_OK) {
            count = 1;
            best = out.rms * out.rms * (W - wk) / sigma2;
            if (!(best < INFINITY)) best = INFINITY;  // a NaN is no candidate's statistic
        }
    }
    const double stat = best;
    int best_k = k;
    // the smallest T_k of the group, on a tie the lowest k: a butterfly over the sixteen lanes, every lane ends with the result
#pragma unroll
    for (int off = 1; off < COARSE_GROUP; off <<= 1) {
        const double ot = __shfl_xor(best, off, COARSE_GROUP);
        const int ok = __shfl_xor(best_k, off, COARSE_GROUP);
        count += __shfl_xor(count, off, COARSE_GROUP);
        if (ot < best || (ot == best && ok < best_k)) best = ot, best_k = ok;
    }
    raim.n_candidates = count;
    if (!(best <= thr2)) {  // FAILED stands, with the full solution
        if (k == 0) a.raim[f] = raim;
        return;
    }
    if (k != best_k) return;

    // EXCLUDED: the winning lane, the row's three records and its observations
    out.iterations += full_steps;
    raim.status = GPSACQ_RAIM_EXCLUDED;
    raim.dof = d - 1;
    raim.excluded = k;
    raim.stat = stat;
    raim.threshold = thr2;
    a.fix.out[f] = out;
    a.fix.info[f] = info;
    a.raim[f] = raim;
    if (a.obs_out) {
        gpsacq_obs* dst = a.obs_out + f * (size_t)sats;
#pragma unroll 1
        for (int s = 0; s < sats; ++s) dst[s] = work[s];
    }
}

void launch_coarse_obs(const CoarseObsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_obs, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_coarse_fix(const CoarseFixArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_fix, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_coarse_exclude(const CoarseRaimArgs& a, hipStream_t s) {
    const size_t lanes = a.fix.n_fix * COARSE_GROUP;
    hipLaunchKernelGGL(k_coarse_exclude, dim3((unsigned)((lanes + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
