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
// left where they are used it is 208 VGPRs, 59 SGPRs, no spill, two waves per SIMD.  No scratch either way.
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

__global__ __launch_bounds__(NAV_BLOCK) void k_coarse_fix(CoarseFixArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    gpsacq_obs* work = a.work + f * (size_t)a.sats;
    const gpsacq_coarse_prior pr = a.prior[f];
    const bool prior_ok = pr.rx_ms >= 0 && pr.rx_ms < WEEK_MS && isfinite(pr.x) && isfinite(pr.y) && isfinite(pr.z);

    // A. whole milliseconds, into work[]
    int ref = -1, n_used = 0;
    double delta = 0.0;
#pragma unroll 1
    for (int s = 0; s < a.sats; ++s) {
        const gpsacq_obs o = obs[s];
        gpsacq_obs w = {0, 0, 0, 0, 0.0, 0.0};
        if (prior_ok && usable(o, a.eph, a.n_eph) && o.tx_frac >= 0.0 && o.tx_frac < 1e-3) {
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
    gpsacq_fix out = blank_fix(GPSACQ_FIX_TOO_FEW, n_used);
    gpsacq_coarse_info info = {ref, 0, 0.0, 0.0, 0.0, 0.0};
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
    a.out[f] = out;
    a.info[f] = info;
}

void launch_coarse_obs(const CoarseObsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_obs, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_coarse_fix(const CoarseFixArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_fix, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
