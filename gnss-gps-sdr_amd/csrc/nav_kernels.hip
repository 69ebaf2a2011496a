// nav_kernels.hip -- the satellite kernels, the plain position fix and the velocity solve of include/gpsacq.h, all in fp64, written
// on nav_device.hpp and orbit_device.hpp (the orbit evaluation, shared with coarse_kernels.hip): "Navigation solver" (k_sat_state,
// k_fix) and "Velocity and clock drift" (k_sat_state_rate, k_vel).  The fixes that run the stage loop and the view from a fix are
// fix_kernels.hip's, which is built with another flag.
//
// k_sat_state: one lane per observation.  Clock correction at the uncorrected satellite time, then IS-GPS-200 Table 20-IV at the
// corrected one.  k_sat_state_rate, one lane per observation: the same evaluation (orbit_at), of which it forms the analytic time
// derivative and the clock drift.  k_fix: one lane per fix.  The row into registers, one Newton iteration (newton() without the pin
// on the set, see there) from the origin with the delays zero.  k_vel, one lane per fix: the row in registers -- every loop over it is unrolled to
// GPSACQ_FIX_MAX_SATS with the row length as a wave-uniform bound -- and one weighted least-squares solve -- the system is
// linear -- with the fix solver's Cholesky and pivot test (add_row, factor and solve of spd_device.hpp, N = 4).  No LDS, no barrier, no atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_device.hpp"
#include "orbit_device.hpp"

namespace acq {

namespace {
constexpr double L1 = 1575.42e6;  // Hz
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_state(SatStateArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_obs o = a.obs[i];
    gpsacq_sat_state st = {0.0, 0.0, 0.0, 0.0};
    if (usable(o, a.eph, a.n_eph)) st = sat_state(orbit_at(a.eph[o.eph], o.tx_ms, o.tx_frac));
    a.out[i] = st;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_fix(FixArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    Row r;
    load_row(a, f, r);
    gpsacq_fix out = blank_fix(GPSACQ_FIX_TOO_FEW, r.n_used);
    if (r.n_used >= 4) {
        State st = {0.0, 0.0, 0.0, 0.0, r.t0, 0.0};
        out.status = GPSACQ_FIX_NO_CONVERGE;
        if (newton<false>(r, r.mask, st, out.iterations)) {
            out.status = GPSACQ_FIX_OK;
            double lat, lon, alt;
            geodetic(st.x, st.y, st.z, lat, lon, alt);
            fill_fix(out, r, st, lat, lon, alt);
        }
    }
    a.out[f] = out;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_state_rate(SatRateArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_obs o = a.obs[i];
    gpsacq_sat_rate r = {0.0, 0.0, 0.0, 0.0};
    if (usable(o, a.eph, a.n_eph)) r = sat_state_rate(a.eph[o.eph], orbit_at(a.eph[o.eph], o.tx_ms, o.tx_frac));
    a.out[i] = r;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_vel(VelArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    const gpsacq_fix fix = a.fix[f];
    gpsacq_vel out;
    out.status = GPSACQ_VEL_NO_FIX;
    out.n_used = 0;
    out.vx = out.vy = out.vz = out.ve = out.vn = out.vu = out.drift = out.rms = 0.0;
    if (fix.status != GPSACQ_FIX_OK) {
        a.out[f] = out;
        return;
    }
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    const gpsacq_rate_obs* robs = a.rate_obs + f * (size_t)a.sats;
    const gpsacq_sat_state* state = a.state + f * (size_t)a.sats;
    const gpsacq_sat_rate* rate = a.rate + f * (size_t)a.sats;

    // the row into registers: unit vector satellite -> receiver, right-hand side, weight
    double ux[S], uy[S], uz[S], yy[S], ww[S];
    uint32_t mask = 0;
    int n_used = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ux[s] = uy[s] = uz[s] = yy[s] = ww[s] = 0.0;
        if (s < a.sats) {
            const gpsacq_obs o = obs[s];
            const gpsacq_rate_obs ro = robs[s];
            if (usable(o, a.eph, a.n_eph) && ro.valid != 0 && ro.weight >= 0.0 && isfinite(ro.weight) && isfinite(ro.doppler_hz)) {
                const gpsacq_sat_state st = state[s];
                const gpsacq_sat_rate sr = rate[s];
                double sn, cs;
                earth_turn(o, st, fix, sn, cs);
                const double rx = st.x * cs - st.y * sn, ry = st.x * sn + st.y * cs;
                const double wx = sr.vx - OMEGA_E * st.y, wy = sr.vy + OMEGA_E * st.x;  // v_s + Omega_e x r_s
                const double vx = wx * cs - wy * sn, vy = wx * sn + wy * cs, vz = sr.vz;
                const double dx = fix.x - rx, dy = fix.y - ry, dz = fix.z - st.z;
                const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
                ux[s] = dx * inv, uy[s] = dy * inv, uz[s] = dz * inv;
                // e = -u:  rho_dot - e . (v_i - Omega_e x r_r) + c clock_drift_i  =  -e . v_r + c drift_r
                const double rel = ux[s] * (vx + OMEGA_E * fix.y) + uy[s] * (vy - OMEGA_E * fix.x) + uz[s] * vz;
                yy[s] = -(C / L1) * ro.doppler_hz + rel + C * sr.clock_drift;
                ww[s] = ro.weight;
                mask |= 1u << s;
                n_used += 1;
            }
        }
    }
    out.n_used = n_used;
    if (n_used < 4) {
        out.status = GPSACQ_VEL_TOO_FEW;
        a.out[f] = out;
        return;
    }
    // weighted normal equations of the rows h = (ux, uy, uz, 1), as in newton()
    Sym<4> n = {}, l;
    double b[4] = {}, d[4] = {};
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (mask >> s & 1) {
            const double h[4] = {ux[s], uy[s], uz[s], 1.0};
            add_row(n, b, h, ww[s], yy[s]);
        }
    out.status = GPSACQ_VEL_SINGULAR;
    bool ok = false;
    if (factor(n, l)) {
        solve(l, b, d);
        ok = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && isfinite(d[3]);
    }
    if (ok) {
        const double d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
        double swrr = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (mask >> s & 1) {
                const double res = yy[s] - (ux[s] * d0 + uy[s] * d1 + uz[s] * d2 + d3);
                swrr += ww[s] * res * res;
            }
        double sl, cl, sp, cp;
        sincos(fix.lon, &sl, &cl);
        sincos(fix.lat, &sp, &cp);
        out.status = GPSACQ_VEL_OK;
        out.vx = d0, out.vy = d1, out.vz = d2;
        out.ve = -sl * d0 + cl * d1;
        out.vn = -sp * cl * d0 - sp * sl * d1 + cp * d2;
        out.vu = cp * cl * d0 + cp * sl * d1 + sp * d2;
        out.drift = d3 / C;
        out.rms = sqrt(swrr / n(3, 3));
    }
    a.out[f] = out;
}

void launch_sat_state(const SatStateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_state, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_fix(const FixArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fix, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_sat_state_rate(const SatRateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_state_rate, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_vel(const VelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_vel, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
