// nav_kernels.hip -- the satellite kernels, the plain position fix and the velocity solve of include/gpsacq.h, all in fp64, written
// on nav_device.hpp: "Navigation solver" (k_sat_state, k_fix) and "Velocity and clock drift" (k_sat_state_rate, k_vel).  The fixes
// that run the stage loop and the view from a fix are fix_kernels.hip's, which is built with another flag.
//
// k_sat_state: one lane per observation.  Clock correction at the uncorrected satellite time, then IS-GPS-200 Table 20-IV at the
// corrected one.  k_sat_state_rate, one lane per observation: the same evaluation (orbit_at), of which it forms the analytic time
// derivative and the clock drift.  k_fix: one lane per fix.  The row into registers, one Newton iteration (newton() without the pin
// on the set, see there) from the origin with the delays zero.  k_vel, one lane per fix: the row in registers -- every loop over it is unrolled to
// GPSACQ_FIX_MAX_SATS with the row length as a wave-uniform bound -- and one weighted least-squares solve -- the system is
// linear -- with the fix solver's Cholesky and pivot test.  No LDS, no barrier, no atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_device.hpp"

namespace acq {

namespace {
constexpr double MU = 3.986005e14;         // WGS-84 gravitational constant, m^3 / s^2
constexpr double F_REL = -4.442807633e-10; // relativistic term, s / sqrt(m)
constexpr double L1 = 1575.42e6;           // Hz
constexpr int KEPLER_PASSES = 30;

// eccentric anomaly at t_k seconds from t_oe: E = M + e sin E from E = M, until the step is below 1e-12
__device__ __forceinline__ double eccentric_anomaly(const NavEph& p, double n, double tk) {
    const double M = p.m_0 + n * tk;
    double E = M;
    for (int k = 0; k < KEPLER_PASSES; ++k) {
        const double prev = E;
        E = M + p.e * sin(E);
        if (fabs(E - prev) < 1e-12) break;
    }
    return E;
}

// the clock correction at the uncorrected satellite time and IS-GPS-200 Table 20-IV at the corrected one, up to the angles and
// the radius the position and its derivative are both formed from
struct Orbit {
    double tc, n, cE0;  // time from t_oc, mean motion, cos E at the uncorrected time: the clock drift's
    double dt, tk;      // clock correction; corrected time from t_oe
    double A, root, q;  // sqrt_a^2, sqrt(1 - e^2), 1 - e cos E
    double sE, s2, c2;  // sin E; sin, cos of twice the argument of latitude
    double r, su, cu, si, ci, so, co;
};

__device__ __forceinline__ Orbit orbit_at(const NavEph& p, int32_t tx_ms, double tx_frac) {
    Orbit o;
    const double tk0 = (double)fold_ms(tx_ms - p.toe_ms) * 1e-3 + tx_frac;  // uncorrected satellite time from t_oe ...
    o.tc = (double)fold_ms(tx_ms - p.toc_ms) * 1e-3 + tx_frac;              // ... and from t_oc
    o.A = p.sqrt_a * p.sqrt_a;
    o.n = sqrt(MU / (o.A * o.A * o.A)) + p.dn;
    double sE0, cE;
    sincos(eccentric_anomaly(p, o.n, tk0), &sE0, &o.cE0);
    o.dt = p.a_f0 + p.a_f1 * o.tc + p.a_f2 * o.tc * o.tc + F_REL * p.e * p.sqrt_a * sE0 - p.t_gd;
    o.tk = tk0 - o.dt;
    sincos(eccentric_anomaly(p, o.n, o.tk), &o.sE, &cE);
    o.q = 1.0 - p.e * cE;
    o.root = sqrt(1.0 - p.e * p.e);
    const double nu = atan2(o.root * o.sE, cE - p.e);
    const double phi = nu + p.omega;
    sincos(2.0 * phi, &o.s2, &o.c2);
    const double u = phi + p.c_us * o.s2 + p.c_uc * o.c2;
    o.r = o.A * o.q + p.c_rs * o.s2 + p.c_rc * o.c2;
    const double inc = p.i_0 + p.c_is * o.s2 + p.c_ic * o.c2 + p.idot * o.tk;
    const double om = p.omega_0 + (p.omega_dot - OMEGA_E) * o.tk - OMEGA_E * ((double)p.toe_ms * 1e-3);
    sincos(u, &o.su, &o.cu);
    sincos(inc, &o.si, &o.ci);
    sincos(om, &o.so, &o.co);
    return o;
}

__device__ __forceinline__ gpsacq_sat_state sat_state(const Orbit& o) {
    const double xp = o.r * o.cu, yp = o.r * o.su;
    gpsacq_sat_state st;
    st.x = xp * o.co - yp * o.ci * o.so;
    st.y = xp * o.so + yp * o.ci * o.co;
    st.z = yp * o.si;
    st.clock_corr = o.dt;
    return st;
}

// velocity (d / dt of Table 20-IV at the corrected time) and clock drift (at the uncorrected one), include/gpsacq.h
__device__ __forceinline__ gpsacq_sat_rate sat_state_rate(const NavEph& p, const Orbit& o) {
    const gpsacq_sat_state st = sat_state(o);
    const double Ed = o.n / o.q;
    const double nud = Ed * o.root / o.q;
    const double ud = nud * (1.0 + 2.0 * (p.c_us * o.c2 - p.c_uc * o.s2));
    const double rd = o.A * p.e * o.sE * Ed + 2.0 * nud * (p.c_rs * o.c2 - p.c_rc * o.s2);
    const double id = p.idot + 2.0 * nud * (p.c_is * o.c2 - p.c_ic * o.s2);
    const double omd = p.omega_dot - OMEGA_E;
    const double xp = o.r * o.cu, yp = o.r * o.su;
    const double xpd = rd * o.cu - yp * ud, ypd = rd * o.su + xp * ud;
    gpsacq_sat_rate out;
    out.vx = xpd * o.co - ypd * o.ci * o.so + yp * o.si * o.so * id - omd * st.y;
    out.vy = xpd * o.so + ypd * o.ci * o.co - yp * o.si * o.co * id + omd * st.x;
    out.vz = ypd * o.si + yp * o.ci * id;
    out.clock_drift = p.a_f1 + 2.0 * p.a_f2 * o.tc + F_REL * p.e * p.sqrt_a * o.cE0 * (o.n / (1.0 - p.e * o.cE0));
    return out;
}
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
    Normal n = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (mask >> s & 1) {
            const double w = ww[s], r = yy[s];
            const double wx = w * ux[s], wy = w * uy[s], wz = w * uz[s];
            n.a00 += wx * ux[s];
            n.a10 += wy * ux[s], n.a11 += wy * uy[s];
            n.a20 += wz * ux[s], n.a21 += wz * uy[s], n.a22 += wz * uz[s];
            n.a30 += wx, n.a31 += wy, n.a32 += wz, n.a33 += w;
            b0 += wx * r, b1 += wy * r, b2 += wz * r, b3 += w * r;
        }
    out.status = GPSACQ_VEL_SINGULAR;
    bool ok = false;
    double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    Normal l;
    if (factor4(n, l)) {
        solve4(l, b0, b1, b2, b3, d0, d1, d2, d3);
        ok = isfinite(d0) && isfinite(d1) && isfinite(d2) && isfinite(d3);
    }
    if (ok) {
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
        out.rms = sqrt(swrr / n.a33);
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
