// orbit_device.hpp -- the orbit evaluation of include/gpsacq.h ("Navigation solver", SATELLITE STATE; "Velocity and clock drift",
// SATELLITE RATE), once, in fp64: nav_kernels.hip (k_sat_state, k_sat_state_rate), coarse_kernels.hip (k_coarse_fix),
// doppler_kernels.hip (k_doppler_fix) and aided_kernels.hip (k_aid_predict) include it, nothing else does.  Clock correction at
// the uncorrected satellite time, IS-GPS-200 Table 20-IV at the corrected one, and the analytic time derivative of both.  Every
// loop is bounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_device.hpp"

namespace acq {

constexpr double MU = 3.986005e14;         // WGS-84 gravitational constant, m^3 / s^2
constexpr double F_REL = -4.442807633e-10; // relativistic term, s / sqrt(m)
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

}  // namespace acq
