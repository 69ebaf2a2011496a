// nav_kernels.hip -- the navigation solver of include/gpsacq.h ("Navigation solver"): satellite state and batched position fixes,
// all in fp64.
//
// k_sat_state: one lane per observation.  Clock correction at the uncorrected satellite time, then IS-GPS-200 Table 20-IV at the
// corrected one.  k_fix: one lane per fix.  Its up-to-12 satellites (position, corrected transmit time as an offset from the fix's
// earliest millisecond, weight) sit in registers -- every loop over them is unrolled to GPSACQ_FIX_MAX_SATS with the row length as
// a wave-uniform bound -- and the lane runs its own Newton iteration: lanes that converge in different pass counts diverge, which
// is accepted (a fix is ~6 passes).  No LDS, no barrier, no atomics; every loop is bounded, so a bad fix ends, it never spins.
//
// "Velocity and clock drift" of the same header: k_sat_state_rate, one lane per observation, repeats k_sat_state's position (its
// own copy of the arithmetic, so that k_sat_state's code and output stay what they were) and adds the analytic time derivative
// and the clock drift.  k_vel, one lane per fix: the row in registers as in k_fix, one weighted least-squares solve -- the system is
// linear -- with k_fix's Cholesky and pivot test.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_launch.hpp"

namespace acq {

namespace {
constexpr double NAV_MU = 3.986005e14;            // WGS-84 gravitational constant, m^3 / s^2
constexpr double NAV_OMEGA_E = 7.2921151467e-5;   // earth rotation rate, rad / s
constexpr double NAV_C = 2.99792458e8;            // m / s
constexpr double NAV_F = -4.442807633e-10;        // relativistic term, s / sqrt(m)
constexpr double NAV_L1 = 1575.42e6;              // Hz
constexpr int32_t NAV_WEEK_MS = 604800000;
constexpr double WGS84_A = 6378137.0;
constexpr double WGS84_E2 = 0.00669437999014132;
constexpr int KEPLER_PASSES = 30, FIX_PASSES = 20, GEODETIC_PASSES = 10;

// difference of two milliseconds of week, folded into half a week either way
__device__ __forceinline__ int32_t fold_ms(int32_t d) {
    if (d > NAV_WEEK_MS / 2) d -= NAV_WEEK_MS;
    else if (d < -NAV_WEEK_MS / 2) d += NAV_WEEK_MS;
    return d;
}

__device__ __forceinline__ bool usable(const gpsacq_obs& o, const NavEph* eph, int n_eph) {
    if (!o.valid || o.eph < 0 || o.eph >= n_eph) return false;
    if (!(o.weight >= 0.0) || !isfinite(o.weight) || !isfinite(o.tx_frac)) return false;
    return eph[o.eph].valid != 0;
}

// eccentric anomaly at t_k seconds from t_oe: E = M + e sin E from E = M, until the step is below 1e-12
__device__ __forceinline__ double eccentric_anomaly(const NavEph& p, double tk) {
    const double A = p.sqrt_a * p.sqrt_a;
    const double n = sqrt(NAV_MU / (A * A * A)) + p.dn;
    const double M = p.m_0 + n * tk;
    double E = M;
    for (int k = 0; k < KEPLER_PASSES; ++k) {
        const double prev = E;
        E = M + p.e * sin(E);
        if (fabs(E - prev) < 1e-12) break;
    }
    return E;
}

__device__ __forceinline__ gpsacq_sat_state sat_state(const NavEph& p, int32_t tx_ms, double tx_frac) {
    const double tk0 = (double)fold_ms(tx_ms - p.toe_ms) * 1e-3 + tx_frac;  // uncorrected satellite time from t_oe ...
    const double tc = (double)fold_ms(tx_ms - p.toc_ms) * 1e-3 + tx_frac;   // ... and from t_oc
    const double dt = p.a_f0 + p.a_f1 * tc + p.a_f2 * tc * tc + NAV_F * p.e * p.sqrt_a * sin(eccentric_anomaly(p, tk0)) - p.t_gd;
    const double tk = tk0 - dt;
    // IS-GPS-200 Table 20-IV
    const double A = p.sqrt_a * p.sqrt_a;
    const double E = eccentric_anomaly(p, tk);
    double sE, cE;
    sincos(E, &sE, &cE);
    const double nu = atan2(sqrt(1.0 - p.e * p.e) * sE, cE - p.e);
    const double phi = nu + p.omega;
    double s2, c2;
    sincos(2.0 * phi, &s2, &c2);
    const double u = phi + p.c_us * s2 + p.c_uc * c2;
    const double r = A * (1.0 - p.e * cE) + p.c_rs * s2 + p.c_rc * c2;
    const double inc = p.i_0 + p.c_is * s2 + p.c_ic * c2 + p.idot * tk;
    double su, cu, si, ci, so, co;
    sincos(u, &su, &cu);
    sincos(inc, &si, &ci);
    const double om = p.omega_0 + (p.omega_dot - NAV_OMEGA_E) * tk - NAV_OMEGA_E * ((double)p.toe_ms * 1e-3);
    sincos(om, &so, &co);
    const double xp = r * cu, yp = r * su;
    gpsacq_sat_state st;
    st.x = xp * co - yp * ci * so;
    st.y = xp * so + yp * ci * co;
    st.z = yp * si;
    st.clock_corr = dt;
    return st;
}

// velocity (d / dt of Table 20-IV at the corrected time) and clock drift (at the uncorrected one), include/gpsacq.h
__device__ __forceinline__ gpsacq_sat_rate sat_state_rate(const NavEph& p, int32_t tx_ms, double tx_frac) {
    const double tk0 = (double)fold_ms(tx_ms - p.toe_ms) * 1e-3 + tx_frac;
    const double tc = (double)fold_ms(tx_ms - p.toc_ms) * 1e-3 + tx_frac;
    const double A = p.sqrt_a * p.sqrt_a;
    const double n = sqrt(NAV_MU / (A * A * A)) + p.dn;
    const double E0 = eccentric_anomaly(p, tk0);
    double sE0, cE0;
    sincos(E0, &sE0, &cE0);
    const double dt = p.a_f0 + p.a_f1 * tc + p.a_f2 * tc * tc + NAV_F * p.e * p.sqrt_a * sE0 - p.t_gd;
    const double tk = tk0 - dt;
    const double E = eccentric_anomaly(p, tk);
    double sE, cE;
    sincos(E, &sE, &cE);
    const double q = 1.0 - p.e * cE;
    const double root = sqrt(1.0 - p.e * p.e);
    const double nu = atan2(root * sE, cE - p.e);
    const double phi = nu + p.omega;
    double s2, c2;
    sincos(2.0 * phi, &s2, &c2);
    const double u = phi + p.c_us * s2 + p.c_uc * c2;
    const double r = A * q + p.c_rs * s2 + p.c_rc * c2;
    const double inc = p.i_0 + p.c_is * s2 + p.c_ic * c2 + p.idot * tk;
    const double om = p.omega_0 + (p.omega_dot - NAV_OMEGA_E) * tk - NAV_OMEGA_E * ((double)p.toe_ms * 1e-3);
    double su, cu, si, ci, so, co;
    sincos(u, &su, &cu);
    sincos(inc, &si, &ci);
    sincos(om, &so, &co);
    // the derivatives
    const double Ed = n / q;
    const double nud = Ed * root / q;
    const double ud = nud * (1.0 + 2.0 * (p.c_us * c2 - p.c_uc * s2));
    const double rd = A * p.e * sE * Ed + 2.0 * nud * (p.c_rs * c2 - p.c_rc * s2);
    const double id = p.idot + 2.0 * nud * (p.c_is * c2 - p.c_ic * s2);
    const double omd = p.omega_dot - NAV_OMEGA_E;
    const double xp = r * cu, yp = r * su;
    const double xpd = rd * cu - yp * ud, ypd = rd * su + xp * ud;
    const double x = xp * co - yp * ci * so;
    const double y = xp * so + yp * ci * co;
    gpsacq_sat_rate out;
    out.vx = xpd * co - ypd * ci * so + yp * si * so * id - omd * y;
    out.vy = xpd * so + ypd * ci * co - yp * si * co * id + omd * x;
    out.vz = ypd * si + yp * ci * id;
    out.clock_drift = p.a_f1 + 2.0 * p.a_f2 * tc + NAV_F * p.e * p.sqrt_a * cE0 * (n / (1.0 - p.e * cE0));
    return out;
}

// LatLonAlt(), c/solve.cpp:273-293, bounded
__device__ __forceinline__ void geodetic(double x, double y, double z, double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)  // the three copies of this function give the same bits whatever kernel they are inlined into
    const double p = sqrt(x * x + y * y);
    if (!(p > 1e-6)) {  // on the axis: p / cos(lat) is 0 / 0
        lon = 0.0;
        lat = z < 0 ? -1.5707963267948966 : 1.5707963267948966;
        alt = fabs(z) - WGS84_A * sqrt(1.0 - WGS84_E2);
        return;
    }
    // tan(lon / 2) = y / (x + p) = (p - x) / y: the form whose sum does not cancel.  With x < 0 the first one loses x + p to rounding
    // next to the antimeridian and is 0 / 0 on it (y == 0: lon = pi, in (-pi, pi])
    if (x >= 0.0) {
        lon = 2.0 * atan2(y, x + p);
    } else {
        const double half = 2.0 * atan2(p - x, fabs(y));
        lon = y < 0.0 ? -half : half;
    }
    lat = atan(z / (p * (1.0 - WGS84_E2)));
    alt = 0.0;
    for (int k = 0; k < GEODETIC_PASSES; ++k) {
        const double prev = alt;
        const double sl = sin(lat);
        const double N = WGS84_A / sqrt(1.0 - WGS84_E2 * sl * sl);
        alt = p / cos(lat) - N;
        lat = atan(z / (p * (1.0 - WGS84_E2 * N / (N + alt))));
        if (fabs(alt - prev) < 1e-9) break;
    }
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_state(SatStateArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_obs o = a.obs[i];
    gpsacq_sat_state st = {0.0, 0.0, 0.0, 0.0};
    if (usable(o, a.eph, a.n_eph)) st = sat_state(a.eph[o.eph], o.tx_ms, o.tx_frac);
    a.out[i] = st;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_fix(FixArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    constexpr int S = GPSACQ_FIX_MAX_SATS;
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    const gpsacq_sat_state* state = a.state + f * (size_t)a.sats;

    // the row into registers; times first as whole milliseconds from the first usable observation
    double sx[S], sy[S], sz[S], tt[S], ww[S];
    int32_t dms[S];
    uint32_t mask = 0;
    int n_used = 0;
    int32_t ms_first = 0, dmin = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        sx[s] = sy[s] = sz[s] = tt[s] = ww[s] = 0.0;
        dms[s] = 0;
        if (s < a.sats) {
            const gpsacq_obs o = obs[s];
            if (usable(o, a.eph, a.n_eph)) {
                const gpsacq_sat_state st = state[s];
                if (!n_used) ms_first = o.tx_ms;
                dms[s] = fold_ms(o.tx_ms - ms_first);
                dmin = dms[s] < dmin ? dms[s] : dmin;
                sx[s] = st.x, sy[s] = st.y, sz[s] = st.z;
                tt[s] = o.tx_frac - st.clock_corr;
                ww[s] = o.weight;
                mask |= 1u << s;
                n_used += 1;
            }
        }
    }

    gpsacq_fix out;
    out.status = GPSACQ_FIX_TOO_FEW;
    out.n_used = n_used;
    out.iterations = 0;
    out.rx_ms = 0;
    out.rx_frac = out.x = out.y = out.z = out.lat = out.lon = out.alt = out.rms = 0.0;
    if (n_used < 4) {
        a.out[f] = out;
        return;
    }

    // corrected transmit times as offsets from the earliest millisecond of the row; the receive time starts 75 ms after their mean
    double t0 = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (mask >> s & 1) {
            tt[s] += (double)(dms[s] - dmin) * 1e-3;
            t0 += tt[s];
        }
    t0 = t0 / (double)n_used + 75e-3;

    double x = 0.0, y = 0.0, z = 0.0, bias = 0.0;  // bias: metres of light time taken off t0
    double trx = t0, rms = 0.0;
    int status = GPSACQ_FIX_NO_CONVERGE, steps = 0;
    for (int pass = 0; pass < FIX_PASSES; ++pass) {
        trx = t0 - bias / NAV_C;
        // weighted normal equations of the rows h = (ux, uy, uz, 1): lower triangle of A = sum w h h^T, b = sum w h r
        double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
        double b0 = 0, b1 = 0, b2 = 0, b3 = 0, swrr = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (mask >> s & 1) {
                double sn, cs;
                sincos(NAV_OMEGA_E * (tt[s] - trx), &sn, &cs);
                const double dx = x - (sx[s] * cs - sy[s] * sn);
                const double dy = y - (sx[s] * sn + sy[s] * cs);
                const double dz = z - sz[s];
                const double range = sqrt(dx * dx + dy * dy + dz * dz);
                const double r = NAV_C * (trx - tt[s]) - range;
                const double inv = 1.0 / range;
                const double ux = dx * inv, uy = dy * inv, uz = dz * inv, w = ww[s];
                const double wx = w * ux, wy = w * uy, wz = w * uz;
                a00 += wx * ux;
                a10 += wy * ux, a11 += wy * uy;
                a20 += wz * ux, a21 += wz * uy, a22 += wz * uz;
                a30 += wx, a31 += wy, a32 += wz, a33 += w;
                b0 += wx * r, b1 += wy * r, b2 += wz * r, b3 += w * r;
                swrr += w * r * r;
            }
        rms = sqrt(swrr / a33);
        // Cholesky A = L L^T; a pivot that is not positive next to its diagonal entry: singular
        constexpr double TINY = 1e-13;
        if (!(a00 > 0.0)) break;
        const double l00 = sqrt(a00);
        const double l10 = a10 / l00, l20 = a20 / l00, l30 = a30 / l00;
        const double p1 = a11 - l10 * l10;
        if (!(p1 > TINY * a11)) break;
        const double l11 = sqrt(p1);
        const double l21 = (a21 - l20 * l10) / l11, l31 = (a31 - l30 * l10) / l11;
        const double p2 = a22 - l20 * l20 - l21 * l21;
        if (!(p2 > TINY * a22)) break;
        const double l22 = sqrt(p2);
        const double l32 = (a32 - l30 * l20 - l31 * l21) / l22;
        const double p3 = a33 - l30 * l30 - l31 * l31 - l32 * l32;
        if (!(p3 > TINY * a33)) break;
        const double l33 = sqrt(p3);
        const double y0 = b0 / l00;
        const double y1 = (b1 - l10 * y0) / l11;
        const double y2 = (b2 - l20 * y0 - l21 * y1) / l22;
        const double y3 = (b3 - l30 * y0 - l31 * y1 - l32 * y2) / l33;
        const double d3 = y3 / l33;
        const double d2 = (y2 - l32 * d3) / l22;
        const double d1 = (y1 - l21 * d2 - l31 * d3) / l11;
        const double d0 = (y0 - l10 * d1 - l20 * d2 - l30 * d3) / l00;
        const double step = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (!isfinite(step) || !isfinite(d3)) break;
        x += d0, y += d1, z += d2, bias += d3;
        steps += 1;
        if (step < 1e-4) {  // the step just applied was the last one
            status = GPSACQ_FIX_OK;
            trx = t0 - bias / NAV_C;
            break;
        }
    }
    out.status = status;
    out.iterations = steps;
    if (status == GPSACQ_FIX_OK) {
        double k = floor(trx * 1e3);
        double frac = trx - k * 1e-3;
        if (frac < 0.0) k -= 1.0, frac += 1e-3;
        if (frac >= 1e-3) k += 1.0, frac -= 1e-3;
        int64_t ms = ((int64_t)ms_first + dmin + (int64_t)k) % NAV_WEEK_MS;
        if (ms < 0) ms += NAV_WEEK_MS;
        out.rx_ms = (int32_t)ms;
        out.rx_frac = frac;
        out.x = x, out.y = y, out.z = z;
        out.rms = rms;
        geodetic(x, y, z, out.lat, out.lon, out.alt);
    }
    a.out[f] = out;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_state_rate(SatRateArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_obs o = a.obs[i];
    gpsacq_sat_rate r = {0.0, 0.0, 0.0, 0.0};
    if (usable(o, a.eph, a.n_eph)) r = sat_state_rate(a.eph[o.eph], o.tx_ms, o.tx_frac);
    a.out[i] = r;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_vel(VelArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    constexpr int S = GPSACQ_FIX_MAX_SATS;
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
                // corrected transmit time less the receive time, the angle the earth turns in between
                const double dt = (double)fold_ms(o.tx_ms - fix.rx_ms) * 1e-3 + ((o.tx_frac - st.clock_corr) - fix.rx_frac);
                double sn, cs;
                sincos(NAV_OMEGA_E * dt, &sn, &cs);
                const double rx = st.x * cs - st.y * sn, ry = st.x * sn + st.y * cs;
                const double wx = sr.vx - NAV_OMEGA_E * st.y, wy = sr.vy + NAV_OMEGA_E * st.x;  // v_s + Omega_e x r_s
                const double vx = wx * cs - wy * sn, vy = wx * sn + wy * cs, vz = sr.vz;
                const double dx = fix.x - rx, dy = fix.y - ry, dz = fix.z - st.z;
                const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
                ux[s] = dx * inv, uy[s] = dy * inv, uz[s] = dz * inv;
                // e = -u:  rho_dot - e . (v_i - Omega_e x r_r) + c clock_drift_i  =  -e . v_r + c drift_r
                const double rel = ux[s] * (vx + NAV_OMEGA_E * fix.y) + uy[s] * (vy - NAV_OMEGA_E * fix.x) + uz[s] * vz;
                yy[s] = -(NAV_C / NAV_L1) * ro.doppler_hz + rel + NAV_C * sr.clock_drift;
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
    // weighted normal equations of the rows h = (ux, uy, uz, 1), as in k_fix
    double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
    double b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (mask >> s & 1) {
            const double w = ww[s], r = yy[s];
            const double wx = w * ux[s], wy = w * uy[s], wz = w * uz[s];
            a00 += wx * ux[s];
            a10 += wy * ux[s], a11 += wy * uy[s];
            a20 += wz * ux[s], a21 += wz * uy[s], a22 += wz * uz[s];
            a30 += wx, a31 += wy, a32 += wz, a33 += w;
            b0 += wx * r, b1 += wy * r, b2 += wz * r, b3 += w * r;
        }
    constexpr double TINY = 1e-13;
    out.status = GPSACQ_VEL_SINGULAR;
    bool ok = false;
    double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    do {
        if (!(a00 > 0.0)) break;
        const double l00 = sqrt(a00);
        const double l10 = a10 / l00, l20 = a20 / l00, l30 = a30 / l00;
        const double p1 = a11 - l10 * l10;
        if (!(p1 > TINY * a11)) break;
        const double l11 = sqrt(p1);
        const double l21 = (a21 - l20 * l10) / l11, l31 = (a31 - l30 * l10) / l11;
        const double p2 = a22 - l20 * l20 - l21 * l21;
        if (!(p2 > TINY * a22)) break;
        const double l22 = sqrt(p2);
        const double l32 = (a32 - l30 * l20 - l31 * l21) / l22;
        const double p3 = a33 - l30 * l30 - l31 * l31 - l32 * l32;
        if (!(p3 > TINY * a33)) break;
        const double l33 = sqrt(p3);
        const double y0 = b0 / l00;
        const double y1 = (b1 - l10 * y0) / l11;
        const double y2 = (b2 - l20 * y0 - l21 * y1) / l22;
        const double y3 = (b3 - l30 * y0 - l31 * y1 - l32 * y2) / l33;
        d3 = y3 / l33;
        d2 = (y2 - l32 * d3) / l22;
        d1 = (y1 - l21 * d2 - l31 * d3) / l11;
        d0 = (y0 - l10 * d1 - l20 * d2 - l30 * d3) / l00;
        ok = isfinite(d0) && isfinite(d1) && isfinite(d2) && isfinite(d3);
    } while (false);
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
        out.drift = d3 / NAV_C;
        out.rms = sqrt(swrr / a33);
    }
    a.out[f] = out;
}

void launch_sat_state_rate(const SatRateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_state_rate, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_vel(const VelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_vel, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_sat_state(const SatStateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_state, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_fix(const FixArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fix, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
