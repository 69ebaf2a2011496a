// atm_kernels.hip -- "Atmosphere, elevation mask and DOP" of include/gpsacq.h, all in fp64.
//
// k_sat_view: one lane per observation: azimuth, elevation, Klobuchar and Saastamoinen delay of a satellite seen from a fix.
// k_fix_atm: one lane per fix.  The row sits in registers as in nav_kernels.hip's k_fix, plus twelve delays, and the lane runs
// stage 0 (k_fix's iteration), the elevation mask, GPSACQ_ATM_ROUNDS rounds of (delays at the current state, Newton from the
// current state), and the dilutions of precision.  The view, ionosphere and troposphere are __device__ functions shared by both
// kernels.  k_fix_atm carries its OWN COPY of k_fix's Newton pass, of usable(), fold_ms() and geodetic() (as k_sat_state_rate
// copies k_sat_state), so that nav_kernels.hip and the code objects of k_sat_state, k_fix and k_vel do not change.  pow and exp
// appear only in the troposphere's height-dependent factor, once per round and lane, not per satellite.
// No LDS, no barrier, no atomics; every loop is bounded.  The row is only ever indexed by compile-time constants, so it stays in
// registers (no scratch): the Newton and DOP loops over the satellites are unrolled to GPSACQ_FIX_MAX_SATS as in k_fix; the
// view loop -- a dozen transcendentals per satellite -- keeps ONE body that works on element 0 and turns the arrays by a place.
// Built with -mllvm -disable-machine-licm (Makefile): hoisted out of the stage loop, the fp64 constants of the inlined libm
// alone overflow the scalar registers (72 spilled); left where they are used the kernel has no spill at all.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atm_launch.hpp"

namespace acq {

namespace {
constexpr double ATM_OMEGA_E = 7.2921151467e-5;  // earth rotation rate, rad / s
constexpr double ATM_C = 2.99792458e8;           // m / s
constexpr double ATM_PI = 3.141592653589793;
constexpr int32_t ATM_WEEK_MS = 604800000;
constexpr double ATM_WGS84_A = 6378137.0;
constexpr double ATM_WGS84_E2 = 0.00669437999014132;
constexpr int ATM_FIX_PASSES = 20, ATM_GEODETIC_PASSES = 10;

// difference of two milliseconds of week, folded into half a week either way
__device__ __forceinline__ int32_t atm_fold_ms(int32_t d) {
    if (d > ATM_WEEK_MS / 2) d -= ATM_WEEK_MS;
    else if (d < -ATM_WEEK_MS / 2) d += ATM_WEEK_MS;
    return d;
}

__device__ __forceinline__ bool atm_usable(const gpsacq_obs& o, const NavEph* eph, int n_eph) {
    if (!o.valid || o.eph < 0 || o.eph >= n_eph) return false;
    if (!(o.weight >= 0.0) || !isfinite(o.weight) || !isfinite(o.tx_frac)) return false;
    return eph[o.eph].valid != 0;
}

// LatLonAlt(), c/solve.cpp:273-293, bounded: k_fix's
__device__ __forceinline__ void atm_geodetic(double x, double y, double z, double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)  // the three copies of this function give the same bits whatever kernel they are inlined into
    const double p = sqrt(x * x + y * y);
    if (!(p > 1e-6)) {  // on the axis: p / cos(lat) is 0 / 0
        lon = 0.0;
        lat = z < 0 ? -1.5707963267948966 : 1.5707963267948966;
        alt = fabs(z) - ATM_WGS84_A * sqrt(1.0 - ATM_WGS84_E2);
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
    lat = atan(z / (p * (1.0 - ATM_WGS84_E2)));
    alt = 0.0;
    for (int k = 0; k < ATM_GEODETIC_PASSES; ++k) {
        const double prev = alt;
        const double sl = sin(lat);
        const double N = ATM_WGS84_A / sqrt(1.0 - ATM_WGS84_E2 * sl * sl);
        alt = p / cos(lat) - N;
        lat = atan(z / (p * (1.0 - ATM_WGS84_E2 * N / (N + alt))));
        if (fabs(alt - prev) < 1e-9) break;
    }
}

// the receiver's local frame and what does not depend on the satellite
struct Site {
    double sp, cp, sl, cl;  // sin / cos of lat and lon
    double phi_u, lam_u;    // semicircles
    double tow;             // receive time of week, seconds
    double zenith;          // tropospheric zenith delay, metres; 0: no troposphere
};

__device__ __forceinline__ Site make_site(double lat, double lon, double alt, double tow, int flags) {
    Site g;
    sincos(lat, &g.sp, &g.cp);
    sincos(lon, &g.sl, &g.cl);
    g.phi_u = lat / ATM_PI, g.lam_u = lon / ATM_PI;
    g.tow = tow;
    g.zenith = 0.0;
    if ((flags & GPSACQ_ATM_TROPO) && !(alt < -100.0) && !(alt > 1e4)) {
        const double h = alt > 0.0 ? alt : 0.0;
        const double P = 1013.25 * pow(1.0 - 2.2557e-5 * h, 5.2568);
        const double T = 288.16 - 6.5e-3 * h;
        const double e = 6.108 * 0.7 * exp((17.15 * T - 4684.0) / (T - 38.45));
        g.zenith = 0.0022768 * P / (1.0 - 0.00266 * (g.cp * g.cp - g.sp * g.sp) - 0.00028 * h / 1000.0) + 0.002277 * (1255.0 / T + 0.05) * e;
    }
    return g;
}

// VIEW: d = satellite - receiver, ECEF.  What the delays need of it: el, and sin az, cos az, sin el as ratios of e, n, u (at the
// zenith, where e = n = 0, az = atan2(0, 0) = 0)
struct View {
    double e, n;    // east, north: az = atan2(e, n)
    double el;
    double sa, ca;  // sin az, cos az
    double sin_el;
};

__device__ __forceinline__ View view_of(const Site& g, double dx, double dy, double dz) {
    View v;
    v.e = -g.sl * dx + g.cl * dy;
    v.n = -g.sp * g.cl * dx - g.sp * g.sl * dy + g.cp * dz;
    const double u = g.cp * g.cl * dx + g.cp * g.sl * dy + g.sp * dz;
    const double h2 = v.e * v.e + v.n * v.n, h = sqrt(h2);
    v.el = atan2(u, h);
    v.sa = h > 0.0 ? v.e / h : 0.0;
    v.ca = h > 0.0 ? v.n / h : 1.0;
    v.sin_el = u / sqrt(h2 + u * u);
    return v;
}

// IONOSPHERE: IS-GPS-200 Figure 20-4; cos(x pi) as cospi(x)
__device__ __forceinline__ double iono_of(const Site& g, const gpsacq_atm_params& p, const View& v) {
    if (!(p.flags & GPSACQ_ATM_IONO) || !(v.el > 0.0)) return 0.0;
    const double E = v.el / ATM_PI;
    const double psi = 0.0137 / (E + 0.11) - 0.022;
    double phi_i = g.phi_u + psi * v.ca;
    phi_i = phi_i > 0.416 ? 0.416 : (phi_i < -0.416 ? -0.416 : phi_i);
    const double lam_i = g.lam_u + psi * v.sa / cospi(phi_i);
    const double phi_m = phi_i + 0.064 * cospi(lam_i - 1.617);
    double t = 4.32e4 * lam_i + g.tow;
    t = t - 86400.0 * floor(t / 86400.0);
    const double k = 0.53 - E;
    const double F = 1.0 + 16.0 * (k * k * k);
    double amp = ((p.alpha[3] * phi_m + p.alpha[2]) * phi_m + p.alpha[1]) * phi_m + p.alpha[0];
    double per = ((p.beta[3] * phi_m + p.beta[2]) * phi_m + p.beta[1]) * phi_m + p.beta[0];
    if (amp < 0.0) amp = 0.0;
    if (per < 72000.0) per = 72000.0;
    const double x = 2.0 * ATM_PI * (t - 50400.0) / per;
    if (!(fabs(x) < 1.57)) return ATM_C * F * 5e-9;
    const double x2 = x * x;
    return ATM_C * F * (5e-9 + amp * (1.0 - x2 / 2.0 + x2 * x2 / 24.0));
}

__device__ __forceinline__ double tropo_of(const Site& g, const View& v) {
    if (!(v.el > 0.0) || g.zenith == 0.0) return 0.0;
    return g.zenith / v.sin_el;
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_view(SatViewArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    gpsacq_sat_view v = {0.0, 0.0, 0.0, 0.0};
    const gpsacq_obs o = a.obs[i];
    const gpsacq_fix fix = a.fix[i / (size_t)a.sats];
    if (fix.status == GPSACQ_FIX_OK && atm_usable(o, a.eph, a.n_eph)) {
        const gpsacq_sat_state st = a.state[i];
        double lat, lon, alt;
        atm_geodetic(fix.x, fix.y, fix.z, lat, lon, alt);
        const Site g = make_site(lat, lon, alt, (double)fix.rx_ms * 1e-3 + fix.rx_frac, a.p.flags);
        // corrected transmit time less the receive time, the angle the earth turns in between (k_vel's)
        const double dt = (double)atm_fold_ms(o.tx_ms - fix.rx_ms) * 1e-3 + ((o.tx_frac - st.clock_corr) - fix.rx_frac);
        double sn, cs;
        sincos(ATM_OMEGA_E * dt, &sn, &cs);
        const double dx = (st.x * cs - st.y * sn) - fix.x, dy = (st.x * sn + st.y * cs) - fix.y, dz = st.z - fix.z;
        const View w = view_of(g, dx, dy, dz);
        v.az = atan2(w.e, w.n);
        v.el = w.el;
        v.iono_m = iono_of(g, a.p, w);
        v.tropo_m = tropo_of(g, w);
    }
    a.out[i] = v;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_fix_atm(FixAtmArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    constexpr int S = GPSACQ_FIX_MAX_SATS;
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    const gpsacq_sat_state* state = a.state + f * (size_t)a.sats;

    // the row into registers, as k_fix does; dd: the delay each satellite's residual is reduced by, metres
    double sx[S], sy[S], sz[S], tt[S], ww[S], dd[S];
    int32_t dms[S];
    uint32_t mask = 0;
    int n_used = 0;
    int32_t ms_first = 0, dmin = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        sx[s] = sy[s] = sz[s] = tt[s] = ww[s] = dd[s] = 0.0;
        dms[s] = 0;
        if (s < a.sats) {
            const gpsacq_obs o = obs[s];
            if (atm_usable(o, a.eph, a.n_eph)) {
                const gpsacq_sat_state st = state[s];
                if (!n_used) ms_first = o.tx_ms;
                dms[s] = atm_fold_ms(o.tx_ms - ms_first);
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
    gpsacq_fix_dop dop;
    dop.used_mask = mask;
    dop.n_masked = 0;
    dop.gdop = dop.pdop = dop.hdop = dop.vdop = dop.tdop = 0.0;
    if (n_used < 4) {
        a.out[f] = out;
        a.dop[f] = dop;
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
    int64_t ms_base = ((int64_t)ms_first + dmin) % ATM_WEEK_MS;  // the millisecond of week the offsets count from
    if (ms_base < 0) ms_base += ATM_WEEK_MS;

    double x = 0.0, y = 0.0, z = 0.0, bias = 0.0;  // bias: metres of light time taken off t0
    double trx = t0, rms = 0.0;
    double lat = 0.0, lon = 0.0, alt = 0.0;
    int status = GPSACQ_FIX_NO_CONVERGE, steps = 0, n_masked = 0;
    constexpr double TINY = 1e-13;
#pragma unroll 1
    for (int stage = 0; stage <= GPSACQ_ATM_ROUNDS; ++stage) {
        // k_fix's Newton iteration from the current state (stage 0: the origin), every residual reduced by its delay
        bool converged = false;
#pragma unroll 1
        for (int pass = 0; pass < ATM_FIX_PASSES; ++pass) {
            trx = t0 - bias / ATM_C;
            double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
            double b0 = 0, b1 = 0, b2 = 0, b3 = 0, swrr = 0;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (mask >> s & 1) {
                    double sn, cs;
                    sincos(ATM_OMEGA_E * (tt[s] - trx), &sn, &cs);
                    const double dx = x - (sx[s] * cs - sy[s] * sn);
                    const double dy = y - (sx[s] * sn + sy[s] * cs);
                    const double dz = z - sz[s];
                    const double range = sqrt(dx * dx + dy * dy + dz * dz);
                    const double r = ATM_C * (trx - tt[s]) - dd[s] - range;
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
            if (step < 1e-4) {  // the step just applied was the last one of this stage
                converged = true;
                trx = t0 - bias / ATM_C;
                break;
            }
        }
        if (!converged) break;
        atm_geodetic(x, y, z, lat, lon, alt);
        if (stage == GPSACQ_ATM_ROUNDS) {
            status = GPSACQ_FIX_OK;
            break;
        }
        // the views from here: after stage 0 the mask, and the delays the next round holds
        const Site g = make_site(lat, lon, alt, (double)ms_base * 1e-3 + trx, a.p.flags);
        // ONE body for the twelve satellites: it works on element 0 and the arrays it touches are then turned by one place
        // (compile-time indices, 120 moves next to ten transcendentals); after S turns every element is back where it was
        uint32_t keep = 0, turn = mask;
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            if (turn & 1) {
                double sn, cs;
                sincos(ATM_OMEGA_E * (tt[0] - trx), &sn, &cs);
                const View v = view_of(g, (sx[0] * cs - sy[0] * sn) - x, (sx[0] * sn + sy[0] * cs) - y, sz[0] - z);
                if (!(stage == 0 && v.el < a.p.elev_mask)) {
                    keep |= 1u << s;
                    dd[0] = iono_of(g, a.p, v) + tropo_of(g, v);
                }
            }
            turn >>= 1;
            const double hx = sx[0], hy = sy[0], hz = sz[0], ht = tt[0], hd = dd[0];
#pragma unroll
            for (int k = 0; k + 1 < S; ++k) sx[k] = sx[k + 1], sy[k] = sy[k + 1], sz[k] = sz[k + 1], tt[k] = tt[k + 1], dd[k] = dd[k + 1];
            sx[S - 1] = hx, sy[S - 1] = hy, sz[S - 1] = hz, tt[S - 1] = ht, dd[S - 1] = hd;
        }
        if (stage == 0) {
            mask = keep;
            const int left = __popc(keep);
            n_masked = n_used - left;
            n_used = left;
            if (n_used < 4) {
                status = GPSACQ_FIX_TOO_FEW;
                break;
            }
            if (!n_masked && !a.p.flags) {
                status = GPSACQ_FIX_OK;
                break;
            }
        }
    }
    out.status = status;
    out.n_used = n_used;
    out.iterations = steps;
    dop.used_mask = mask;
    dop.n_masked = n_masked;
    if (status == GPSACQ_FIX_OK) {
        double k = floor(trx * 1e3);
        double frac = trx - k * 1e-3;
        if (frac < 0.0) k -= 1.0, frac += 1e-3;
        if (frac >= 1e-3) k += 1.0, frac -= 1e-3;
        int64_t ms = ((int64_t)ms_first + dmin + (int64_t)k) % ATM_WEEK_MS;
        if (ms < 0) ms += ATM_WEEK_MS;
        out.rx_ms = (int32_t)ms;
        out.rx_frac = frac;
        out.x = x, out.y = y, out.z = z;
        out.rms = rms;
        out.lat = lat, out.lon = lon, out.alt = alt;

        // DOP: unweighted normal matrix of the rows (ux, uy, uz, 1) over the satellites used with weight > 0
        double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if ((mask >> s & 1) && ww[s] > 0.0) {
                double sn, cs;
                sincos(ATM_OMEGA_E * (tt[s] - trx), &sn, &cs);
                const double dx = x - (sx[s] * cs - sy[s] * sn);
                const double dy = y - (sx[s] * sn + sy[s] * cs);
                const double dz = z - sz[s];
                const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
                const double ux = dx * inv, uy = dy * inv, uz = dz * inv;
                a00 += ux * ux;
                a10 += uy * ux, a11 += uy * uy;
                a20 += uz * ux, a21 += uz * uy, a22 += uz * uz;
                a30 += ux, a31 += uy, a32 += uz, a33 += 1.0;
            }
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
            // M = L^-1 (lower); Q = M^T M, so v^T Q v = |M v|^2
            const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22, m33 = 1.0 / l33;
            const double m10 = -l10 * m00 * m11;
            const double m21 = -l21 * m11 * m22;
            const double m20 = -(l20 * m00 + l21 * m10) * m22;
            const double m32 = -l32 * m22 * m33;
            const double m31 = -(l31 * m11 + l32 * m21) * m33;
            const double m30 = -(l30 * m00 + l31 * m10 + l32 * m20) * m33;
            double sp, cp, sl, cl;
            sincos(lat, &sp, &cp);
            sincos(lon, &sl, &cl);
            const double dir[3][3] = {{-sl, cl, 0.0}, {-sp * cl, -sp * sl, cp}, {cp * cl, cp * sl, sp}};  // east, north, up
            double q[3];
#pragma unroll
            for (int k2 = 0; k2 < 3; ++k2) {
                const double v0 = dir[k2][0], v1 = dir[k2][1], v2 = dir[k2][2];
                const double c0 = m00 * v0, c1 = m10 * v0 + m11 * v1, c2 = m20 * v0 + m21 * v1 + m22 * v2, c3 = m30 * v0 + m31 * v1 + m32 * v2;
                q[k2] = c0 * c0 + c1 * c1 + c2 * c2 + c3 * c3;
            }
            const double qtt = m33 * m33;
            const double gd = sqrt(q[0] + q[1] + q[2] + qtt), pd = sqrt(q[0] + q[1] + q[2]), hd = sqrt(q[0] + q[1]), vd = sqrt(q[2]), td = sqrt(qtt);
            if (!isfinite(gd) || !isfinite(pd) || !isfinite(hd) || !isfinite(vd) || !isfinite(td)) break;
            dop.gdop = gd, dop.pdop = pd, dop.hdop = hd, dop.vdop = vd, dop.tdop = td;
        } while (false);
    }
    a.out[f] = out;
    a.dop[f] = dop;
}

void launch_sat_view(const SatViewArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_view, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_fix_atm(const FixAtmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fix_atm, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
