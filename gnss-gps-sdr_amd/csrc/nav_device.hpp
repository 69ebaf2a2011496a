// nav_device.hpp -- the device functions the navigation kernels are written on, all in fp64: nav_kernels.hip (k_sat_state,
// k_sat_state_rate, k_fix, k_vel), fix_kernels.hip (k_sat_view, k_fix_atm, k_raim_detect, k_raim_exclude), coarse_kernels.hip
// (k_coarse_fix), doppler_kernels.hip (k_doppler_fix) and aided_kernels.hip (k_aid_predict) include it, and orbit_device.hpp, the orbit evaluation, is written on its constants; nothing else does.  Constants, geodetic(), the view and the two delays, and the fix solver as functions over a
// row held in registers: load_row, newton, delays, full_fix, residuals, dop_of, fill_fix.  The normal equations of the rows
// (ux, uy, uz, 1) are a Sym<4> of spd_device.hpp, which holds the one Cholesky, its pivot rule and the inverse DOP is read from.
// No LDS, no barrier, no atomics; every loop is bounded, so a bad fix ends, it never spins.  The row is only ever indexed by
// compile-time constants (a subset of it is a bit mask, data and not an index), so it stays in registers: the loops over the
// satellites are unrolled to GPSACQ_FIX_MAX_SATS; the view loop -- a dozen transcendentals per satellite -- keeps ONE body that
// works on element 0 and turns the arrays by a place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_launch.hpp"
#include "spd_device.hpp"

namespace acq {

constexpr double OMEGA_E = 7.2921151467e-5;  // earth rotation rate, rad / s
constexpr double C = 2.99792458e8;           // m / s
constexpr double PI = 3.141592653589793;
constexpr int32_t WEEK_MS = 604800000;
constexpr double WGS84_A = 6378137.0;
constexpr double WGS84_E2 = 0.00669437999014132;
constexpr int FIX_PASSES = 20, GEODETIC_PASSES = 10;
constexpr int S = GPSACQ_FIX_MAX_SATS;

// difference of two milliseconds of week, folded into half a week either way
__device__ __forceinline__ int32_t fold_ms(int32_t d) {
    if (d > WEEK_MS / 2) d -= WEEK_MS;
    else if (d < -WEEK_MS / 2) d += WEEK_MS;
    return d;
}

// t seconds into whole milliseconds and a fraction in [0, 1e-3): fill_fix's rule (k_coarse_fix, k_doppler_fix)
__device__ __forceinline__ void split(double t, double& k, double& frac) {
    k = floor(t * 1e3);
    frac = t - k * 1e-3;
    if (frac < 0.0) k -= 1.0, frac += 1e-3;
    if (frac >= 1e-3) k += 1.0, frac -= 1e-3;
}

// millisecond of week base + k.  A k that is no count of milliseconds (a diverged or non-finite time) is taken as 0: the row
// fails its own tests, the conversion must not overflow on the way there
__device__ __forceinline__ int32_t week_ms(int32_t base, double k) {
    if (!(fabs(k) < 1e12)) k = 0.0;
    int64_t ms = ((int64_t)base + (int64_t)k) % WEEK_MS;
    if (ms < 0) ms += WEEK_MS;
    return (int32_t)ms;
}

__device__ __forceinline__ bool usable(const gpsacq_obs& o, const NavEph* eph, int n_eph) {
    if (!o.valid || o.eph < 0 || o.eph >= n_eph) return false;
    if (!(o.weight >= 0.0) || !isfinite(o.weight) || !isfinite(o.tx_frac)) return false;
    return eph[o.eph].valid != 0;
}

// the satellite turned with the earth from its corrected transmit time to the fix's receive time: sin and cos of the angle
__device__ __forceinline__ void earth_turn(const gpsacq_obs& o, const gpsacq_sat_state& st, const gpsacq_fix& fix, double& sn, double& cs) {
    const double dt = (double)fold_ms(o.tx_ms - fix.rx_ms) * 1e-3 + ((o.tx_frac - st.clock_corr) - fix.rx_frac);
    sincos(OMEGA_E * dt, &sn, &cs);
}

// ---- the receiver's place -----------------------------------------------------------------------------------------------------
// LatLonAlt(), c/solve.cpp:273-293, bounded
__device__ __forceinline__ void geodetic(double x, double y, double z, double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)  // the same bits whatever kernel this is inlined into: fix_raim == fix_atm is asserted in bytes
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

// the receiver's local frame and what does not depend on the satellite.  pow and exp appear only here, in the troposphere's
// height-dependent factor: once per round and lane, not per satellite
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
    g.phi_u = lat / PI, g.lam_u = lon / PI;
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
    const double E = v.el / PI;
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
    const double x = 2.0 * PI * (t - 50400.0) / per;
    if (!(fabs(x) < 1.57)) return C * F * 5e-9;
    const double x2 = x * x;
    return C * F * (5e-9 + amp * (1.0 - x2 / 2.0 + x2 * x2 / 24.0));
}

__device__ __forceinline__ double tropo_of(const Site& g, const View& v) {
    if (!(v.el > 0.0) || g.zenith == 0.0) return 0.0;
    return g.zenith / v.sin_el;
}

// ---- the fix solver -----------------------------------------------------------------------------------------------------------
// the row in registers: satellite position, corrected transmit time as an offset from the row's earliest millisecond, weight, and
// dd: the delay each satellite's residual is reduced by, metres
struct Row {
    double sx[S], sy[S], sz[S], tt[S], ww[S], dd[S];
    uint32_t mask;  // the usable observations
    int n_used;
    int32_t ms_first, dmin;
    double t0;  // the start of the receive time: 75 ms after the mean transmit time
};

struct State {
    double x, y, z, bias;  // bias: metres of light time taken off t0
    double trx, rms;
};

// the row of fix f, its usable observations, the corrected transmit times as offsets from the earliest millisecond of the row,
// the start of the receive time.  Args: FixArgs, FixAtmArgs or RaimArgs
template <class Args>
__device__ __forceinline__ void load_row(const Args& a, size_t f, Row& r) {
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    const gpsacq_sat_state* state = a.state + f * (size_t)a.sats;
    int32_t dms[S];  // whole milliseconds from the first usable observation
    r.mask = 0;
    r.n_used = 0;
    r.ms_first = 0, r.dmin = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        r.sx[s] = r.sy[s] = r.sz[s] = r.tt[s] = r.ww[s] = r.dd[s] = 0.0;
        dms[s] = 0;
        if (s < a.sats) {
            const gpsacq_obs o = obs[s];
            if (usable(o, a.eph, a.n_eph)) {
                const gpsacq_sat_state st = state[s];
                if (!r.n_used) r.ms_first = o.tx_ms;
                dms[s] = fold_ms(o.tx_ms - r.ms_first);
                r.dmin = dms[s] < r.dmin ? dms[s] : r.dmin;
                r.sx[s] = st.x, r.sy[s] = st.y, r.sz[s] = st.z;
                r.tt[s] = o.tx_frac - st.clock_corr;
                r.ww[s] = o.weight;
                r.mask |= 1u << s;
                r.n_used += 1;
            }
        }
    }
    double t0 = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (r.mask >> s & 1) {
            r.tt[s] += (double)(dms[s] - r.dmin) * 1e-3;
            t0 += r.tt[s];
        }
    r.t0 = r.n_used ? t0 / (double)r.n_used + 75e-3 : 0.0;
}

// what a row's records hold until a solve fills them in
__device__ __forceinline__ gpsacq_fix blank_fix(int status, int n_used) {
    gpsacq_fix out;
    out.status = status;
    out.n_used = n_used;
    out.iterations = 0;
    out.rx_ms = 0;
    out.rx_frac = out.x = out.y = out.z = out.lat = out.lon = out.alt = out.rms = 0.0;
    return out;
}

__device__ __forceinline__ gpsacq_fix_dop blank_dop(uint32_t mask, int n_masked) {
    gpsacq_fix_dop dop;
    dop.used_mask = mask;
    dop.n_masked = n_masked;
    dop.gdop = dop.pdop = dop.hdop = dop.vdop = dop.tdop = 0.0;
    return dop;
}

// satellite s of the row from the state given, with the Sagnac turn: the unit vector satellite -> receiver and the residual,
// reduced by the satellite's delay
__device__ __forceinline__ void sight(const Row& r, int s, const State& st, double& ux, double& uy, double& uz, double& res) {
    double sn, cs;
    sincos(OMEGA_E * (r.tt[s] - st.trx), &sn, &cs);
    const double dx = st.x - (r.sx[s] * cs - r.sy[s] * sn);
    const double dy = st.y - (r.sx[s] * sn + r.sy[s] * cs);
    const double dz = st.z - r.sz[s];
    const double range = sqrt(dx * dx + dy * dy + dz * dz);
    res = C * (st.trx - r.tt[s]) - r.dd[s] - range;
    const double inv = 1.0 / range;
    ux = dx * inv, uy = dy * inv, uz = dz * inv;
}

// the Newton iteration from the state given over the satellites of `mask`, every residual reduced by its delay.  A lane runs its
// own iteration: lanes that converge in different pass counts diverge, which is accepted (a fix is ~6 passes).
// PIN: the set is tested bit by bit INSIDE the pass: taken out of the loop, the twelve tests are twelve lane masks (24 scalar
// registers) that live as long as the kernel does and, in k_raim_exclude, spill.  k_fix, which has the registers, runs without
// the pin: with it (and built as fix_kernels.hip is) it measured 3 % slower than before on 81 800 fixes and 9 % on 20 000, without
// it 1 to 3 % faster (DESIGN.md f13 has both sets of runs)
template <bool PIN = true>
__device__ __forceinline__ bool newton(const Row& r, uint32_t mask, State& st, int& steps) {
#pragma unroll 1
    for (int pass = 0; pass < FIX_PASSES; ++pass) {
        if (PIN) asm volatile("" : "+v"(mask));
        st.trx = r.t0 - st.bias / C;
        // weighted normal equations of the rows h = (ux, uy, uz, 1): lower triangle of A = sum w h h^T, b = sum w h r
        Sym<4> n = {};
        double b[4] = {}, swrr = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (mask >> s & 1) {
                double h[4] = {0.0, 0.0, 0.0, 1.0}, res;
                sight(r, s, st, h[0], h[1], h[2], res);
                add_row(n, b, h, r.ww[s], res);
                swrr += r.ww[s] * res * res;
            }
        st.rms = sqrt(swrr / n(3, 3));
        Sym<4> l;
        if (!factor(n, l)) return false;
        double d[4];
        solve(l, b, d);
        const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!isfinite(step) || !isfinite(d[3])) return false;
        st.x += d[0], st.y += d[1], st.z += d[2], st.bias += d[3];
        steps += 1;
        if (step < 1e-4) {  // the step just applied was the last one
            st.trx = r.t0 - st.bias / C;
            return true;
        }
    }
    return false;
}

// the view loop: ONE body for the twelve satellites, which works on element 0 and then turns the arrays it touches by one place
// (compile-time indices, 120 moves next to ten transcendentals); after S turns every element is back where it was.
// The satellites of `mask` get their delay at the state given; `masking`: one below elev_mask is dropped instead.  Returns the
// satellites kept.
__device__ __forceinline__ uint32_t delays(Row& r, uint32_t mask, const State& st, const Site& g, const gpsacq_atm_params& p, bool masking) {
    uint32_t keep = 0, turn = mask;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        if (turn & 1) {
            double sn, cs;
            sincos(OMEGA_E * (r.tt[0] - st.trx), &sn, &cs);
            const View v = view_of(g, (r.sx[0] * cs - r.sy[0] * sn) - st.x, (r.sx[0] * sn + r.sy[0] * cs) - st.y, r.sz[0] - st.z);
            if (!(masking && v.el < p.elev_mask)) {
                keep |= 1u << s;
                r.dd[0] = iono_of(g, p, v) + tropo_of(g, v);
            }
        }
        turn >>= 1;
        const double hx = r.sx[0], hy = r.sy[0], hz = r.sz[0], ht = r.tt[0], hd = r.dd[0];
#pragma unroll
        for (int k = 0; k + 1 < S; ++k)
            r.sx[k] = r.sx[k + 1], r.sy[k] = r.sy[k + 1], r.sz[k] = r.sz[k + 1], r.tt[k] = r.tt[k + 1], r.dd[k] = r.dd[k + 1];
        r.sx[S - 1] = hx, r.sy[S - 1] = hy, r.sz[S - 1] = hz, r.tt[S - 1] = ht, r.dd[S - 1] = hd;
    }
    return keep;
}

// the millisecond of week the row's offsets count from, seconds
__device__ __forceinline__ double base_s(const Row& r) {
    int64_t ms_base = ((int64_t)r.ms_first + r.dmin) % WEEK_MS;
    if (ms_base < 0) ms_base += WEEK_MS;
    return (double)ms_base * 1e-3;
}

// FULL, what k_fix_atm and k_raim_detect solve: stage 0 (the plain iteration from the origin), the elevation mask, then
// GPSACQ_ATM_ROUNDS rounds of (delays at the current state, Newton from the current state)
struct Full {
    State st;
    double lat, lon, alt;
    uint32_t mask;  // the usable observations the elevation mask left
    int status, steps, n_masked, n_used;
};

__device__ __forceinline__ Full full_fix(Row& r, const gpsacq_atm_params& p) {
    Full u = {{0.0, 0.0, 0.0, 0.0, r.t0, 0.0}, 0.0, 0.0, 0.0, r.mask, GPSACQ_FIX_NO_CONVERGE, 0, 0, r.n_used};
    const double base = base_s(r);
#pragma unroll 1
    for (int stage = 0; stage <= GPSACQ_ATM_ROUNDS; ++stage) {
        if (!newton(r, u.mask, u.st, u.steps)) break;
        geodetic(u.st.x, u.st.y, u.st.z, u.lat, u.lon, u.alt);
        if (stage == GPSACQ_ATM_ROUNDS) {
            u.status = GPSACQ_FIX_OK;
            break;
        }
        // the views from here: after stage 0 the mask, and the delays the next round holds
        const Site g = make_site(u.lat, u.lon, u.alt, base + u.st.trx, p.flags);
        const uint32_t keep = delays(r, u.mask, u.st, g, p, stage == 0);
        if (stage == 0) {
            u.mask = keep;
            const int left = __popc(keep);
            u.n_masked = u.n_used - left;
            u.n_used = left;
            if (u.n_used < 4) {
                u.status = GPSACQ_FIX_TOO_FEW;
                break;
            }
            if (!u.n_masked && !p.flags) {
                u.status = GPSACQ_FIX_OK;
                break;
            }
        }
    }
    return u;
}

// STATISTIC and the sums of DOP in one pass at the state given: returns sum w r^2 over `mask` (a weight-0 observation adds 0),
// n the unweighted normal matrix over the satellites of `mask` with weight > 0
__device__ __forceinline__ double residuals(const Row& r, uint32_t mask, const State& st, Sym<4>& n) {
    n = {};
    double swrr = 0.0;
    asm volatile("" : "+v"(mask));  // as in newton: the twelve tests stay here
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((mask >> s & 1) && r.ww[s] > 0.0) {
            double h[4] = {0.0, 0.0, 0.0, 1.0}, res;
            sight(r, s, st, h[0], h[1], h[2], res);
            swrr += r.ww[s] * res * res;
            add_row(n, h, 1.0);
        }
    return swrr;
}

// DOP from the normal matrix of residuals(), at (lat, lon); a failed pivot leaves the five zeros
__device__ __forceinline__ void dop_of(const Sym<4>& n, double lat, double lon, gpsacq_fix_dop& dop) {
    Sym<4> l, m;
    if (!factor(n, l)) return;
    inverse_lower(l, m);  // Q = M^T M, so v^T Q v = |M v|^2
    double sp, cp, sl, cl;
    sincos(lat, &sp, &cp);
    sincos(lon, &sl, &cl);
    const double dir[3][3] = {{-sl, cl, 0.0}, {-sp * cl, -sp * sl, cp}, {cp * cl, cp * sl, sp}};  // east, north, up
    const double q[3] = {inverse_along(m, dir[0]), inverse_along(m, dir[1]), inverse_along(m, dir[2])};
    const double qtt = m(3, 3) * m(3, 3);
    const double gd = sqrt(q[0] + q[1] + q[2] + qtt), pd = sqrt(q[0] + q[1] + q[2]), hd = sqrt(q[0] + q[1]), vd = sqrt(q[2]), td = sqrt(qtt);
    if (!isfinite(gd) || !isfinite(pd) || !isfinite(hd) || !isfinite(vd) || !isfinite(td)) return;
    dop.gdop = gd, dop.pdop = pd, dop.hdop = hd, dop.vdop = vd, dop.tdop = td;
}

// the fields of a gpsacq_fix that is GPSACQ_FIX_OK: the receive time as millisecond of week and fraction, the state, the place
__device__ __forceinline__ void fill_fix(gpsacq_fix& out, const Row& r, const State& st, double lat, double lon, double alt) {
    double k = floor(st.trx * 1e3);
    double frac = st.trx - k * 1e-3;
    if (frac < 0.0) k -= 1.0, frac += 1e-3;
    if (frac >= 1e-3) k += 1.0, frac -= 1e-3;
    int64_t ms = ((int64_t)r.ms_first + r.dmin + (int64_t)k) % WEEK_MS;
    if (ms < 0) ms += WEEK_MS;
    out.rx_ms = (int32_t)ms;
    out.rx_frac = frac;
    out.x = st.x, out.y = st.y, out.z = st.z;
    out.rms = st.rms;
    out.lat = lat, out.lon = lon, out.alt = alt;
}

// the fix and DOP records of full_fix()'s result; returns sum w r^2 at its state (0 where it is not GPSACQ_FIX_OK)
__device__ __forceinline__ double full_records(const Row& r, const Full& u, gpsacq_fix& out, gpsacq_fix_dop& dop) {
    out.status = u.status;
    out.n_used = u.n_used;
    out.iterations = u.steps;
    dop.used_mask = u.mask;
    dop.n_masked = u.n_masked;
    if (u.status != GPSACQ_FIX_OK) return 0.0;
    fill_fix(out, r, u.st, u.lat, u.lon, u.alt);
    Sym<4> n;
    const double swrr = residuals(r, u.mask, u.st, n);
    dop_of(n, u.lat, u.lon, dop);
    return swrr;
}

// the observations of the row with weight > 0: the ones the statistic and DOP count
__device__ __forceinline__ uint32_t weighted(const Row& r) {
    uint32_t m = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) m |= (r.ww[s] > 0.0 ? 1u : 0u) << s;
    return m;
}

}  // namespace acq
