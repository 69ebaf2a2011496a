// raim_kernels.hip -- "Fix integrity: residual test and single-satellite exclusion" of include/gpsacq.h, all in fp64.
//
// k_raim_detect: one lane per fix.  k_fix_atm's algorithm (stage 0, the mask, the rounds, DOP) followed by ONE more pass over the
// row that gives the statistic T(S) at the converged state and, in the same loop, the sums DOP is made from.  It writes
// gpsacq_fix, gpsacq_fix_dop and gpsacq_fix_raim of every row, and for a row that fails the test with something to exclude a
// RaimRow (raim_launch.hpp) in engine scratch.
// k_raim_exclude: sixteen lanes per fix, four fixes per wave64.  Every lane of a group holds the whole row in registers; lane k
// runs the Newton iteration over S \ {k} from the full solution's state with its delays held, the sixteen (T_k, k) are reduced
// to the smallest by four __shfl_xor exchanges of width 16 (no LDS, no atomics), and the winning lane alone goes on: FINAL's
// rounds, the statistic and DOP over the final set, and the row's three records.  Lanes 12-15 and lanes whose k is not in S or
// has weight 0 carry T = +inf.  The candidate solve and every round of FINAL are iterations of ONE stage loop, so the kernel holds
// one copy of the Newton pass and one of the statistic / DOP pass.  A group whose row did not ask for exclusion returns at once.
// Both kernels carry their OWN COPY of the Newton pass, usable(), fold_ms(), geodetic(), the view and the delay functions, as
// atm_kernels.hip copies from nav_kernels.hip, so that the code objects of k_sat_state, k_fix, k_vel, k_sat_view and k_fix_atm
// do not change.  Every loop is bounded.  The row is only ever indexed by compile-time constants (the subset a lane solves is a
// bit mask, data and not an index; the lane's own weight is picked by an unrolled select), so it stays in registers.
// Built with -mllvm -disable-machine-licm (Makefile), as atm_kernels.hip and for its reason: the resource-usage remarks of the
// build show no spill and no scratch in either kernel with it (see DESIGN.md for the figures).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raim_launch.hpp"

namespace acq {

namespace {
constexpr double RAIM_OMEGA_E = 7.2921151467e-5;  // earth rotation rate, rad / s
constexpr double RAIM_C = 2.99792458e8;           // m / s
constexpr double RAIM_PI = 3.141592653589793;
constexpr int32_t RAIM_WEEK_MS = 604800000;
constexpr double RAIM_WGS84_A = 6378137.0;
constexpr double RAIM_WGS84_E2 = 0.00669437999014132;
constexpr int RAIM_FIX_PASSES = 20, RAIM_GEODETIC_PASSES = 10;
constexpr double RAIM_TINY = 1e-13;
constexpr int S = GPSACQ_FIX_MAX_SATS;

// difference of two milliseconds of week, folded into half a week either way
__device__ __forceinline__ int32_t raim_fold_ms(int32_t d) {
    if (d > RAIM_WEEK_MS / 2) d -= RAIM_WEEK_MS;
    else if (d < -RAIM_WEEK_MS / 2) d += RAIM_WEEK_MS;
    return d;
}

__device__ __forceinline__ bool raim_usable(const gpsacq_obs& o, const NavEph* eph, int n_eph) {
    if (!o.valid || o.eph < 0 || o.eph >= n_eph) return false;
    if (!(o.weight >= 0.0) || !isfinite(o.weight) || !isfinite(o.tx_frac)) return false;
    return eph[o.eph].valid != 0;
}

// LatLonAlt(), c/solve.cpp:273-293, bounded: k_fix's
__device__ __forceinline__ void raim_geodetic(double x, double y, double z, double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)  // the three copies of this function give the same bits whatever kernel they are inlined into
    const double p = sqrt(x * x + y * y);
    if (!(p > 1e-6)) {  // on the axis: p / cos(lat) is 0 / 0
        lon = 0.0;
        lat = z < 0 ? -1.5707963267948966 : 1.5707963267948966;
        alt = fabs(z) - RAIM_WGS84_A * sqrt(1.0 - RAIM_WGS84_E2);
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
    lat = atan(z / (p * (1.0 - RAIM_WGS84_E2)));
    alt = 0.0;
    for (int k = 0; k < RAIM_GEODETIC_PASSES; ++k) {
        const double prev = alt;
        const double sl = sin(lat);
        const double N = RAIM_WGS84_A / sqrt(1.0 - RAIM_WGS84_E2 * sl * sl);
        alt = p / cos(lat) - N;
        lat = atan(z / (p * (1.0 - RAIM_WGS84_E2 * N / (N + alt))));
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

__device__ __forceinline__ Site raim_site(double lat, double lon, double alt, double tow, int flags) {
    Site g;
    sincos(lat, &g.sp, &g.cp);
    sincos(lon, &g.sl, &g.cl);
    g.phi_u = lat / RAIM_PI, g.lam_u = lon / RAIM_PI;
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

// VIEW: d = satellite - receiver, ECEF (atm_kernels.hip's)
struct View {
    double e, n;    // east, north: az = atan2(e, n)
    double el;
    double sa, ca;  // sin az, cos az
    double sin_el;
};

__device__ __forceinline__ View raim_view(const Site& g, double dx, double dy, double dz) {
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
__device__ __forceinline__ double raim_iono(const Site& g, const gpsacq_atm_params& p, const View& v) {
    if (!(p.flags & GPSACQ_ATM_IONO) || !(v.el > 0.0)) return 0.0;
    const double E = v.el / RAIM_PI;
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
    const double x = 2.0 * RAIM_PI * (t - 50400.0) / per;
    if (!(fabs(x) < 1.57)) return RAIM_C * F * 5e-9;
    const double x2 = x * x;
    return RAIM_C * F * (5e-9 + amp * (1.0 - x2 / 2.0 + x2 * x2 / 24.0));
}

__device__ __forceinline__ double raim_tropo(const Site& g, const View& v) {
    if (!(v.el > 0.0) || g.zenith == 0.0) return 0.0;
    return g.zenith / v.sin_el;
}

// the row in registers, as k_fix_atm holds it; dd: the delay each satellite's residual is reduced by, metres
struct Row {
    double sx[S], sy[S], sz[S], tt[S], ww[S], dd[S];
    uint32_t mask;  // the usable observations
    int n_used;
    int32_t ms_first, dmin;
    double t0;
};

struct State {
    double x, y, z, bias;  // bias: metres of light time taken off t0
    double trx, rms;
};

// the unweighted normal matrix of the rows (ux, uy, uz, 1): what DOP is made from
struct Normal {
    double a00, a10, a11, a20, a21, a22, a30, a31, a32, a33;
};

// k_fix_atm's prologue: the row, its usable observations, the corrected transmit times as offsets from the earliest millisecond
// of the row, the start of the receive time
__device__ __forceinline__ void raim_load(const RaimArgs& a, size_t f, Row& r) {
    const gpsacq_obs* obs = a.obs + f * (size_t)a.sats;
    const gpsacq_sat_state* state = a.state + f * (size_t)a.sats;
    int32_t dms[S];
    r.mask = 0;
    r.n_used = 0;
    r.ms_first = 0, r.dmin = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        r.sx[s] = r.sy[s] = r.sz[s] = r.tt[s] = r.ww[s] = r.dd[s] = 0.0;
        dms[s] = 0;
        if (s < a.sats) {
            const gpsacq_obs o = obs[s];
            if (raim_usable(o, a.eph, a.n_eph)) {
                const gpsacq_sat_state st = state[s];
                if (!r.n_used) r.ms_first = o.tx_ms;
                dms[s] = raim_fold_ms(o.tx_ms - r.ms_first);
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

// k_fix's Newton iteration from the state given over the satellites of `mask`, every residual reduced by its delay
__device__ __forceinline__ bool raim_newton(const Row& r, uint32_t mask, State& st, int& steps) {
#pragma unroll 1
    for (int pass = 0; pass < RAIM_FIX_PASSES; ++pass) {
        // the set is tested bit by bit INSIDE the pass: taken out of the loop, the twelve tests are twelve lane masks (24 scalar
        // registers) that live as long as the kernel does and, in k_raim_exclude, spill
        asm volatile("" : "+v"(mask));
        st.trx = r.t0 - st.bias / RAIM_C;
        double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
        double b0 = 0, b1 = 0, b2 = 0, b3 = 0, swrr = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (mask >> s & 1) {
                double sn, cs;
                sincos(RAIM_OMEGA_E * (r.tt[s] - st.trx), &sn, &cs);
                const double dx = st.x - (r.sx[s] * cs - r.sy[s] * sn);
                const double dy = st.y - (r.sx[s] * sn + r.sy[s] * cs);
                const double dz = st.z - r.sz[s];
                const double range = sqrt(dx * dx + dy * dy + dz * dz);
                const double res = RAIM_C * (st.trx - r.tt[s]) - r.dd[s] - range;
                const double inv = 1.0 / range;
                const double ux = dx * inv, uy = dy * inv, uz = dz * inv, w = r.ww[s];
                const double wx = w * ux, wy = w * uy, wz = w * uz;
                a00 += wx * ux;
                a10 += wy * ux, a11 += wy * uy;
                a20 += wz * ux, a21 += wz * uy, a22 += wz * uz;
                a30 += wx, a31 += wy, a32 += wz, a33 += w;
                b0 += wx * res, b1 += wy * res, b2 += wz * res, b3 += w * res;
                swrr += w * res * res;
            }
        st.rms = sqrt(swrr / a33);
        // Cholesky A = L L^T; a pivot that is not positive next to its diagonal entry: singular
        if (!(a00 > 0.0)) return false;
        const double l00 = sqrt(a00);
        const double l10 = a10 / l00, l20 = a20 / l00, l30 = a30 / l00;
        const double p1 = a11 - l10 * l10;
        if (!(p1 > RAIM_TINY * a11)) return false;
        const double l11 = sqrt(p1);
        const double l21 = (a21 - l20 * l10) / l11, l31 = (a31 - l30 * l10) / l11;
        const double p2 = a22 - l20 * l20 - l21 * l21;
        if (!(p2 > RAIM_TINY * a22)) return false;
        const double l22 = sqrt(p2);
        const double l32 = (a32 - l30 * l20 - l31 * l21) / l22;
        const double p3 = a33 - l30 * l30 - l31 * l31 - l32 * l32;
        if (!(p3 > RAIM_TINY * a33)) return false;
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
        if (!isfinite(step) || !isfinite(d3)) return false;
        st.x += d0, st.y += d1, st.z += d2, st.bias += d3;
        steps += 1;
        if (step < 1e-4) {  // the step just applied was the last one
            st.trx = r.t0 - st.bias / RAIM_C;
            return true;
        }
    }
    return false;
}

// k_fix_atm's view loop: ONE body for the twelve satellites, which works on element 0 and then turns the arrays by one place.
// The satellites of `mask` get their delay at the state given; `masking`: one below elev_mask is dropped instead.  Returns the
// satellites kept.
__device__ __forceinline__ uint32_t raim_delays(Row& r, uint32_t mask, const State& st, const Site& g, const gpsacq_atm_params& p, bool masking) {
    uint32_t keep = 0, turn = mask;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        if (turn & 1) {
            double sn, cs;
            sincos(RAIM_OMEGA_E * (r.tt[0] - st.trx), &sn, &cs);
            const View v = raim_view(g, (r.sx[0] * cs - r.sy[0] * sn) - st.x, (r.sx[0] * sn + r.sy[0] * cs) - st.y, r.sz[0] - st.z);
            if (!(masking && v.el < p.elev_mask)) {
                keep |= 1u << s;
                r.dd[0] = raim_iono(g, p, v) + raim_tropo(g, v);
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

// STATISTIC and the sums of DOP in one pass at the state given: returns sum w r^2 over `mask` (a weight-0 observation adds 0),
// n the normal matrix over the satellites of `mask` with weight > 0
__device__ __forceinline__ double raim_residuals(const Row& r, uint32_t mask, const State& st, Normal& n) {
    n.a00 = n.a10 = n.a11 = n.a20 = n.a21 = n.a22 = n.a30 = n.a31 = n.a32 = n.a33 = 0.0;
    double swrr = 0.0;
    asm volatile("" : "+v"(mask));  // as in raim_newton: the twelve tests stay here
#pragma unroll
    for (int s = 0; s < S; ++s)
        if ((mask >> s & 1) && r.ww[s] > 0.0) {
            double sn, cs;
            sincos(RAIM_OMEGA_E * (r.tt[s] - st.trx), &sn, &cs);
            const double dx = st.x - (r.sx[s] * cs - r.sy[s] * sn);
            const double dy = st.y - (r.sx[s] * sn + r.sy[s] * cs);
            const double dz = st.z - r.sz[s];
            const double range = sqrt(dx * dx + dy * dy + dz * dz);
            const double res = RAIM_C * (st.trx - r.tt[s]) - r.dd[s] - range;
            swrr += r.ww[s] * res * res;
            const double inv = 1.0 / range;
            const double ux = dx * inv, uy = dy * inv, uz = dz * inv;
            n.a00 += ux * ux;
            n.a10 += uy * ux, n.a11 += uy * uy;
            n.a20 += uz * ux, n.a21 += uz * uy, n.a22 += uz * uz;
            n.a30 += ux, n.a31 += uy, n.a32 += uz, n.a33 += 1.0;
        }
    return swrr;
}

// DOP of the section above from its normal matrix, at (lat, lon); a failed pivot leaves the five zeros
__device__ __forceinline__ void raim_dop(const Normal& n, double lat, double lon, gpsacq_fix_dop& dop) {
    if (!(n.a00 > 0.0)) return;
    const double l00 = sqrt(n.a00);
    const double l10 = n.a10 / l00, l20 = n.a20 / l00, l30 = n.a30 / l00;
    const double p1 = n.a11 - l10 * l10;
    if (!(p1 > RAIM_TINY * n.a11)) return;
    const double l11 = sqrt(p1);
    const double l21 = (n.a21 - l20 * l10) / l11, l31 = (n.a31 - l30 * l10) / l11;
    const double p2 = n.a22 - l20 * l20 - l21 * l21;
    if (!(p2 > RAIM_TINY * n.a22)) return;
    const double l22 = sqrt(p2);
    const double l32 = (n.a32 - l30 * l20 - l31 * l21) / l22;
    const double p3 = n.a33 - l30 * l30 - l31 * l31 - l32 * l32;
    if (!(p3 > RAIM_TINY * n.a33)) return;
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
    if (!isfinite(gd) || !isfinite(pd) || !isfinite(hd) || !isfinite(vd) || !isfinite(td)) return;
    dop.gdop = gd, dop.pdop = pd, dop.hdop = hd, dop.vdop = vd, dop.tdop = td;
}

// the fields of a gpsacq_fix that is GPSACQ_FIX_OK, as k_fix_atm writes them
__device__ __forceinline__ void raim_fill_fix(gpsacq_fix& out, const Row& r, const State& st, double lat, double lon, double alt) {
    double k = floor(st.trx * 1e3);
    double frac = st.trx - k * 1e-3;
    if (frac < 0.0) k -= 1.0, frac += 1e-3;
    if (frac >= 1e-3) k += 1.0, frac -= 1e-3;
    int64_t ms = ((int64_t)r.ms_first + r.dmin + (int64_t)k) % RAIM_WEEK_MS;
    if (ms < 0) ms += RAIM_WEEK_MS;
    out.rx_ms = (int32_t)ms;
    out.rx_frac = frac;
    out.x = st.x, out.y = st.y, out.z = st.z;
    out.rms = st.rms;
    out.lat = lat, out.lon = lon, out.alt = alt;
}

// the millisecond of week the row's offsets count from, seconds
__device__ __forceinline__ double raim_base_s(const Row& r) {
    int64_t ms_base = ((int64_t)r.ms_first + r.dmin) % RAIM_WEEK_MS;
    if (ms_base < 0) ms_base += RAIM_WEEK_MS;
    return (double)ms_base * 1e-3;
}

__device__ __forceinline__ uint32_t raim_weighted(const Row& r) {
    uint32_t m = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) m |= (r.ww[s] > 0.0 ? 1u : 0u) << s;
    return m;
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_raim_detect(RaimArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    Row r;
    raim_load(a, f, r);

    gpsacq_fix out;
    out.status = GPSACQ_FIX_TOO_FEW;
    out.n_used = r.n_used;
    out.iterations = 0;
    out.rx_ms = 0;
    out.rx_frac = out.x = out.y = out.z = out.lat = out.lon = out.alt = out.rms = 0.0;
    gpsacq_fix_dop dop;
    dop.used_mask = r.mask;
    dop.n_masked = 0;
    dop.gdop = dop.pdop = dop.hdop = dop.vdop = dop.tdop = 0.0;
    gpsacq_fix_raim raim;
    raim.status = GPSACQ_RAIM_NONE;
    raim.dof = 0, raim.excluded = -1, raim.n_candidates = 0;
    raim.stat_full = raim.stat = raim.threshold = 0.0;
    a.rows[f].go = 0;
    if (r.n_used < 4) {
        a.out[f] = out;
        a.dop[f] = dop;
        a.raim[f] = raim;
        return;
    }

    // FULL: k_fix_atm's stages
    const double base_s = raim_base_s(r);
    State st = {0.0, 0.0, 0.0, 0.0, r.t0, 0.0};
    double lat = 0.0, lon = 0.0, alt = 0.0;
    uint32_t mask = r.mask;
    int status = GPSACQ_FIX_NO_CONVERGE, steps = 0, n_masked = 0, n_used = r.n_used;
#pragma unroll 1
    for (int stage = 0; stage <= GPSACQ_ATM_ROUNDS; ++stage) {
        if (!raim_newton(r, mask, st, steps)) break;
        raim_geodetic(st.x, st.y, st.z, lat, lon, alt);
        if (stage == GPSACQ_ATM_ROUNDS) {
            status = GPSACQ_FIX_OK;
            break;
        }
        // the views from here: after stage 0 the mask, and the delays the next round holds
        const Site g = raim_site(lat, lon, alt, base_s + st.trx, a.p.flags);
        const uint32_t keep = raim_delays(r, mask, st, g, a.p, stage == 0);
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
        raim_fill_fix(out, r, st, lat, lon, alt);
        Normal n;
        const double swrr = raim_residuals(r, mask, st, n);
        raim_dop(n, lat, lon, dop);
        // TEST
        const int d = __popc(mask & raim_weighted(r)) - 4;
        const double T = swrr / (a.r.sigma_m * a.r.sigma_m);
        raim.dof = d;
        raim.stat_full = raim.stat = T;
        if (d < 1) {
            raim.status = GPSACQ_RAIM_UNCHECKED;
        } else {
            // d <= GPSACQ_RAIM_MAX_DOF; a select over the table, not an index
            double thr = a.r.threshold[0];
#pragma unroll
            for (int j = 1; j < GPSACQ_RAIM_MAX_DOF; ++j) thr = d == j + 1 ? a.r.threshold[j] : thr;
            raim.threshold = thr;
            if (T <= thr) {
                raim.status = GPSACQ_RAIM_PASS;
            } else {
                raim.status = GPSACQ_RAIM_FAILED;  // k_raim_exclude overwrites the row where an exclusion mends it
                if (a.r.exclude && d >= 2) {
                    RaimRow* row = a.rows + f;
                    row->x = st.x, row->y = st.y, row->z = st.z, row->bias = st.bias;
                    row->t0 = r.t0;
#pragma unroll
                    for (int s = 0; s < S; ++s) row->delay[s] = r.dd[s];
                    row->stat_full = T;
                    row->mask = mask;
                    row->steps = steps;
                    row->n_masked = n_masked;
                    row->go = 1;
                }
            }
        }
    }
    a.out[f] = out;
    a.dop[f] = dop;
    a.raim[f] = raim;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_raim_exclude(RaimArgs a) {
    const size_t lane = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    const size_t f = lane / RAIM_GROUP;
    const int k = (int)(lane % RAIM_GROUP);
    if (f >= a.n_fix) return;
    const RaimRow* row = a.rows + f;
    if (!row->go) return;  // the same for the sixteen lanes of a group

    Row r;
    raim_load(a, f, r);
    r.t0 = row->t0;
#pragma unroll
    for (int s = 0; s < S; ++s) r.dd[s] = row->delay[s];
    const uint32_t full = row->mask;
    const uint32_t weighted = full & raim_weighted(r);
    const int d = __popc(weighted) - 4;  // >= 2: k_raim_detect's test
    const uint32_t mask = full & ~(1u << k);
    const int n_masked = row->n_masked;
    const double stat_full = row->stat_full;
    double thr = a.r.threshold[0];  // threshold[d - 2], by select
#pragma unroll
    for (int j = 1; j < GPSACQ_RAIM_MAX_DOF; ++j) thr = d - 1 == j + 1 ? a.r.threshold[j] : thr;
    double sigma2 = a.r.sigma_m * a.r.sigma_m;
    const double base_s = raim_base_s(r);
    gpsacq_fix* fix_out = a.out + f;
    gpsacq_fix_dop* dop_out = a.dop + f;
    gpsacq_fix_raim* raim_out = a.raim + f;
    asm volatile("" : "+v"(sigma2), "+v"(fix_out), "+v"(dop_out), "+v"(raim_out));  // for the same reason as the flags below
    // the flags in a vector register: as scalars, they and the lane masks of their two bit tests live through the whole stage
    // loop, six scalar registers more than there are
    int flags = a.p.flags;
    asm volatile("" : "+v"(flags));
    const int rounds = !n_masked && !flags ? 0 : GPSACQ_ATM_ROUNDS;  // of FINAL

    State st = {row->x, row->y, row->z, row->bias, 0.0, 0.0};
    double lat = 0.0, lon = 0.0, alt = 0.0;
    int steps = 0, n_candidates = 0;
    // what the winning lane writes if FINAL fails; filled in where it ends well
    gpsacq_fix out;
    out.status = GPSACQ_FIX_NO_CONVERGE;
    out.n_used = __popc(mask);
    out.rx_ms = 0;
    out.rx_frac = out.x = out.y = out.z = out.lat = out.lon = out.alt = out.rms = 0.0;
    gpsacq_fix_dop dop;
    dop.used_mask = mask;
    dop.n_masked = n_masked;
    dop.gdop = dop.pdop = dop.hdop = dop.vdop = dop.tdop = 0.0;
    gpsacq_fix_raim raim;
    raim.status = GPSACQ_RAIM_NONE;
    raim.dof = 0, raim.excluded = k, raim.n_candidates = 0;
    raim.stat_full = raim.stat = raim.threshold = 0.0;
    // stage 0: the candidate solve of every lane (k is a candidate where it is in S with weight > 0: never for k >= 12) and the
    // reduction; stages 1 .. rounds: FINAL's rounds, winner only
#pragma unroll 1
    for (int stage = 0; stage <= rounds; ++stage) {
        bool converged = false;
        if (stage > 0 || (weighted >> k & 1)) converged = raim_newton(r, mask, st, steps);
        const bool last = stage == rounds;
        double swrr = INFINITY;
        Normal n;
        if (converged && (stage == 0 || last)) swrr = raim_residuals(r, mask, st, n);
        if (stage == 0) {
            // the smallest T_k of the group, on a tie the lowest k: a butterfly over the sixteen lanes, every lane ends with the result
            double best = swrr / sigma2;
            if (!(best < INFINITY)) best = INFINITY;  // a NaN is no candidate's statistic
            int best_k = k, count = converged ? 1 : 0;
#pragma unroll
            for (int off = 1; off < RAIM_GROUP; off <<= 1) {
                const double ot = __shfl_xor(best, off, RAIM_GROUP);
                const int ok = __shfl_xor(best_k, off, RAIM_GROUP);
                count += __shfl_xor(count, off, RAIM_GROUP);
                if (ot < best || (ot == best && ok < best_k)) best = ot, best_k = ok;
            }
            n_candidates = count;
            if (!(best <= thr)) {  // FAILED stands, with the full solution; only the count is news
                if (k == 0) raim_out->n_candidates = n_candidates;
                return;
            }
            if (k != best_k) return;
        } else if (!converged) {
            break;
        }
        raim_geodetic(st.x, st.y, st.z, lat, lon, alt);
        if (last) {
            out.status = GPSACQ_FIX_OK;
            raim_fill_fix(out, r, st, lat, lon, alt);
            raim_dop(n, lat, lon, dop);
            raim.status = GPSACQ_RAIM_EXCLUDED;
            raim.dof = d - 1;
            raim.n_candidates = n_candidates;
            raim.stat_full = stat_full;
            raim.stat = swrr / sigma2;
            raim.threshold = thr;
            break;
        }
        gpsacq_atm_params p = a.p;
        p.flags = flags;
        const Site g = raim_site(lat, lon, alt, base_s + st.trx, flags);
        raim_delays(r, mask, st, g, p, false);
    }
    // the winning lane: the row's three records
    out.iterations = row->steps + steps;
    *fix_out = out;
    *dop_out = dop;
    *raim_out = raim;
}

void launch_raim_detect(const RaimArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_raim_detect, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_raim_exclude(const RaimArgs& a, hipStream_t s) {
    const size_t lanes = a.n_fix * RAIM_GROUP;
    hipLaunchKernelGGL(k_raim_exclude, dim3((unsigned)((lanes + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
