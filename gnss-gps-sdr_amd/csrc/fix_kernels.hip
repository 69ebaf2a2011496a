// fix_kernels.hip -- the position fixes of include/gpsacq.h that run the stage loop, and the view from a fix, all in fp64, written
// on nav_device.hpp's solver: "Atmosphere, elevation mask and DOP" (k_sat_view, k_fix_atm) and "Fix integrity: residual test and
// single-satellite exclusion" (k_raim_detect, k_raim_exclude).  The plain fix, k_fix, is nav_kernels.hip's.
//
// k_sat_view: one lane per observation: azimuth, elevation, Klobuchar and Saastamoinen delay of a satellite seen from a fix.
// k_fix_atm: one lane per fix.  full_fix() -- stage 0 (k_fix's iteration), the elevation mask, GPSACQ_ATM_ROUNDS rounds of (delays
// at the current state, Newton from the current state) -- and the dilutions of precision.
// k_raim_detect: one lane per fix.  k_fix_atm's algorithm, whose ONE more pass over the row also gives the statistic T(S) at the
// converged state.  It writes gpsacq_fix, gpsacq_fix_dop and gpsacq_fix_raim of every row, and for a row that fails the test with
// something to exclude a RaimRow (raim_launch.hpp) in engine scratch.
// k_raim_exclude: sixteen lanes per fix, four fixes per wave64.  Every lane of a group holds the whole row in registers; lane k
// runs the Newton iteration over S \ {k} from the full solution's state with its delays held, the sixteen (T_k, k) are reduced
// to the smallest by four __shfl_xor exchanges of width 16 (no LDS, no atomics), and the winning lane alone goes on: FINAL's
// rounds, the statistic and DOP over the final set, and the row's three records.  Lanes 12-15 and lanes whose k is not in S or
// has weight 0 carry T = +inf.  The candidate solve and every round of FINAL are iterations of ONE stage loop, so the kernel holds
// one copy of the Newton pass and one of the statistic / DOP pass.  A group whose row did not ask for exclusion returns at once.
// Built with -mllvm -disable-machine-licm (Makefile): hoisted out of the stage loop, the fp64 constants of the inlined libm alone
// overflow the scalar registers (k_fix_atm: 72 spilled); left where they are used no kernel here has a spill or scratch, and
// k_sat_view fits five waves per SIMD instead of four (see DESIGN.md for the figures).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atm_launch.hpp"
#include "nav_device.hpp"
#include "raim_launch.hpp"

namespace acq {

__global__ __launch_bounds__(NAV_BLOCK) void k_sat_view(SatViewArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    gpsacq_sat_view v = {0.0, 0.0, 0.0, 0.0};
    const gpsacq_obs o = a.obs[i];
    const gpsacq_fix fix = a.fix[i / (size_t)a.sats];
    if (fix.status == GPSACQ_FIX_OK && usable(o, a.eph, a.n_eph)) {
        const gpsacq_sat_state st = a.state[i];
        double lat, lon, alt;
        geodetic(fix.x, fix.y, fix.z, lat, lon, alt);
        const Site g = make_site(lat, lon, alt, (double)fix.rx_ms * 1e-3 + fix.rx_frac, a.p.flags);
        double sn, cs;
        earth_turn(o, st, fix, sn, cs);
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
    Row r;
    load_row(a, f, r);
    gpsacq_fix out = blank_fix(GPSACQ_FIX_TOO_FEW, r.n_used);
    gpsacq_fix_dop dop = blank_dop(r.mask, 0);
    if (r.n_used >= 4) full_records(r, full_fix(r, a.p), out, dop);
    a.out[f] = out;
    a.dop[f] = dop;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_raim_detect(RaimArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    Row r;
    load_row(a, f, r);
    gpsacq_fix out = blank_fix(GPSACQ_FIX_TOO_FEW, r.n_used);
    gpsacq_fix_dop dop = blank_dop(r.mask, 0);
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

    const Full u = full_fix(r, a.p);
    const double swrr = full_records(r, u, out, dop);
    if (u.status == GPSACQ_FIX_OK) {
        // TEST
        const int d = __popc(u.mask & weighted(r)) - 4;
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
                    row->x = u.st.x, row->y = u.st.y, row->z = u.st.z, row->bias = u.st.bias;
                    row->t0 = r.t0;
#pragma unroll
                    for (int s = 0; s < S; ++s) row->delay[s] = r.dd[s];
                    row->stat_full = T;
                    row->mask = u.mask;
                    row->steps = u.steps;
                    row->n_masked = u.n_masked;
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
    load_row(a, f, r);
    r.t0 = row->t0;
#pragma unroll
    for (int s = 0; s < S; ++s) r.dd[s] = row->delay[s];
    const uint32_t full = row->mask;
    const uint32_t wmask = full & weighted(r);
    const int d = __popc(wmask) - 4;  // >= 2: k_raim_detect's test
    const uint32_t mask = full & ~(1u << k);
    const int n_masked = row->n_masked;
    const double stat_full = row->stat_full;
    double thr = a.r.threshold[0];  // threshold[d - 2], by select
#pragma unroll
    for (int j = 1; j < GPSACQ_RAIM_MAX_DOF; ++j) thr = d - 1 == j + 1 ? a.r.threshold[j] : thr;
    double sigma2 = a.r.sigma_m * a.r.sigma_m;
    const double base = base_s(r);
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
    gpsacq_fix out = blank_fix(GPSACQ_FIX_NO_CONVERGE, __popc(mask));
    gpsacq_fix_dop dop = blank_dop(mask, n_masked);
    gpsacq_fix_raim raim;
    raim.status = GPSACQ_RAIM_NONE;
    raim.dof = 0, raim.excluded = k, raim.n_candidates = 0;
    raim.stat_full = raim.stat = raim.threshold = 0.0;
    // stage 0: the candidate solve of every lane (k is a candidate where it is in S with weight > 0: never for k >= 12) and the
    // reduction; stages 1 .. rounds: FINAL's rounds, winner only
#pragma unroll 1
    for (int stage = 0; stage <= rounds; ++stage) {
        bool converged = false;
        if (stage > 0 || (wmask >> k & 1)) converged = newton(r, mask, st, steps);
        const bool last = stage == rounds;
        double swrr = INFINITY;
        Sym<4> n;
        if (converged && (stage == 0 || last)) swrr = residuals(r, mask, st, n);
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
        geodetic(st.x, st.y, st.z, lat, lon, alt);
        if (last) {
            out.status = GPSACQ_FIX_OK;
            fill_fix(out, r, st, lat, lon, alt);
            dop_of(n, lat, lon, dop);
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
        const Site g = make_site(lat, lon, alt, base + st.trx, flags);
        delays(r, mask, st, g, p, false);
    }
    // the winning lane: the row's three records
    out.iterations = row->steps + steps;
    *fix_out = out;
    *dop_out = dop;
    *raim_out = raim;
}

void launch_sat_view(const SatViewArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sat_view, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_fix_atm(const FixAtmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fix_atm, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_raim_detect(const RaimArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_raim_detect, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_raim_exclude(const RaimArgs& a, hipStream_t s) {
    const size_t lanes = a.n_fix * RAIM_GROUP;
    hipLaunchKernelGGL(k_raim_exclude, dim3((unsigned)((lanes + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
