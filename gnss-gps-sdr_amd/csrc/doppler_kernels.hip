// doppler_kernels.hip -- "Cold snapshot fixes: fine Doppler and a Doppler-only position solver" of include/gpsacq.h.
//
// k_fine_dop: one workgroup of DOP_WAVES wave64 per task, k_refine's word loop (capture_words.hpp holds the one copy) with the
// prompt replica alone: per 32-sample word three masks (cos, -sin, prompt chips; D = 0, so the 32-chip window starts at the prompt
// chip of bit 0) and two popcounts.  The two counts of a segment pack into one register (spm <= 65535), are summed over the wave
// with xor shuffles, and lane 0 leaves the segment's (I, Q) in LDS as two int32.  After ONE barrier thread i takes the segments
// i, i + 256, ...: the power of s and, from s = 1 on, the lag-1 product of the squares of s and s - 1.  The four 64-bit sums are
// added in unsigned arithmetic modulo 2^64 (re and im are read back as int64: the host has refused every engine whose sums could
// leave the int64 range, so the wrap-around never shows), reduced over the wave with 32-bit shuffles of their halves, and meet in
// LDS, where thread 0 adds the four waves' and writes the record (dopfine_record of snapshot_records.hpp builds it, for this kernel
// and for k_fine_dop_iq).  No atomics, no float before the estimate: the record does not
// depend on the order of anything.  Two barriers; every loop is bounded by kernel arguments; s < segments <= DOP_MAX_SEGMENTS
// (checked by the host) bounds every LDS index.
// k_rate_obs_fine: one lane per (fix, channel), a record into the rate observation k_vel and k_doppler_fix read.
// k_doppler_fix: one lane per fix.  As k_coarse_fix it holds nothing of the row in registers: the satellite loop of every pass
// is ONE body (#pragma unroll 1) that reads the column back from memory -- eph and the two valid flags, Doppler and weight, and
// its light time from `tau` (engine scratch, -1 for a column that is not usable) -- evaluates the orbit (orbit_device.hpp) and
// adds into the 10 + 4 sums of the weighted normal equations and the 10 of the unweighted ones pdop is read from (two Sym<4>
// of spd_device.hpp: add_row, factor, solve, and inverse_lower / inverse_diagonal for pdop).  The orbit code
// is inlined twice: the start (positions only) and the Newton body.  No LDS, no barrier, no atomics; every loop is bounded.
// Built with -ffp-contract=off (Makefile): the NCO words must be gpsacq_handoff_engine's to the bit, as in refine_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture_words.hpp"
#include "doppler_launch.hpp"
#include "nav_device.hpp"
#include "orbit_device.hpp"
#include "snapshot_records.hpp"

namespace acq {

namespace {
constexpr int DOPFINE_UNUSABLE = GPSACQ_DOPFINE_NO_HIT | GPSACQ_DOPFINE_NO_POWER | GPSACQ_DOPFINE_FEW | GPSACQ_DOPFINE_WEAK;
constexpr double L1_HZ = 1575.42e6;
constexpr double EARTH_R = 6371000.0;  // the sphere the solver starts on, metres

}  // namespace

__global__ __launch_bounds__(64 * DOP_WAVES) void k_fine_dop(FineDopArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ int32_t s_iq[DOP_MAX_SEGMENTS][2];
    __shared__ unsigned long long s_part[DOP_WAVES][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const gpsacq_peak pk = a.c.peaks[t];

    // steps 1 to 3 of "Fine code phases"
    double base_hz;
    const Window win = window_of(pk, a.c, t, a.p.snr_min, a.p.blocks, base_hz);
    const uint64_t o = win.o, spm = (uint64_t)a.c.spm, segments = win.segments;
    const uint32_t lo_rate = win.lo_rate, ca_rate = win.ca_rate;
    if (!win.hit) {
        if (threadIdx.x == 0) a.out[t] = gpsacq_dopfine{GPSACQ_DOPFINE_NO_HIT, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0};
        return;
    }
    chips_to_lds(a.c.chips, win.prn, s_chips);
    __syncthreads();

    // prompt sums
    const uint64_t P0 = (uint64_t)pk.ca_shift * ca_rate % FULL;
    for (uint64_t s = wv; s < segments; s += DOP_WAVES) {
        const uint64_t a0 = o + s * spm, a1 = a0 + spm;  // the segment's samples [a0, a1), counted from the aligned base
        const uint64_t w1 = (a1 - 1) >> 5;
        uint32_t ones_i = 0, ones_q = 0;  // samples whose product is -1
        for (uint64_t wi = (a0 >> 5) + lane; wi <= w1; wi += 64) {
            const WordPos w = word_pos(a.c.words, a.c.n_bytes, wi, a0, a1, o, P0, 0u, lo_rate, ca_rate, s_chips);
            uint32_t cm, sp, em, pm, lm;
            word_masks<false>(w, 0u, lo_rate, ca_rate, cm, sp, em, pm, lm);
            ones_i += __popc((w.x ^ pm ^ cm) & w.valid);
            ones_q += __popc((w.x ^ pm ^ ~sp) & w.valid);
        }
        uint32_t pkd = ones_i | ones_q << 16;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) pkd += (uint32_t)__shfl_xor((int)pkd, m, 64);
        if (lane == 0) {
            s_iq[s][0] = a.c.spm - 2 * (int32_t)(pkd & 0xFFFF);
            s_iq[s][1] = a.c.spm - 2 * (int32_t)(pkd >> 16);
        }
    }
    __syncthreads();

    // squares and lag-1 sums, modulo 2^64
    uint64_t re = 0, im = 0, mag = 0, power = 0;
    for (uint64_t s = threadIdx.x; s < segments; s += 64 * DOP_WAVES) {
        const int64_t I = s_iq[s][0], Q = s_iq[s][1];
        const uint64_t pw = (uint64_t)(I * I + Q * Q);
        power += pw;
        if (s >= 1) {
            const int64_t I1 = s_iq[s - 1][0], Q1 = s_iq[s - 1][1];
            const uint64_t A = (uint64_t)(I * I - Q * Q), B = (uint64_t)(2 * I * Q);
            const uint64_t A1 = (uint64_t)(I1 * I1 - Q1 * Q1), B1 = (uint64_t)(2 * I1 * Q1);
            re += A * A1 + B * B1;
            im += B * A1 - A * B1;
            mag += pw * (uint64_t)(I1 * I1 + Q1 * Q1);
        }
    }
    re = wave_sum(re), im = wave_sum(im), mag = wave_sum(mag), power = wave_sum(power);
    if (lane == 0) s_part[wv][0] = re, s_part[wv][1] = im, s_part[wv][2] = mag, s_part[wv][3] = power;
    __syncthreads();
    if (threadIdx.x != 0) return;

    // estimate, flags: snapshot_records.hpp.  lo_rate is read UNSIGNED: fc + lo_dop may pass fs / 2 on a real capture
    re = im = mag = power = 0;
    for (int w = 0; w < DOP_WAVES; ++w) re += s_part[w][0], im += s_part[w][1], mag += s_part[w][2], power += s_part[w][3];
    const double nco_hz = ((double)lo_rate * a.c.fs) / 4294967296.0;
    a.out[t] = dopfine_record(segments, win.fit, a.p, lo_rate, ca_rate, re, im, mag, power, nco_hz, base_hz, (double)a.c.spm / a.c.fs);
}

__global__ __launch_bounds__(NAV_BLOCK) void k_rate_obs_fine(RateObsFineArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_peak pk = a.peaks[i];
    const gpsacq_dopfine f = a.dopfine[i];
    gpsacq_rate_obs o = {0, 0, 0, 0.0, 0.0};
    if ((double)pk.snr >= a.snr_min && !(f.flags & DOPFINE_UNUSABLE) && isfinite(f.doppler_hz)) {
        o.valid = 1;
        o.doppler_hz = f.doppler_hz;
        o.weight = 1.0;
    }
    a.out[i] = o;
}

namespace {
// a column of k_doppler_fix's row as the passes read it back
struct Column {
    bool usable;
    int32_t eph;
    double doppler_hz, weight;
};

__device__ __forceinline__ Column column_of(const DopplerFixArgs& a, size_t i) {
    const gpsacq_obs o = a.obs[i];
    const gpsacq_rate_obs ro = a.rate_obs[i];
    Column c = {false, o.eph, ro.doppler_hz, ro.weight};
    c.usable = o.valid != 0 && ro.valid != 0 && o.eph >= 0 && o.eph < a.n_eph && isfinite(ro.doppler_hz) && isfinite(ro.weight) && ro.weight >= 0.0;
    if (c.usable) c.usable = a.eph[o.eph].valid != 0;
    return c;
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_doppler_fix(DopplerFixArgs a) {
    const size_t f = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (f >= a.n_fix) return;
    const size_t row = f * (size_t)a.sats;
    double* tau = a.tau + row;
    const int32_t rx_ms = a.rx_ms[f];
    const bool time_ok = rx_ms >= 0 && rx_ms < WEEK_MS;

    // START: the usable columns, their light times, the mean satellite direction
    int n_used = 0;
    double ux = 0.0, uy = 0.0, uz = 0.0;
#pragma unroll 1
    for (int s = 0; s < a.sats; ++s) {
        const Column c = column_of(a, row + s);
        const bool use = time_ok && c.usable;
        tau[s] = use ? 75e-3 : -1.0;
        if (!use) continue;
        double k, frac, sn, cs;
        split(-75e-3, k, frac);
        const gpsacq_sat_state st = sat_state(orbit_at(a.eph[c.eph], week_ms(rx_ms, k), frac));
        sincos(-OMEGA_E * 75e-3, &sn, &cs);
        const double rx = st.x * cs - st.y * sn, ry = st.x * sn + st.y * cs, rz = st.z;
        const double inv = 1.0 / sqrt(rx * rx + ry * ry + rz * rz);
        ux += rx * inv, uy += ry * inv, uz += rz * inv;
        n_used += 1;
    }

    gpsacq_doppler_fix out = {GPSACQ_FIX_TOO_FEW, n_used, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double x = 0.0, y = 0.0, z = 0.0, g = 0.0, rms = 0.0, pdop = 0.0;
    bool ok = false;
    if (n_used >= 4) {
        out.status = GPSACQ_FIX_NO_CONVERGE;
        const double un = sqrt(ux * ux + uy * uy + uz * uz);
        const bool start = un >= 1e-6;
        if (start) x = EARTH_R * ux / un, y = EARTH_R * uy / un, z = EARTH_R * uz / un;
#pragma unroll 1
        for (int pass = 0; start && pass < FIX_PASSES; ++pass) {
            Sym<4> n = {}, m = {};  // weighted; unweighted over weight > 0
            double b[4] = {}, swrr = 0;
#pragma unroll 1
            for (int s = 0; s < a.sats; ++s) {
                const double t = tau[s];
                if (t < 0.0) continue;
                const Column c = column_of(a, row + s);
                const NavEph& p = a.eph[c.eph];
                double k, frac, sn, cs;
                split(-t, k, frac);
                const Orbit orb = orbit_at(p, week_ms(rx_ms, k), frac);
                const gpsacq_sat_state st = sat_state(orb);
                const gpsacq_sat_rate sr = sat_state_rate(p, orb);
                sincos(-OMEGA_E * t, &sn, &cs);
                const double qx = sr.vx - OMEGA_E * st.y, qy = sr.vy + OMEGA_E * st.x;  // v + Omega x p
                const double dx = (st.x * cs - st.y * sn) - x, dy = (st.x * sn + st.y * cs) - y, dz = st.z - z;
                const double range = sqrt(dx * dx + dy * dy + dz * dz);
                const double inv = 1.0 / range;
                const double ex = dx * inv, ey = dy * inv, ez = dz * inv;
                const double wx = (qx * cs - qy * sn) + OMEGA_E * y, wy = (qx * sn + qy * cs) - OMEGA_E * x, wz = sr.vz;  // vi - Omega x (x, y, z)
                const double ew = ex * wx + ey * wy + ez * wz;
                const double pred = (ew + g) - C * sr.clock_drift;
                const double res = -(C / L1_HZ) * c.doppler_hz - pred;
                const double h[4] = {-(wx - ew * ex) * inv - OMEGA_E * ey, -(wy - ew * ey) * inv + OMEGA_E * ex, -(wz - ew * ez) * inv, 1.0};
                const double w = c.weight;
                add_row(n, b, h, w, res);
                swrr += w * res * res;
                if (w > 0.0) add_row(m, h, 1.0);
                tau[s] = range / C;
            }
            rms = sqrt(swrr / n(3, 3));
            Sym<4> l;
            if (!factor(n, l)) break;
            double d[4];
            solve(l, b, d);
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (!isfinite(step) || !isfinite(d[3])) break;
            x += d[0], y += d[1], z += d[2], g += d[3];
            out.iterations += 1;
            if (!(sqrt(x * x + y * y + z * z) <= 1e8)) break;
            if (step < 1e-3) {  // the step just applied was the last one: pdop from the rows it was made from
                if (factor(m, l)) {
                    Sym<4> li;
                    double q[4];
                    inverse_lower(l, li);
                    inverse_diagonal(li, q);
                    const double pd = sqrt(q[0] + q[1] + q[2]);
                    if (isfinite(pd)) pdop = pd;
                }
                ok = true;
                break;
            }
        }
    }

    gpsacq_coarse_prior pr = {nan(""), nan(""), nan(""), rx_ms, 0};
    if (ok) {
        out.status = GPSACQ_FIX_OK;
        out.x = x, out.y = y, out.z = z;
        geodetic(x, y, z, out.lat, out.lon, out.alt);
        out.drift = g / C;
        out.rms = rms;
        out.pdop = pdop;
        if (n_used >= 5 && rms > a.p.rms_max_mps) out.flags |= GPSACQ_DOPPLER_INCONSISTENT;
        else pr.x = x, pr.y = y, pr.z = z;
    }
    a.out[f] = out;
    if (a.prior) a.prior[f] = pr;
}

void launch_fine_dop(const FineDopArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fine_dop, dim3((unsigned)a.c.n_tasks), dim3(64 * DOP_WAVES), 0, s, a);
}

void launch_rate_obs_fine(const RateObsFineArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_rate_obs_fine, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_doppler_fix(const DopplerFixArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_doppler_fix, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
