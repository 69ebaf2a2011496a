// aided_kernels.hip -- "Aided acquisition: predicted code phase and Doppler, windowed search" of include/gpsacq.h.
//
// k_aid_predict: one lane per (fix, channel), in fp64 on nav_device.hpp (split, week_ms, earth_turn, geodetic, view_of) and
// orbit_device.hpp (the one orbit evaluation): the two light-time passes of k_coarse_fix's step A from the fix's place (one loop
// body), then the satellite's state and rate at the time its replica shows, k_vel's row read backwards and k_sat_view's elevation.
// No LDS, no barrier, no atomics; every loop is bounded.
//
// k_aided: one workgroup of AIDED_WAVES wave64 per task.  The PRN's chips go into LDS as in k_refine; wave w takes the segments
// w, w + 4, ... of the window, and per Doppler hypothesis d and segment it does two things.
//   BUILD.  The segment's 32-sample words (and the 2 W / 32 + 1 words behind them, for the chip stream alone) are shared out over
//     the lanes; each word is built ONCE with k_refine's word_pos / word_masks<false> (capture_words.hpp): the samples, the bits
//     that belong to the segment, the cos and -sin masks and the prompt chips of hypothesis h = 0, which at sample j + h are the
//     chips of hypothesis h at sample j.  Into the wave's own LDS go {x ^ cos, x ^ ~sin, valid} per word (one 16-byte entry) and
//     the chip-mask stream, one word per 32 samples.
//   WALK.  After a wave-local wait lane l owns code hypothesis h = l (l + 64, l + 128, l + 192 in further passes over the same
//     masks).  It walks the segment's words: every lane reads the same 16-byte entry (a broadcast), lanes 0..31 and 32..63 read one
//     stream word each (two broadcasts), the lane cuts its chip mask out of the stream word it kept from the last step and the
//     new one with a funnel shift by h & 31 (word offset h >> 5), and takes two xor-popcounts over the WHOLE word: the bits that
//     are not the segment's (only its first and last word have any) are counted once more by themselves and taken off.  Five
//     vector instructions and two LDS reads per word serve 64 hypotheses; nothing crosses lanes.  At the segment's end the lane
//     squares its own I and Q into its own uint64.
// A segment of more than AIDED_CHUNK words (spm above 6100) is built and walked in chunks; the counts carry over.  Once per d the four
// waves' sums meet in LDS (two barriers), thread h adds them, writes power(h, d), and keeps its total and the largest KEY
// power << 13 | (31 - d) << 8 | (255 - h) (power < 2^39: include/gpsacq.h, step 4): the maximum of the keys over the workgroup is
// the record's best, whatever the order.  Steps 1 and 2 (kept, no aid) and the record and peak are built in snapshot_records.hpp
// (aided_prologue, aided_record; aided_coh_record for k_aided_coh), which the kernels of aided_iq_kernels.hip and
// aided_coh_iq_kernels.hip call too: this file unpacks its key and brings the floor 2 spm segments.
// No atomics.  Every loop is bounded by kernel arguments; s_x is indexed below AIDED_CHUNK, s_stream below AIDED_CHUNK + 2 W / 32 + 1 <= AIDED_CHUNK + 8, s_pow below 2 W + 1 <= 255 (W <= 127 is checked by the
// host); nothing is read at or beyond byte n_bytes (word_at).
// Built with -ffp-contract=off (Makefile): the NCO words must be gpsacq_handoff_engine's to the bit, as in refine_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aided_launch.hpp"
#include "capture_words.hpp"
#include "nav_device.hpp"
#include "orbit_device.hpp"
#include "snapshot_records.hpp"

namespace acq {

namespace {
constexpr double L1_HZ = 1575.42e6;
constexpr int AIDED_CHUNK = 192;               // capture words built and walked at a time: 6144 samples
constexpr int AIDED_STREAM = AIDED_CHUNK + 8;  // and the stream words that go with them
static_assert((2 * AIDED_MAX_CODE_HALF >> 5) + 1 <= AIDED_STREAM - AIDED_CHUNK, "the stream's tail");
static_assert(2 * AIDED_MAX_CODE_HALF + 1 <= 64 * AIDED_PASSES && 2 * AIDED_MAX_DOP_HALF + 1 <= 32, "passes and key");

// BUILD and WALK of one segment [a0, a1) of a window that starts at sample o, on the calling wave's sx[AIDED_CHUNK] and
// st_all[AIDED_STREAM]: the ONE copy, for k_aided (PASSES = 4) and k_aided_coh (PASSES = 1).  Pass p serves code hypothesis
// h = lane + 64 p; ones_i[p], ones_q[p] are the samples of the segment whose product with cos and -sin is -1 (0 for h >= n_code),
// so that I = spm - 2 ones_i, Q = spm - 2 ones_q
template <int PASSES>
__device__ __forceinline__ void segment_ones(const uint32_t* words, size_t n_bytes, uint64_t a0, uint64_t a1, uint64_t o, uint64_t P0, uint32_t lo_rate,
                                             uint32_t ca_rate, const uint32_t* s_chips, uint4* sx, uint32_t* st_all, int lane, int n_code, int extra,
                                             uint32_t (&ones_i)[PASSES], uint32_t (&ones_q)[PASSES]) {
    const uint64_t w1 = (a1 - 1) >> 5;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) ones_i[p] = ones_q[p] = 0;
    for (uint64_t c0 = a0 >> 5; c0 <= w1; c0 += AIDED_CHUNK) {
        const int nw = w1 - c0 + 1 < (uint64_t)AIDED_CHUNK ? (int)(w1 - c0 + 1) : AIDED_CHUNK;
        for (int i = lane; i < nw + extra; i += 64) {
            const uint64_t wi = c0 + i;
            const WordPos w = word_pos(words, n_bytes, wi, a0, i < nw ? a1 : (wi << 5) + 32, o, P0, 0u, lo_rate, ca_rate, s_chips);
            uint32_t cm, sp, em, pm, lm;
            word_masks<false>(w, 0u, lo_rate, ca_rate, cm, sp, em, pm, lm);
            st_all[i] = pm;
            if (i < nw) sx[i] = make_uint4(w.x ^ cm, w.x ^ ~sp, w.valid, 0u);
        }
        wave_sync();
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int h = lane + 64 * p;
            if (h < n_code) {
                const int off = h >> 5;
                const uint32_t sh = (uint32_t)h & 31u;
                const uint32_t* st = &st_all[off];
                // the bits outside the segment, which only its first and last word have, are taken off again: the loop
                // counts whole words
                uint32_t below = st[0], above = st[1];
                const uint4 first = sx[0];
                uint32_t m = __funnelshift_r(below, above, sh);
                uint32_t ci = 0u - __popc((first.x ^ m) & ~first.z), cq = 0u - __popc((first.y ^ m) & ~first.z);
                if (nw > 1) {
                    const uint4 last = sx[nw - 1];
                    m = __funnelshift_r(st[nw - 1], st[nw], sh);
                    ci -= __popc((last.x ^ m) & ~last.z), cq -= __popc((last.y ^ m) & ~last.z);
                }
#pragma unroll 4
                for (int i = 0; i < nw; ++i) {
                    above = st[i + 1];
                    m = __funnelshift_r(below, above, sh);
                    const uint2 x = *reinterpret_cast<const uint2*>(&sx[i]);
                    ci += __popc(x.x ^ m);
                    cq += __popc(x.y ^ m);
                    below = above;
                }
                ones_i[p] += ci, ones_q[p] += cq;
            }
        }
        wave_sync();
    }
}
}  // namespace

__global__ __launch_bounds__(NAV_BLOCK) void k_aid_predict(AidPredictArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_fix * (size_t)a.chans) return;
    const size_t f = i / (size_t)a.chans;
    const int c = (int)(i % (size_t)a.chans);
    gpsacq_aid out = {0, 0, 0, 0, 0.0, 0.0, 0.0};
    const gpsacq_fix fix = a.fix[f];
    if (fix.status != GPSACQ_FIX_OK) {
        out.flags = GPSACQ_AID_NO_FIX;
    } else if (c >= a.n_eph || !a.eph[c].valid) {
        out.flags = GPSACQ_AID_NO_EPH;
    } else {
        const NavEph& p = a.eph[c];
        // light time
        double tau = 75e-3, cc = 0.0, k, frac, sn, cs;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {  // at -75 ms, then at -tau
            split(fix.rx_frac + -tau, k, frac);
            const gpsacq_sat_state st = sat_state(orbit_at(p, week_ms(fix.rx_ms, k), frac));
            sincos(-OMEGA_E * tau, &sn, &cs);
            const double dx = fix.x - (st.x * cs - st.y * sn), dy = fix.y - (st.x * sn + st.y * cs), dz = fix.z - st.z;
            tau = sqrt(dx * dx + dy * dy + dz * dz) / C;
            cc = st.clock_corr;
        }
        // code
        split(fix.rx_frac + (cc - tau), k, frac);
        const gpsacq_obs o = {c, 1, week_ms(fix.rx_ms, k), 0, frac, 1.0};
        // Doppler
        const Orbit orb = orbit_at(p, o.tx_ms, o.tx_frac);
        const gpsacq_sat_state st = sat_state(orb);
        const gpsacq_sat_rate sr = sat_state_rate(p, orb);
        earth_turn(o, st, fix, sn, cs);
        const double qx = sr.vx - OMEGA_E * st.y, qy = sr.vy + OMEGA_E * st.x;  // v + Omega x p
        const double dx = (st.x * cs - st.y * sn) - fix.x, dy = (st.x * sn + st.y * cs) - fix.y, dz = st.z - fix.z;
        const double range = sqrt(dx * dx + dy * dy + dz * dz);
        const double ex = dx / range, ey = dy / range, ez = dz / range;
        double vx = 0.0, vy = 0.0, vz = 0.0, drift = 0.0;
        if (a.vel) {
            const gpsacq_vel v = a.vel[f];
            if (v.status == GPSACQ_VEL_OK) vx = v.vx, vy = v.vy, vz = v.vz, drift = v.drift;
        }
        const double wx = (qx * cs - qy * sn) - (vx - OMEGA_E * fix.y), wy = (qx * sn + qy * cs) - (vy + OMEGA_E * fix.x), wz = sr.vz - vz;
        const double rho = (ex * wx + ey * wy + ez * wz) + C * drift - C * sr.clock_drift;
        const double dop = -(L1_HZ / C) * rho;
        // elevation
        double lat, lon, alt;
        geodetic(fix.x, fix.y, fix.z, lat, lon, alt);
        const View v = view_of(make_site(lat, lon, alt, 0.0, 0), dx, dy, dz);
        const double elev = v.el * 180.0 / PI;
        if (!isfinite(range) || !isfinite(o.tx_frac) || !isfinite(dop) || !isfinite(elev)) {
            out.flags = GPSACQ_AID_NO_EPH;
        } else {
            out.tx_frac = o.tx_frac, out.doppler_hz = dop, out.elev_deg = elev;
            out.ca_center = (int32_t)nearbyint(o.tx_frac * a.fs) % a.spm;
            const double n = nearbyint(dop / a.step_hz);
            if (fabs(n) < 2147483648.0) out.lo_center = (int32_t)n;
            else out.flags |= GPSACQ_AID_OFF_GRID;
            if (out.lo_center < -a.kmax || out.lo_center > a.kmax) out.flags |= GPSACQ_AID_OFF_GRID;
            if (elev < a.p.elev_min_deg) out.flags |= GPSACQ_AID_LOW;
        }
    }
    a.out[i] = out;
}

__global__ __launch_bounds__(64 * AIDED_WAVES) void k_aided(AidedArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ uint4 s_x[AIDED_WAVES][AIDED_CHUNK];  // x ^ cos mask, x ^ ~sin mask, the bits of the segment, unused
    __shared__ uint32_t s_stream[AIDED_WAVES][AIDED_STREAM];
    __shared__ unsigned long long s_pow[AIDED_WAVES][64 * AIDED_PASSES];
    __shared__ unsigned long long s_red[AIDED_WAVES][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const int W = a.p.code_half, K = a.p.dop_half, n_code = 2 * W + 1, n_dop = 2 * K + 1;
    unsigned long long* const powers = a.powers ? a.powers + t * (size_t)(n_dop * n_code) : nullptr;

    // 1. kept, 2. no aid: the flag and zeros (snapshot_records.hpp)
    const gpsacq_aid aid = a.aid[t];
    gpsacq_peak pk_out;
    Window win;
    int d_first;
    if (!aided_prologue(a, t, aid, powers, n_dop * n_code, pk_out, win, d_first)) return;
    chips_to_lds(a.c.chips, win.prn, s_chips);
    __syncthreads();

    // 3. hypotheses, 4. sums
    const uint64_t o = win.o, spm = (uint64_t)a.c.spm, segments = win.segments;
    const uint32_t base = aided_base(aid, W, a.c.spm);
    const int extra = (2 * W >> 5) + 1;  // stream words behind a chunk's capture words
    uint64_t total = 0, key = 0;         // of hypothesis h = threadIdx.x
    for (int d = 0; d < n_dop; ++d) {
        const Window wd = window_at(a, t, (int64_t)aid.lo_center - K + d);
        if (!wd.hit) {  // every lane decides the same
            if (powers && (int)threadIdx.x < n_code) powers[d * n_code + threadIdx.x] = 0;
            continue;
        }
        const uint32_t lo_rate = wd.lo_rate, ca_rate = wd.ca_rate;
        const uint64_t P0 = (uint64_t)base * ca_rate % FULL;
        uint64_t acc[AIDED_PASSES] = {0, 0, 0, 0};
        for (uint64_t s = wv; s < segments; s += AIDED_WAVES) {
            const uint64_t a0 = o + s * spm;  // the segment's samples [a0, a0 + spm), counted from the aligned base
            uint32_t ones_i[AIDED_PASSES], ones_q[AIDED_PASSES];
            segment_ones<AIDED_PASSES>(a.c.words, a.c.n_bytes, a0, a0 + spm, o, P0, lo_rate, ca_rate, s_chips, s_x[wv], s_stream[wv], lane, n_code, extra, ones_i,
                                       ones_q);
#pragma unroll
            for (int p = 0; p < AIDED_PASSES; ++p) {
                const int64_t I = (int64_t)a.c.spm - 2 * (int64_t)ones_i[p], Q = (int64_t)a.c.spm - 2 * (int64_t)ones_q[p];
                acc[p] += (uint64_t)(I * I + Q * Q);
            }
        }
#pragma unroll
        for (int p = 0; p < AIDED_PASSES; ++p) s_pow[wv][lane + 64 * p] = acc[p];
        __syncthreads();
        if ((int)threadIdx.x < n_code) {
            uint64_t pw = 0;
            for (int w = 0; w < AIDED_WAVES; ++w) pw += s_pow[w][threadIdx.x];
            if (powers) powers[d * n_code + threadIdx.x] = pw;
            total += pw;
            const uint64_t kd = pw << 13 | (uint64_t)(31 - d) << 8 | (uint64_t)(255 - threadIdx.x);
            key = kd > key ? kd : key;
        }
        __syncthreads();
    }

    // 5. record, 6. peak: the largest key and the total over the workgroup, then snapshot_records.hpp
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t other = shfl_xor64(key, m);
        key = other > key ? other : key;
        total += shfl_xor64(total, m);
    }
    if (lane == 0) s_red[wv][0] = key, s_red[wv][1] = total;
    __syncthreads();
    if (threadIdx.x != 0) return;
    key = total = 0;
    for (int w = 0; w < AIDED_WAVES; ++w) {
        key = s_red[w][0] > key ? s_red[w][0] : key;
        total += s_red[w][1];
    }
    // the key unpacked; the floor of a +-1 stream
    aided_record(a, t, aid, base, segments, win.fit, key >> 13, 255 - (int32_t)(key & 255), 31 - (int32_t)(key >> 8 & 31), total, 2 * spm * segments, pk_out);
}

// ---- "Coherent aided acquisition: 20 ms sums, bit edge and fine Doppler" of include/gpsacq.h -------------------------------------
//
// k_aided_coh<M>: one workgroup of AIDED_WAVES wave64 per task, two stages per Doppler hypothesis d.
//   CORRELATION.  k_aided's BUILD and WALK at one pass (2 W + 1 <= 63 hypotheses, lane h owns h): segment_ones<1>() above, the
//     walk both kernels call; instead of squaring, lane h stores (I, Q) as an int32 pair into s_z[s * n_code + h].
//   COHERENT.  After a barrier the work item is (h, g), item g * n_code + h on thread item % 256: neighbouring lanes read
//     neighbouring 8-byte entries of a z row (no bank conflict), lanes of equal h and different g the same entry (a broadcast).
//     One walk over the segments: the table entry (C | S << 16, one LDS word) at k, k += f u mod 1024; the turned sums go into
//     the prefix (PA, PB); segment s closes the period of edge e = s mod M alone, as the prefix minus the prefix kept at that
//     edge's last boundary (LA[e], LB[e]).  The walk is unrolled by M from a multiple of M, so e is the unrolled index and the
//     three arrays of M live in registers.  The last, partial period of every e closes after the walk.  An edge that closes at
//     s = 0 (e = 0) or never (e >= S) adds an empty period, 0.
//   Per d the largest key of the workgroup is found (shuffles, one LDS step) and every thread keeps the running best and the
//   non-coherent sum of its (h, d), which item (h, g = 0) left in s_nc.  No atomics.
// LDS: s_chips 136 + s_x 12288 + s_stream 3200 + s_z 40960 + s_tab 4096 + s_nc 512 + s_red 32 = 61224 bytes.  s_z is indexed
// below segments * n_code <= fit * (2 W + 1) <= COH_MAX_Z (checked by the host), s_tab below 1024 (masked), s_nc below 64.
template <int M> __global__ __launch_bounds__(64 * AIDED_WAVES) void k_aided_coh(AidedCohArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ uint4 s_x[AIDED_WAVES][AIDED_CHUNK];
    __shared__ uint32_t s_stream[AIDED_WAVES][AIDED_STREAM];
    __shared__ int2 s_z[COH_MAX_Z];
    __shared__ uint32_t s_tab[COH_TABLE];  // C[k] in the low half, S[k] in the high half
    __shared__ unsigned long long s_nc[64];
    __shared__ unsigned long long s_red[AIDED_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const int W = a.p.code_half, K = a.p.dop_half, F = a.p.fine_half, n_code = 2 * W + 1, n_dop = 2 * K + 1, n_fine = 2 * F + 1;
    const int row = n_fine * M * n_code;  // powers of one d
    unsigned long long* const powers = a.powers ? a.powers + t * (size_t)(n_dop * row) : nullptr;

    // 1. kept, 2. no aid: the flag and zeros (snapshot_records.hpp)
    const gpsacq_aid aid = a.aid[t];
    gpsacq_peak pk_out;
    Window win;
    int d_first;
    if (!aided_prologue(a, t, aid, powers, n_dop * row, pk_out, win, d_first)) return;
    chips_to_lds(a.c.chips, win.prn, s_chips);
    for (int i = threadIdx.x; i < COH_TABLE; i += 64 * AIDED_WAVES)
        s_tab[i] = (uint32_t)(uint16_t)a.table[i] | (uint32_t)(uint16_t)a.table[COH_TABLE + i] << 16;
    __syncthreads();

    const uint64_t o = win.o, spm = (uint64_t)a.c.spm;
    const int S = (int)win.segments;  // S * n_code <= COH_MAX_Z
    const uint32_t base = aided_base(aid, W, a.c.spm);
    const int extra = (2 * W >> 5) + 1;
    const int items = n_code * n_fine;
    uint64_t best_key = 0, best_nc = 0;  // the same in every thread
    for (int d = 0; d < n_dop; ++d) {
        const Window wd = window_at(a, t, (int64_t)aid.lo_center - K + d);
        if (!wd.hit) {  // every lane decides the same
            if (powers)
                for (int i = threadIdx.x; i < row; i += 64 * AIDED_WAVES) powers[d * row + i] = 0;
            continue;
        }
        // 4. segment sums
        const uint64_t P0 = (uint64_t)base * wd.ca_rate % FULL;
        for (int s = wv; s < S; s += AIDED_WAVES) {
            const uint64_t a0 = o + (uint64_t)s * spm;
            uint32_t ones_i[1], ones_q[1];
            segment_ones<1>(a.c.words, a.c.n_bytes, a0, a0 + spm, o, P0, wd.lo_rate, wd.ca_rate, s_chips, s_x[wv], s_stream[wv], lane, n_code, extra, ones_i, ones_q);
            if (lane < n_code) s_z[s * n_code + lane] = make_int2(a.c.spm - 2 * (int32_t)ones_i[0], a.c.spm - 2 * (int32_t)ones_q[0]);
        }
        __syncthreads();
        // 5. coherent sums
        uint64_t key = 0;
        for (int it = threadIdx.x; it < items; it += 64 * AIDED_WAVES) {
            const int g = it / n_code, h = it - g * n_code;
            const uint32_t step = (uint32_t)((g - F) * a.p.fine_step) & (COH_TABLE - 1);  // (f u) mod 1024, a true modulo
            uint32_t k = 0;
            int64_t PA = 0, PB = 0, LA[M], LB[M];
            uint64_t acc[M], nc = 0;
#pragma unroll
            for (int j = 0; j < M; ++j) LA[j] = LB[j] = 0, acc[j] = 0;
            for (int s0 = 0; s0 < S; s0 += M) {
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const int s = s0 + j;  // s mod M == j
                    if (s < S) {
                        acc[j] += sq2((PA - LA[j]) >> 14, (PB - LB[j]) >> 14);
                        LA[j] = PA, LB[j] = PB;
                        const int2 z = s_z[s * n_code + h];
                        const uint32_t cs = s_tab[k];
                        const int64_t c = (int16_t)(cs & 0xffffu), sn = (int16_t)(cs >> 16);
                        PA += z.x * c + z.y * sn;
                        PB += z.y * c - z.x * sn;
                        nc += sq2(z.x, z.y);
                        k = (k + step) & (COH_TABLE - 1);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const uint64_t pw = acc[j] + sq2((PA - LA[j]) >> 14, (PB - LB[j]) >> 14);
                if (powers) powers[d * row + (g * M + j) * n_code + h] = pw;
                const uint64_t kd = pw << COH_KEY_SHIFT | (uint64_t)(31 - d) << 15 | (uint64_t)(15 - g) << 11 | (uint64_t)(31 - j) << 6 | (uint64_t)(63 - h);
                key = kd > key ? kd : key;
            }
            if (g == 0) s_nc[h] = nc;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t other = shfl_xor64(key, m);
            key = other > key ? other : key;
        }
        if (lane == 0) s_red[wv] = key;
        __syncthreads();  // also: every thread is done with s_z before the next d writes it
        for (int w = 0; w < AIDED_WAVES; ++w) key = s_red[w] > key ? s_red[w] : key;
        if (key > best_key) best_key = key, best_nc = s_nc[63 - (int)(key & 63)];
        // s_red and s_nc are written again only behind the next d's first barrier
    }

    // 6. record and peak: the key unpacked and the floor of a +-1 stream, then snapshot_records.hpp
    if (threadIdx.x != 0) return;
    aided_coh_record(a, t, aid, base, (uint64_t)S, win.fit, M, best_key >> COH_KEY_SHIFT, 63 - (int32_t)(best_key & 63), 31 - (int32_t)(best_key >> 15 & 31),
                     15 - (int32_t)(best_key >> 11 & 15), 31 - (int32_t)(best_key >> 6 & 31), best_nc, 2 * spm * (uint64_t)S, pk_out);
}

// "THE RECEIVE INSTANT ON THE DEVICE": one lane per fix; the record travels as ten 64-bit words so that a copy is byte for byte
__global__ __launch_bounds__(NAV_BLOCK) void k_aid_instant(AidInstantArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_fix) return;
    static_assert(sizeof(gpsacq_fix) == 80, "ten words");
    union {
        gpsacq_fix f;
        uint64_t w[10];
    } u;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(a.fix + i);
    for (int k = 0; k < 10; ++k) u.w[k] = src[k];
    if (u.f.status == GPSACQ_FIX_OK) {
        const gpsacq_coarse_info in = a.info[i];
        const double tt = nearbyint(1e3 * in.coarse_s) * 1e-3 - in.bias_m / C;
        const double k = floor(1e3 * tt);
        if (!isfinite(in.coarse_s) || !isfinite(in.bias_m) || !(k >= -2147483648.0 && k <= 2147483647.0)) {
            u.f.status = GPSACQ_FIX_NO_CONVERGE;
        } else {
            int64_t ms = ((int64_t)a.prior[i].rx_ms + (int64_t)k) % WEEK_MS;
            if (ms < 0) ms += WEEK_MS;
            u.f.rx_ms = (int32_t)ms;
            u.f.rx_frac = tt - 1e-3 * k;
        }
    }
    uint64_t* dst = reinterpret_cast<uint64_t*>(a.out + i);
    for (int k = 0; k < 10; ++k) dst[k] = u.w[k];
}

void launch_aided_coh(const AidedCohArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.c.n_tasks), block(64 * AIDED_WAVES);
    switch (a.p.coh_ms) {  // the host has checked that it is one of these
        case 1: hipLaunchKernelGGL(k_aided_coh<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_aided_coh<2>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_aided_coh<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_aided_coh<5>, grid, block, 0, s, a); break;
        case 10: hipLaunchKernelGGL(k_aided_coh<10>, grid, block, 0, s, a); break;
        case 20: hipLaunchKernelGGL(k_aided_coh<20>, grid, block, 0, s, a); break;
    }
}

void launch_aid_instant(const AidInstantArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_aid_instant, dim3((unsigned)((a.n_fix + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_aid_predict(const AidPredictArgs& a, hipStream_t s) {
    const size_t n = a.n_fix * (size_t)a.chans;
    hipLaunchKernelGGL(k_aid_predict, dim3((unsigned)((n + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

void launch_aided(const AidedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_aided, dim3((unsigned)a.c.n_tasks), dim3(64 * AIDED_WAVES), 0, s, a);
}

}  // namespace acq
