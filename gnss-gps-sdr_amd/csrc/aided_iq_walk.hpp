// aided_iq_walk.hpp -- the chunk walk of the aided searches that go back to an 8-bit IQ capture, once: WIPE / STREAM / SUM by
// summation by parts over one segment of a window, as aided_iq_kernels.hip's head comment describes them.  k_aided_iq
// (PASSES = 4, 256 + 1024 + 256 slots) and aided_coh_iq_kernels.hip's k_aided_coh_iq (PASSES = 1, 64 + 512 + 64 slots) call it;
// nothing else does.  The geometry G of the calling wave's prefix array gives
//     G::CHUNK  samples whose prefix sums the wave holds at a time (a multiple of 8)
//     G::PAD    slots in front of them: A[k] sits in slot G::PAD + k, and the slots 0 .. G::PAD are zero from the kernel's start
// and the caller owes W with 2 W <= G::PAD - 2, an array of G::PAD + G::CHUNK + 2 W slots and a list of G::CHUNK + 2 W - 1 entries
// rounded up to a multiple of four (a stream of M + 1 positions has at most M transitions).  The array is read at slot
// G::PAD + m - h with m in [0, n + 2 W - 1] and h in [0, 64 * PASSES - 1], so in [1, G::PAD + n + 2 W - 1], and written in
// [G::PAD + 1, G::PAD + n + 2 W - 1]; the list is indexed below that size.  What can be checked at compile time is (below): the
// lanes of every pass stay inside the pad, the chunk is whole groups, and a list entry holds its position in 15 bits for any W the
// pad allows.  Nothing at or beyond byte 2 * n_samples of the capture is read (load_group).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture_groups.hpp"

namespace acq {

typedef uint16_t __attribute__((may_alias)) list_u16;  // the list is written entry by entry and read four entries at a time

// The segment [a0, a1) (capture samples) of a window that starts at sample o (a multiple of 8), on the calling wave's prefix array
// A and list lq: pass p serves code hypothesis h = lane + 64 p, and Ri[p], Rq[p] come back as the segment's (I_P, Q_P) of that
// hypothesis in wrap-around uint32 (the lanes beyond n_code hold sums that are not used).  fl is the lane's share of the
// segment's sum of v_i^2 + v_q^2 where with_floor, else 0: < 2^27, at most 1032 samples of a lane in a segment, 2^17 each
template <int PASSES, class G>
__device__ __forceinline__ void segment_sums_by_parts(const IqCaptureArgs& c, uint64_t a0, uint64_t a1, uint64_t o, uint32_t base, uint32_t lo_rate,
                                                      uint32_t ca_rate, const uint32_t* s_chips, int2* A, uint2* lq, int lane, int W, int n_code,
                                                      bool with_floor, uint32_t (&Ri)[PASSES], uint32_t (&Rq)[PASSES], uint32_t& fl) {
    static_assert(PASSES >= 1 && 64 * PASSES <= G::PAD, "lane h = lane + 64 p reads slot PAD + m - h >= 1");
    static_assert(G::CHUNK > 0 && G::CHUNK % 8 == 0, "a chunk is whole 8-sample groups");
    static_assert(G::CHUNK + G::PAD < (1 << 15), "a list entry: 15 bits of position (m <= CHUNK + 2 W - 1 < CHUNK + PAD), one of sign");
    list_u16* const list = reinterpret_cast<list_u16*>(lq);
    const size_t iq_bytes = 2 * c.n_samples;
    const int dc_i = c.dc_i, dc_q = c.dc_q;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) Ri[p] = Rq[p] = 0;
    fl = 0;
    for (uint64_t cs = a0 & ~7ull; cs < a1; cs += G::CHUNK) {
        const int n = a1 - cs < (uint64_t)G::CHUNK ? (int)((a1 - cs + 7) & ~7ull) : G::CHUNK;  // a multiple of 8
        const int M = n + 2 * W - 1;
        // WIPE
        uint32_t ci = 0, cq = 0;  // A of the groups before, the same in every lane
        for (int g0 = 0; g0 < n / 8; g0 += 64) {
            const int gl = g0 + lane;
            const bool mine = gl < n / 8;
            const uint64_t gs = cs + 8ull * (uint64_t)gl;
            uint32_t x[4] = {0, 0, 0, 0};
            if (mine) {
                const uint4 raw = load_group(c.iq, iq_bytes, gs >> 3);
                x[0] = raw.x ^ c.flip, x[1] = raw.y ^ c.flip, x[2] = raw.z ^ c.flip, x[3] = raw.w ^ c.flip;
            }
            const uint32_t b_lo = gs < a0 ? (uint32_t)(a0 - gs) : 0u;                       // 0 .. 7
            const uint32_t b_hi = !mine || gs >= a1 ? 0u : gs + 8 > a1 ? (uint32_t)(a1 - gs) : 8u;  // 0 .. 8
            uint32_t ph = (uint32_t)(gs - o) * lo_rate;
            uint32_t pi[8], pq[8], si = 0, sq = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t w = x[k >> 1] >> (16 * (k & 1));
                const bool keep = (uint32_t)k >= b_lo && (uint32_t)k < b_hi;
                const int vi = keep ? (int)(int8_t)(w & 0xffu) - dc_i : 0, vq = keep ? (int)(int8_t)((w >> 8) & 0xffu) - dc_q : 0;
                const bool cneg = ((ph >> 31) ^ (ph >> 30)) & 1u, sneg = (~ph >> 31) & 1u;  // the carrier bits of THE CHANNEL MODEL
                const int vic = cneg ? -vi : vi, vqc = cneg ? -vq : vq, vis = sneg ? -vi : vi, vqs = sneg ? -vq : vq;
                si += (uint32_t)(vic - vqs);  // v_i C - v_q S
                sq += (uint32_t)(vis + vqc);  // v_i S + v_q C
                pi[k] = si, pq[k] = sq;
                if (with_floor) fl += (uint32_t)(vi * vi + vq * vq);
                ph += lo_rate;
            }
            // the lanes' totals, summed up over the wave
            uint32_t ti = si, tq = sq;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const uint32_t ui = (uint32_t)__shfl_up((int)ti, m, 64), uq = (uint32_t)__shfl_up((int)tq, m, 64);
                if (lane >= m) ti += ui, tq += uq;
            }
            const uint32_t bi = ci + ti - si, bq = cq + tq - sq;  // A before the lane's group
            if (mine) {
                int2* dst = A + G::PAD + 8 * gl + 1;
#pragma unroll
                for (int k = 0; k < 8; ++k) dst[k] = make_int2((int)(bi + pi[k]), (int)(bq + pq[k]));
            }
            ci += (uint32_t)__shfl((int)ti, 63, 64), cq += (uint32_t)__shfl((int)tq, 63, 64);
        }
        for (int i = lane + 1; i < 2 * W; i += 64) A[G::PAD + n + i] = make_int2((int)ci, (int)cq);  // A[k] = A[n] for k > n
        // STREAM: the chip of position m is that of window sample (cs - o) + m at h = 0
        int count = 0;
        uint32_t chip_M = 0;
        uint64_t before = 0;
        const uint64_t q0 = cs - o;
        for (int m0 = 0; m0 <= M; m0 += 64) {
            const uint64_t P = mod_full(((uint64_t)base + q0 + (uint64_t)(m0 + lane)) * ca_rate);  // below 2^23 * 2^32
            const uint32_t cb = (uint32_t)(P >> 32);                                                // 0 .. 1022
            const uint32_t chip = (s_chips[cb >> 5] >> (cb & 31)) & 1u;
            const uint64_t bits = __ballot(chip != 0);
            const uint64_t prev = m0 == 0 ? bits & 1ull : before >> 63;
            const int left = M - m0;  // the positions of this round are 0 .. min(left, 63)
            const uint64_t valid = left >= 63 ? ~0ull : (2ull << left) - 1ull;
            const uint64_t trans = (bits ^ (bits << 1 | prev)) & valid;
            if (trans >> lane & 1ull) list[count + __popcll(trans & ((1ull << lane) - 1ull))] = (uint16_t)((uint32_t)(m0 + lane) | chip << 15);
            count += __popcll(trans);
            if (left <= 63) chip_M = (uint32_t)(bits >> left) & 1u;
            before = bits;
        }
        if (lane < 3 && count + lane < ((count + 3) & ~3)) list[count + lane] = 0;  // up to a multiple of four: entries that read A[-h] = 0
        const int quads = (count + 3) >> 2;
        wave_sync();
        // SUM
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            if (64 * p < n_code) {  // the lanes beyond n_code read slots that exist and are not used
                const int2* const Ah = A + G::PAD - (lane + 64 * p);
                uint32_t sx = 0, sy = 0;
                for (int i = 0; i < quads; ++i) {
                    const uint2 e = lq[i];
                    const uint32_t ent[4] = {e.x & 0xffffu, e.x >> 16, e.y & 0xffffu, e.y >> 16};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int2 v = Ah[ent[k] & 0x7fffu];
                        const uint32_t msk = (ent[k] >> 15) - 1u;  // the new chip 1 (s' falls, D = -2): + A; 0 (D = +2): - A
                        sx += ((uint32_t)v.x ^ msk) - msk;
                        sy += ((uint32_t)v.y ^ msk) - msk;
                    }
                }
                const uint32_t sM = chip_M ? ~0u : 0u;  // s'[M] A[n]
                Ri[p] += ((ci ^ sM) - sM) + 2u * sx;
                Rq[p] += ((cq ^ sM) - sM) + 2u * sy;
            }
        }
        wave_sync();
    }
}

}  // namespace acq
