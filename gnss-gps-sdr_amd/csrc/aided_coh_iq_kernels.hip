// aided_coh_iq_kernels.hip -- "Coherent aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, multi-bit mode: the 20 ms
// coherent search of "Coherent aided acquisition" on the segment sums of "Aided acquisition on an 8-bit IQ capture", both arms and
// every amplitude bit.
//
// k_aided_coh_iq<M>: one workgroup of AIDED_COH_IQ_WAVES wave64 per task, two stages per Doppler hypothesis d.
//   CORRELATION.  k_aided_iq's WIPE / STREAM / SUM by summation by parts at one pass (2 W + 1 <= 63 hypotheses, lane h owns h):
//     aided_iq_walk.hpp's segment_sums_by_parts<1, AidedCohIqGeometry>, the walk both kernels call.  Wave w takes the segments
//     w, w + 4, ...; the stage is entered ONCE per (segment, d), never per g or e.  Instead of squaring, lane h stores (I, Q) as an
//     int32 pair into s_z[s * n_code + h].  The floor's sum v_i^2 + v_q^2 rides along at the first valid d.
//   COHERENT.  After a barrier the work item is (h, g), item g * n_code + h on thread item % 256: neighbouring lanes read
//     neighbouring 8-byte entries of a z row, lanes of equal h and different g the same entry (a broadcast).  One walk over the
//     segments: the table entry (C | S << 16, one LDS word) at k, k += f u mod 1024; the turned sums go into the prefix (PA, PB);
//     segment s closes the period of edge e = s mod M alone, as the prefix minus the prefix kept at that edge's last boundary.
//     The walk is unrolled by M from a multiple of M, so e is the unrolled index and the three arrays of M live in registers.
//     The last, partial period of every e closes after the walk.  This is k_aided_coh's walk with other integer types: |z| <= 2^9
//     spm < 2^25, so a product with the int16 table is a 64-bit product, a prefix stays below 2^52, A' below 2^30 and a power
//     below 2^60 (the header's BOUNDS) -- past the 44 bits of k_aided_coh's packed key, so the key is the PAIR (power, tag) with
//     tag = 31 - d << 15 | 15 - g << 11 | 31 - e << 6 | 63 - h, compared lexicographically, as in k_aided_iq.  That kernel's walk
//     is not shared through a header: its key and its products would have to become template parameters of its own source.
//   Per d the largest pair of the workgroup is found (shuffles, one LDS step) and every thread keeps the running best and the
//   non-coherent sum of its (h, d), which item (h, g = 0) left in s_nc.  Steps 1 and 2 and the record and peak are aided_prologue
//   and aided_coh_record of snapshot_records.hpp, k_aided_coh's: this file unpacks its tag and brings the measured floor.
//   No atomics, no scratch, no float before the ratio.
// Every loop is bounded by kernel arguments.  The prefix array is read at slot PAD + m - h with m in [0, n + 2 W - 1] and h in
// [0, 63], so in [1, AIDED_COH_IQ_SLOTS - 3], written in [0, PAD + n + 2 W - 1]; the list is indexed below n + 2 W + 2 <=
// AIDED_COH_IQ_LIST (W <= 31 is the host's check, n <= 512 the chunk); s_z is indexed below segments * n_code <= fit * (2 W + 1)
// <= COH_MAX_Z (checked by the host), s_tab below 1024 (masked), s_nc below 64; nothing at or beyond byte 2 * n_samples of the
// capture is read (load_group).
// Static LDS: s_chips 136 + s_a 20480 + s_list 4608 + s_z 40960 + s_tab 4096 + s_nc 512 + s_red 64 = 70856 bytes (70864 with alignment in
// the compiler's report): two workgroups per CU.
// Built with -ffp-contract=off (Makefile): the NCO words must be the host's to the bit, as in refine_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aided_coh_iq_launch.hpp"
#include "aided_iq_walk.hpp"
#include "snapshot_records.hpp"

namespace acq {

template <int M> __global__ __launch_bounds__(64 * AIDED_COH_IQ_WAVES) void k_aided_coh_iq(AidedCohIqArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ int2 s_a[AIDED_COH_IQ_WAVES][AIDED_COH_IQ_SLOTS];         // slot PAD + k holds A[k]
    __shared__ uint2 s_list[AIDED_COH_IQ_WAVES][AIDED_COH_IQ_LIST / 4];  // four 16-bit entries per uint2
    __shared__ int2 s_z[COH_MAX_Z];
    __shared__ uint32_t s_tab[COH_TABLE];  // C[k] in the low half, S[k] in the high half
    __shared__ unsigned long long s_nc[64];
    __shared__ unsigned long long s_red[AIDED_COH_IQ_WAVES][2];
    constexpr int PAD = AidedCohIqGeometry::PAD;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const int W = a.p.code_half, K = a.p.dop_half, F = a.p.fine_half, n_code = 2 * W + 1, n_dop = 2 * K + 1, n_fine = 2 * F + 1;
    const int row = n_fine * M * n_code;  // powers of one d
    unsigned long long* const powers = a.powers ? a.powers + t * (size_t)(n_dop * row) : nullptr;

    // 1. kept, 2. no aid: the flag and zeros (snapshot_records.hpp)
    const gpsacq_aid aid = a.aid[t];
    gpsacq_peak pk_out;
    Window win;
    int d_first;  // the first valid d: the floor is summed there
    if (!aided_prologue(a, t, aid, powers, n_dop * row, pk_out, win, d_first)) return;
    chips_to_lds(a.c.chips, win.prn, s_chips);
    for (int i = threadIdx.x; i < COH_TABLE; i += 64 * AIDED_COH_IQ_WAVES)
        s_tab[i] = (uint32_t)(uint16_t)a.table[i] | (uint32_t)(uint16_t)a.table[COH_TABLE + i] << 16;
    int2* const A = s_a[wv];
    for (int i = lane; i <= PAD; i += 64) A[i] = make_int2(0, 0);  // A[k] = 0 for k <= 0: never written again
    __syncthreads();

    const uint64_t o = win.o, spm = (uint64_t)a.c.spm;  // o is a multiple of 8: stride is one of 16
    const int S = (int)win.segments;                    // S * n_code <= COH_MAX_Z
    const uint32_t base = aided_base(aid, W, a.c.spm);
    const int items = n_code * n_fine;
    uint64_t best = 0, best_nc = 0, floor_sum = 0;  // best, best_nc and tag the same in every thread; floor_sum of the lane's samples
    uint32_t tag = 0;
    for (int d = 0; d < n_dop; ++d) {
        const Window wd = window_at(a, t, (int64_t)aid.lo_center - K + d);
        if (!wd.hit) {  // every lane decides the same
            if (powers)
                for (int i = threadIdx.x; i < row; i += 64 * AIDED_COH_IQ_WAVES) powers[d * row + i] = 0;
            continue;
        }
        // 4. segment sums
        const bool with_floor = d == d_first;
        for (int s = wv; s < S; s += AIDED_COH_IQ_WAVES) {
            const uint64_t a0 = o + (uint64_t)s * spm;
            uint32_t Ri[1], Rq[1], fl;
            segment_sums_by_parts<1, AidedCohIqGeometry>(a.c, a0, a0 + spm, o, base, wd.lo_rate, wd.ca_rate, s_chips, A, s_list[wv], lane, W, n_code, with_floor,
                                                         Ri, Rq, fl);
            if (lane < n_code) s_z[s * n_code + lane] = make_int2((int)Ri[0], (int)Rq[0]);
            floor_sum += fl;
        }
        __syncthreads();
        // 5. coherent sums
        uint64_t kpw = 0;
        uint32_t ktag = 0;
        for (int it = threadIdx.x; it < items; it += 64 * AIDED_COH_IQ_WAVES) {
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
                        const int64_t c = (int16_t)(cs & 0xffffu), sn = (int16_t)(cs >> 16), zi = z.x, zq = z.y;
                        PA += zi * c + zq * sn;
                        PB += zq * c - zi * sn;
                        nc += sq2(zi, zq);
                        k = (k + step) & (COH_TABLE - 1);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const uint64_t pw = acc[j] + sq2((PA - LA[j]) >> 14, (PB - LB[j]) >> 14);
                if (powers) powers[d * row + (g * M + j) * n_code + h] = pw;
                key_max(kpw, ktag, pw, (uint32_t)(31 - d) << 15 | (uint32_t)(15 - g) << 11 | (uint32_t)(31 - j) << 6 | (uint32_t)(63 - h));
            }
            if (g == 0) s_nc[h] = nc;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t opw = shfl_xor64(kpw, m);
            const uint32_t otag = (uint32_t)__shfl_xor((int)ktag, m, 64);
            key_max(kpw, ktag, opw, otag);
        }
        if (lane == 0) s_red[wv][0] = kpw, s_red[wv][1] = ktag;
        __syncthreads();  // also: every thread is done with s_z before the next d writes it
        for (int w = 0; w < AIDED_COH_IQ_WAVES; ++w) key_max(kpw, ktag, s_red[w][0], (uint32_t)s_red[w][1]);
        if (kpw > best || (kpw == best && ktag > tag)) best = kpw, tag = ktag, best_nc = s_nc[63 - (int)(ktag & 63)];
        // s_red and s_nc are written again only behind the next d's first barrier
    }

    // 6. record and peak: the floor's sum over the workgroup first; the barrier in front lets every thread finish reading s_red
    floor_sum = wave_sum(floor_sum);
    __syncthreads();
    if (lane == 0) s_red[wv][0] = floor_sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    floor_sum = 0;
    for (int w = 0; w < AIDED_COH_IQ_WAVES; ++w) floor_sum += s_red[w][0];
    // the tag unpacked and the measured floor, then snapshot_records.hpp
    aided_coh_record(a, t, aid, base, (uint64_t)S, win.fit, M, best, 63 - (int32_t)(tag & 63), 31 - (int32_t)(tag >> 15 & 31), 15 - (int32_t)(tag >> 11 & 15),
                     31 - (int32_t)(tag >> 6 & 31), best_nc, 2 * floor_sum, pk_out);
}

void launch_aided_coh_iq(const AidedCohIqArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.c.n_tasks), block(64 * AIDED_COH_IQ_WAVES);
    switch (a.p.coh_ms) {  // the host has checked that it is one of these
        case 1: hipLaunchKernelGGL(k_aided_coh_iq<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_aided_coh_iq<2>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_aided_coh_iq<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_aided_coh_iq<5>, grid, block, 0, s, a); break;
        case 10: hipLaunchKernelGGL(k_aided_coh_iq<10>, grid, block, 0, s, a); break;
        case 20: hipLaunchKernelGGL(k_aided_coh_iq<20>, grid, block, 0, s, a); break;
    }
}

}  // namespace acq
