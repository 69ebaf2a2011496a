// aided_iq_kernels.hip -- "Aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, multi-bit mode: the windowed search of
// "Aided acquisition" B on the IQ bytes themselves, both arms and every amplitude bit.
//
// k_aided_iq: one workgroup of AIDED_IQ_WAVES wave64 per task.  The PRN's chips go into LDS as in k_refine_iq; wave w takes the
// segments w, w + 4, ... of the window.  The 2 W + 1 code hypotheses of one (segment, d) share one carrier-wiped series
// a_j = (v_i C - v_q S, v_i S + v_q C) and one chip stream s'[m] = +-1: hypothesis h wants sum_j s'[j + h] a_j.  Summed by parts
// over a chunk of n samples that is
//     R(h) = s'[M] A[n] - sum over m in [1, M] of D[m] A[m - h],      M = n + 2 W - 1,
// with A[k] the inclusive prefix sums of a (A[k] = 0 for k <= 0, A[k] = A[n] for k >= n) and D[m] = s'[m] - s'[m - 1], which is 0
// except at the chip TRANSITIONS of the stream (0.19 per sample at 5.456 MHz).  Exact, in integers.  The walk itself is
// aided_iq_walk.hpp's segment_sums_by_parts, which k_aided_coh_iq shares, here at four passes on AidedIqGeometry.  Per (segment, d)
// and chunk of AIDED_IQ_CHUNK samples (counted from the 8-sample group the segment starts in; samples of the chunk before or after the
// segment count as a = 0):
//   WIPE.  Lane l takes the 16-byte groups l, l + 64 of the chunk (iq_groups.hpp: load_group and the flip word): per sample the
//     mean is taken off, the carrier signs come from ph = j lo_rate, the eight a's are summed up inside the lane, a wave scan
//     (shuffles) of the lanes' totals plus the total carried from the groups before gives A[1 .. n], int2, into the wave's LDS;
//     2 W copies of A[n] go behind.  The slots in front are zero from the kernel's start.
//   STREAM.  The lanes evaluate the chip of stream position m = 0 .. M, 64 at a time; a ballot gives the chips as one mask, the
//     mask xor itself shifted by one position (the last chip of the 64 before carried in) the transitions, and a popcount below the
//     lane the transition's place in the wave's list: 15 bits of m and the new chip, in order.  The list is filled up to a
//     multiple of four with entries that read a zero.
//   SUM.  Lane h (h + 64, ... in further passes over the same list) walks the list: one 8-byte broadcast read brings four
//     entries, per entry one ds_read_b64 of A[m - h] -- neighbouring lanes read neighbouring int2 -- added or subtracted in
//     wrap-around uint32; R(h) of the chunk adds into the lane's (I, Q) of the segment.
// At the segment's end the lane squares its own I and Q into its own uint64.  The floor's sum v_i^2 + v_q^2 is taken in WIPE at
// the first valid d alone.  Once per d the four waves' sums meet in LDS (the waves' own prefix arrays serve: two barriers); thread h
// adds them, writes power(h, d) and keeps its total and the largest (power, 31 - d, 255 - h): a power may take 62 bits here, so
// the key is a pair.  Steps 1 and 2 and the record and peak are aided_prologue and aided_record of snapshot_records.hpp, k_aided's:
// this file unpacks its tag and brings the measured floor.
// No atomics, no float before the ratio.  Every loop is bounded by kernel arguments; the prefix array is
// read at slot AIDED_IQ_PAD + m - h with m in [0, n + 2 W - 1] and h in [0, 255] (the lanes beyond 2 W read and are not used), so in
// [1, AIDED_IQ_SLOTS - 3], written in [0, AIDED_IQ_PAD + n + 2 W - 1], and the list is indexed below n + 2 W + 2 <= AIDED_IQ_LIST
// (W <= 127 and n <= 1024 are the host's check and the chunk); nothing at or beyond byte 2 * n_samples is read (load_group).
// Static LDS: s_chips 136 + s_a 49152 + s_list 10240 + s_red 128 = 59656 bytes (59664 with alignment in the compiler's report), below k_aided_coh's 61224: two workgroups per CU.
// Built with -ffp-contract=off (Makefile): the NCO words must be the host's to the bit, as in refine_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aided_iq_launch.hpp"
#include "aided_iq_walk.hpp"
#include "snapshot_records.hpp"

namespace acq {

__global__ __launch_bounds__(64 * AIDED_IQ_WAVES) void k_aided_iq(AidedIqArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ int2 s_a[AIDED_IQ_WAVES][AIDED_IQ_SLOTS];         // slot AIDED_IQ_PAD + k holds A[k]
    __shared__ uint2 s_list[AIDED_IQ_WAVES][AIDED_IQ_LIST / 4];  // four 16-bit entries per uint2
    __shared__ unsigned long long s_red[AIDED_IQ_WAVES][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const int W = a.p.code_half, K = a.p.dop_half, n_code = 2 * W + 1, n_dop = 2 * K + 1;
    unsigned long long* const powers = a.powers ? a.powers + t * (size_t)(n_dop * n_code) : nullptr;

    // 1. kept, 2. no aid: the flag and zeros (snapshot_records.hpp)
    const gpsacq_aid aid = a.aid[t];
    gpsacq_peak pk_out;
    Window win;
    int d_first;  // the first valid d: the floor is summed there
    if (!aided_prologue(a, t, aid, powers, n_dop * n_code, pk_out, win, d_first)) return;
    chips_to_lds(a.c.chips, win.prn, s_chips);
    int2* const A = s_a[wv];
    for (int i = lane; i <= AIDED_IQ_PAD; i += 64) A[i] = make_int2(0, 0);  // A[k] = 0 for k <= 0: never written again
    __syncthreads();

    // 3. hypotheses, 4. sums
    const uint64_t o = win.o, spm = (uint64_t)a.c.spm, segments = win.segments;  // o is a multiple of 8: stride is one of 16
    const uint32_t base = aided_base(aid, W, a.c.spm);
    uint64_t total = 0, best = 0, floor_sum = 0;  // of hypothesis h = threadIdx.x; floor_sum of the lane's samples
    uint32_t tag = 0;
    for (int d = 0; d < n_dop; ++d) {
        const Window wd = window_at(a, t, (int64_t)aid.lo_center - K + d);
        if (!wd.hit) {  // every lane decides the same
            if (powers && (int)threadIdx.x < n_code) powers[d * n_code + threadIdx.x] = 0;
            continue;
        }
        const uint32_t lo_rate = wd.lo_rate, ca_rate = wd.ca_rate;
        const bool with_floor = d == d_first;
        uint64_t acc[AIDED_PASSES] = {0, 0, 0, 0};
        for (uint64_t s = wv; s < segments; s += AIDED_IQ_WAVES) {
            const uint64_t a0 = o + s * spm, a1 = a0 + spm;  // the segment's samples [a0, a1) of the capture
            uint32_t Ri[AIDED_PASSES], Rq[AIDED_PASSES], fl;
            segment_sums_by_parts<AIDED_PASSES, AidedIqGeometry>(a.c, a0, a1, o, base, lo_rate, ca_rate, s_chips, A, s_list[wv], lane, W, n_code, with_floor, Ri,
                                                                 Rq, fl);
#pragma unroll
            for (int p = 0; p < AIDED_PASSES; ++p) {
                const int64_t I = (int32_t)Ri[p], Q = (int32_t)Rq[p];
                acc[p] += (uint64_t)(I * I + Q * Q);
            }
            floor_sum += fl;
        }
        // the waves' sums meet in their prefix arrays: slot h of wave w holds its acc of hypothesis h
#pragma unroll
        for (int p = 0; p < AIDED_PASSES; ++p) A[AIDED_IQ_PAD + 1 + lane + 64 * p] = make_int2((int)(uint32_t)acc[p], (int)(uint32_t)(acc[p] >> 32));
        __syncthreads();
        if ((int)threadIdx.x < n_code) {
            uint64_t pw = 0;
            for (int w = 0; w < AIDED_IQ_WAVES; ++w) {
                const int2 v = s_a[w][AIDED_IQ_PAD + 1 + threadIdx.x];
                pw += (uint64_t)(uint32_t)v.y << 32 | (uint32_t)v.x;
            }
            if (powers) powers[d * n_code + threadIdx.x] = pw;
            total += pw;
            key_max(best, tag, pw, (uint32_t)(31 - d) << 8 | (uint32_t)(255 - threadIdx.x) | 1u << 16);
        }
        __syncthreads();
    }

    // 5. record, 6. peak: the largest pair, the total and the floor over the workgroup, then snapshot_records.hpp
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t opw = shfl_xor64(best, m);
        const uint32_t otag = (uint32_t)__shfl_xor((int)tag, m, 64);
        key_max(best, tag, opw, otag);
        total += shfl_xor64(total, m);
        floor_sum += shfl_xor64(floor_sum, m);
    }
    if (lane == 0) s_red[wv][0] = best, s_red[wv][1] = tag, s_red[wv][2] = total, s_red[wv][3] = floor_sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    best = total = floor_sum = 0, tag = 0;
    for (int w = 0; w < AIDED_IQ_WAVES; ++w) {
        key_max(best, tag, s_red[w][0], (uint32_t)s_red[w][1]);
        total += s_red[w][2];
        floor_sum += s_red[w][3];
    }
    // the tag unpacked; the measured floor
    aided_record(a, t, aid, base, segments, win.fit, best, 255 - (int32_t)(tag & 255), 31 - (int32_t)(tag >> 8 & 31), total, 2 * floor_sum, pk_out);
}

void launch_aided_iq(const AidedIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_aided_iq, dim3((unsigned)a.c.n_tasks), dim3(64 * AIDED_IQ_WAVES), 0, s, a);
}

}  // namespace acq
