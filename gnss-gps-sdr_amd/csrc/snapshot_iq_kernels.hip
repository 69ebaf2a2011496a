// snapshot_iq_kernels.hip -- "Snapshot chain on an 8-bit IQ capture" of include/gpsacq.h, multi-bit mode: the fine code phase and the
// fine Doppler of a search peak from the capture at full amplitude, both arms.
//
// k_refine_iq: one workgroup of SNAP_IQ_WAVES wave64 per task, k_refine's plan on bytes.  The PRN's chips go into LDS twice over;
// wave w takes the segments w, w + 4, ... of the task's window; within a segment lane l takes the 16-byte groups (8 samples)
// l, l + 64, ... of the capture (capture_groups.hpp: segment_sums): per group one 16-byte load, the chips of its 24 replica samples
// as bits of ONE 32-chip window cut out of LDS by a funnel shift, and 24 dot products (v_dot4_i32_i8) of a dword of two samples
// against weight bytes +1 / -1 / 0 -- 0 for a sample before or after the segment, so a block may start at any sample and the
// capture may end anywhere.  The six int32 sums of a segment meet over the wave through xor shuffles; every lane adds the three
// squares I^2 + Q^2 (|I|, |Q| <= 512 spm < 2^25) into 64-bit partials, the four waves' partials meet in LDS and thread 0 writes the
// record (fine_record of snapshot_records.hpp, k_refine's).  Integer sums, no atomics, no float before the estimate: the record does not depend on the order of anything.  Two
// barriers; every loop is bounded by kernel arguments.
// k_fine_dop_iq: the same loop with the prompt replica alone (8 dot products per group); every segment's (I, Q) goes into LDS as
// k_fine_dop's do.  The 25-bit sums are then normalised exactly: thread i takes the largest |I_s|, |Q_s| of the segments i, i + 256,
// ..., an integer max over the wave and over LDS gives M in every thread, k = max(0, bitlength(M) - 12), and the lag-1 sums are
// formed from I' = (I + 2^(k-1)) >> k, |I'| <= 2^12: a term is at most 2^50 and fewer than 2^12 of them stay below 2^62.  power is
// the sum of the unshifted squares; the record is dopfine_record's (snapshot_records.hpp), k_fine_dop's.  Four barriers.
// Built with -ffp-contract=off (Makefile): the NCO words must be the host's to the bit, as in refine_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture_groups.hpp"
#include "snapshot_iq_launch.hpp"
#include "snapshot_records.hpp"

namespace acq {

__global__ __launch_bounds__(64 * SNAP_IQ_WAVES) void k_refine_iq(RefineIqArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ unsigned long long s_part[SNAP_IQ_WAVES][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const gpsacq_peak pk = a.c.peaks[t];

    // 1. the NCO words, 2. what is no hit, 3. window and segments
    double base_hz;
    const Window win = window_of(pk, a.c, t, a.p.snr_min, a.p.blocks, base_hz);
    const uint64_t o = win.o, spm = (uint64_t)a.c.spm, segments = win.segments;
    const uint32_t lo_rate = win.lo_rate, ca_rate = win.ca_rate;
    if (!win.hit) {
        if (threadIdx.x == 0) a.out[t] = gpsacq_fine{GPSACQ_FINE_NO_HIT, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
        return;
    }
    chips_to_lds(a.c.chips, win.prn, s_chips);
    __syncthreads();

    // 4. sums
    const uint32_t D = (uint32_t)(a.p.half_spacing_chips * 4294967296.0);
    const uint64_t P0 = (uint64_t)pk.ca_shift * ca_rate % FULL;
    uint64_t acc[3] = {0, 0, 0};  // early, prompt, late: the same in every lane of the wave
    for (uint64_t s = wv; s < segments; s += SNAP_IQ_WAVES) {
        const uint64_t a0 = o + s * spm;  // the segment's samples [a0, a0 + spm) of the capture
        int32_t sums[6];                  // IE QE IP QP IL QL
        segment_sums<3>(a.c, a0, a0 + spm, o, P0, D, lo_rate, ca_rate, s_chips, lane, sums);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t I = sums[2 * q], Q = sums[2 * q + 1];
            acc[q] += (uint64_t)(I * I + Q * Q);
        }
    }
    if (lane == 0)
        for (int q = 0; q < 3; ++q) s_part[wv][q] = acc[q];
    __syncthreads();
    if (threadIdx.x != 0) return;

    // 5. estimate, 6. usable: snapshot_records.hpp
    uint64_t early = 0, prompt = 0, late = 0;
    for (int w = 0; w < SNAP_IQ_WAVES; ++w) early += s_part[w][0], prompt += s_part[w][1], late += s_part[w][2];
    a.out[t] = fine_record(segments, win.fit, a.p.min_segments, lo_rate, ca_rate, D, P0, early, prompt, late);
}

__global__ __launch_bounds__(64 * SNAP_IQ_WAVES) void k_fine_dop_iq(FineDopIqArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ int32_t s_iq[DOP_MAX_SEGMENTS][2];
    __shared__ uint32_t s_max[SNAP_IQ_WAVES];
    __shared__ unsigned long long s_part[SNAP_IQ_WAVES][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const gpsacq_peak pk = a.c.peaks[t];

    // steps 1 to 3
    double base_hz;
    const Window win = window_of(pk, a.c, t, a.p.snr_min, a.p.blocks, base_hz);
    const uint64_t o = win.o, spm = (uint64_t)a.c.spm, segments = win.segments;  // segments <= DOP_MAX_SEGMENTS: the host's check
    const uint32_t lo_rate = win.lo_rate, ca_rate = win.ca_rate;
    if (!win.hit) {
        if (threadIdx.x == 0) a.out[t] = gpsacq_dopfine{GPSACQ_DOPFINE_NO_HIT, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0};
        return;
    }
    chips_to_lds(a.c.chips, win.prn, s_chips);
    __syncthreads();

    // prompt sums
    const uint64_t P0 = (uint64_t)pk.ca_shift * ca_rate % FULL;
    for (uint64_t s = wv; s < segments; s += SNAP_IQ_WAVES) {
        const uint64_t a0 = o + s * spm;
        int32_t sums[2];
        segment_sums<1>(a.c, a0, a0 + spm, o, P0, 0u, lo_rate, ca_rate, s_chips, lane, sums);
        if (lane == 0) s_iq[s][0] = sums[0], s_iq[s][1] = sums[1];
    }
    __syncthreads();

    // the normalisation: M, the largest |I_s| or |Q_s|, in every thread
    uint32_t m = 0;
    for (uint64_t s = threadIdx.x; s < segments; s += 64 * SNAP_IQ_WAVES) {
        const int32_t I = s_iq[s][0], Q = s_iq[s][1];
        const uint32_t ai = (uint32_t)(I < 0 ? -I : I), aq = (uint32_t)(Q < 0 ? -Q : Q);
        m = max(m, max(ai, aq));
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, x, 64));
    if (lane == 0) s_max[wv] = m;
    __syncthreads();
    for (int w = 0; w < SNAP_IQ_WAVES; ++w) m = max(m, s_max[w]);
    const int bitlen = 32 - __clz((int)m);  // 0 for m = 0; m < 2^25
    const int k = bitlen > 12 ? bitlen - 12 : 0;
    const int32_t half = k > 0 ? 1 << (k - 1) : 0;

    // squares and lag-1 sums of the shifted values, modulo 2^64 (nothing wraps: the bound is in the head comment); power unshifted
    uint64_t re = 0, im = 0, mag = 0, power = 0;
    for (uint64_t s = threadIdx.x; s < segments; s += 64 * SNAP_IQ_WAVES) {
        const int64_t I0 = s_iq[s][0], Q0 = s_iq[s][1];
        power += (uint64_t)(I0 * I0 + Q0 * Q0);
        if (s >= 1) {
            const int64_t I = (s_iq[s][0] + half) >> k, Q = (s_iq[s][1] + half) >> k;
            const int64_t I1 = (s_iq[s - 1][0] + half) >> k, Q1 = (s_iq[s - 1][1] + half) >> k;
            const uint64_t A = (uint64_t)(I * I - Q * Q), B = (uint64_t)(2 * I * Q);
            const uint64_t A1 = (uint64_t)(I1 * I1 - Q1 * Q1), B1 = (uint64_t)(2 * I1 * Q1);
            re += A * A1 + B * B1;
            im += B * A1 - A * B1;
            mag += (uint64_t)(I * I + Q * Q) * (uint64_t)(I1 * I1 + Q1 * Q1);
        }
    }
    re = wave_sum(re), im = wave_sum(im), mag = wave_sum(mag), power = wave_sum(power);
    if (lane == 0) s_part[wv][0] = re, s_part[wv][1] = im, s_part[wv][2] = mag, s_part[wv][3] = power;
    __syncthreads();
    if (threadIdx.x != 0) return;

    // estimate, flags: snapshot_records.hpp.  lo_rate is read SIGNED: complex baseband
    re = im = mag = power = 0;
    for (int w = 0; w < SNAP_IQ_WAVES; ++w) re += s_part[w][0], im += s_part[w][1], mag += s_part[w][2], power += s_part[w][3];
    const double nco_hz = ((double)(int32_t)lo_rate * a.c.fs) / 4294967296.0;
    a.out[t] = dopfine_record(segments, win.fit, a.p, lo_rate, ca_rate, re, im, mag, power, nco_hz, base_hz, (double)a.c.spm / a.c.fs);
}

void launch_refine_iq(const RefineIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_refine_iq, dim3((unsigned)a.c.n_tasks), dim3(64 * SNAP_IQ_WAVES), 0, s, a);
}

void launch_fine_dop_iq(const FineDopIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fine_dop_iq, dim3((unsigned)a.c.n_tasks), dim3(64 * SNAP_IQ_WAVES), 0, s, a);
}

}  // namespace acq
