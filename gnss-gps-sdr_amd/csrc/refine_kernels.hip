// refine_kernels.hip -- "Fine code phases: search peaks refined below a sample" of include/gpsacq.h.
//
// k_refine: one workgroup of REFINE_WAVES wave64 per task.  The PRN's chips go into LDS; wave w takes the segments (one
// nominal code period of spm samples each) w, w + 4, ... of the task's window.  Within a segment lane l takes the 32-sample words
// l, l + 64, ... of the capture: per word it builds five 32-bit masks (cos, -sin, early, prompt, late chips) one sample at a time
// from the two NCOs and takes six popcounts against the sample word, as BitsCorr of track_kernels.hip does.  What differs from it:
//   * the code position wraps inside a segment (the window starts at the hit's code phase, not at chip 0): a modulo per word
//     finds the late position L0 of the word's bit 0, and from there on the word counts chips RELATIVE to b = L0 >> 32.  The 32
//     samples of a word advance by less than 28 chips (REFINE_MAX_CA_RATE, checked by the host), early is at most one chip ahead
//     of late's start plus that, so all 96 chips of a word lie in the 32 chips from b on: ONE 32-bit window, cut by a funnel
//     shift out of two words of the chip sequence written twice over in LDS (so that b + 31 needs no wrap), and every chip is a
//     bit of that register -- two LDS reads per word instead of three per sample, and no 64-bit compare in the sample loop;
//   * the early / late spacing is the parameter D, not half a chip;
//   * a block starts at any byte of the capture, so the words are addressed from the capture's 4-byte-aligned base and a mask
//     keeps the bits before and after the segment out of the counts;
//   * the last bytes of the capture are read bytewise, nothing at or beyond byte n_bytes.
// The six counts of ones pack in pairs (a segment has spm <= 65535 samples) and are summed over the wave with xor shuffles; every
// lane then adds the three squares I^2 + Q^2 into 64-bit partials, the four waves' partials meet in LDS and thread 0 writes the
// record, which fine_record of snapshot_records.hpp builds from the three sums for this kernel and for k_refine_iq.  Integer
// sums, no atomics: the record does not depend on the order of anything.  Two barriers; every loop is bounded by kernel arguments.  The word loop's pieces (word_at, mod_full, the chips in LDS, the per-word window and masks) live in
// capture_words.hpp, which k_fine_dop of doppler_kernels.hip shares.
// k_coarse_obs_fine: one lane per (fix, channel), k_coarse_obs of coarse_kernels.hip with the code phase of a usable record.
// Built with -ffp-contract=off (Makefile): the NCO words must be gpsacq_handoff_engine's to the bit, and `lo_shift * step + fc`
// or `lo_dop / L1 * CPS + CPS` fused into an FMA round differently from the host's two operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture_words.hpp"
#include "nav_launch.hpp"
#include "refine_launch.hpp"
#include "snapshot_records.hpp"

namespace acq {

__global__ __launch_bounds__(64 * REFINE_WAVES) void k_refine(RefineArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ unsigned long long s_part[REFINE_WAVES][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const gpsacq_peak pk = a.c.peaks[t];

    // 1. the NCO words of gpsacq_handoff_engine, 2. what is no hit, 3. window and segments
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
    for (uint64_t s = wv; s < segments; s += REFINE_WAVES) {
        const uint64_t a0 = o + s * spm, a1 = a0 + spm;  // the segment's samples [a0, a1), counted from the aligned base
        const uint64_t w1 = (a1 - 1) >> 5;
        uint32_t ones[6] = {0, 0, 0, 0, 0, 0};  // IE QE IP QP IL QL: samples whose product is -1
        for (uint64_t wi = (a0 >> 5) + lane; wi <= w1; wi += 64) {
            const WordPos w = word_pos(a.c.words, a.c.n_bytes, wi, a0, a1, o, P0, D, lo_rate, ca_rate, s_chips);
            const uint32_t x = w.x, valid = w.valid;
            uint32_t cm, sp, em, pm, lm;
            word_masks<true>(w, D, lo_rate, ca_rate, cm, sp, em, pm, lm);
            const uint32_t sm = ~sp;
            ones[0] += __popc((x ^ em ^ cm) & valid);
            ones[1] += __popc((x ^ em ^ sm) & valid);
            ones[2] += __popc((x ^ pm ^ cm) & valid);
            ones[3] += __popc((x ^ pm ^ sm) & valid);
            ones[4] += __popc((x ^ lm ^ cm) & valid);
            ones[5] += __popc((x ^ lm ^ sm) & valid);
        }
        uint32_t pkd[3] = {ones[0] | ones[1] << 16, ones[2] | ones[3] << 16, ones[4] | ones[5] << 16};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < 3; ++q) pkd[q] += (uint32_t)__shfl_xor((int)pkd[q], m, 64);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t I = (int64_t)a.c.spm - 2 * (int64_t)(pkd[q] & 0xFFFF), Q = (int64_t)a.c.spm - 2 * (int64_t)(pkd[q] >> 16);
            acc[q] += (uint64_t)(I * I + Q * Q);
        }
    }
    if (lane == 0)
        for (int q = 0; q < 3; ++q) s_part[wv][q] = acc[q];
    __syncthreads();
    if (threadIdx.x != 0) return;

    // 5. estimate, 6. usable: snapshot_records.hpp
    uint64_t early = 0, prompt = 0, late = 0;
    for (int w = 0; w < REFINE_WAVES; ++w) early += s_part[w][0], prompt += s_part[w][1], late += s_part[w][2];
    a.out[t] = fine_record(segments, win.fit, a.p.min_segments, lo_rate, ca_rate, D, P0, early, prompt, late);
}

__global__ __launch_bounds__(NAV_BLOCK) void k_coarse_obs_fine(CoarseObsFineArgs a) {
    const size_t i = (size_t)blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_peak pk = a.peaks[i];
    const gpsacq_fine f = a.fine[i];
    gpsacq_obs o = {0, 0, 0, 0, 0.0, 0.0};
    if ((double)pk.snr >= a.snr_min && pk.ca_shift >= 0 && (double)pk.ca_shift < a.fs / 1000.0 && !(f.flags & FINE_UNUSABLE) && f.tx_frac >= 0.0 &&
        f.tx_frac < 1e-3) {
        o.eph = (int32_t)(i % (size_t)a.chans);
        o.valid = 1;
        o.tx_frac = f.tx_frac;
        o.weight = 1.0;
    }
    a.out[i] = o;
}

void launch_refine(const RefineArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_refine, dim3((unsigned)a.c.n_tasks), dim3(64 * REFINE_WAVES), 0, s, a);
}

void launch_coarse_obs_fine(const CoarseObsFineArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_obs_fine, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
