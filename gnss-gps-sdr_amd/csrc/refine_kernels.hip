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
// record.  Integer sums, no atomics: the record does not depend on the order of anything.  Two barriers; every loop is bounded by
// kernel arguments.
// k_coarse_obs_fine: one lane per (fix, channel), k_coarse_obs of coarse_kernels.hip with the code phase of a usable record.
// Built with -ffp-contract=off (Makefile): the NCO words must be gpsacq_handoff_engine's to the bit, and `lo_shift * step + fc`
// or `lo_dop / L1 * CPS + CPS` fused into an FMA round differently from the host's two operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nav_launch.hpp"
#include "refine_launch.hpp"

namespace acq {

namespace {
constexpr uint64_t FULL = 1023ull << 32;  // one code period, chips * 2^32
constexpr int FINE_UNUSABLE = GPSACQ_FINE_NO_HIT | GPSACQ_FINE_NO_POWER | GPSACQ_FINE_FEW;

// 32 samples from byte 4 wi of the aligned capture; the capture's last bytes one at a time, nothing at or beyond n_bytes
__device__ __forceinline__ uint32_t word_at(const uint32_t* words, size_t n_bytes, uint64_t wi) {
    const size_t off = (size_t)wi * 4;
    if (off + 4 <= n_bytes) return words[wi];
    const uint8_t* b = reinterpret_cast<const uint8_t*>(words);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (off + k < n_bytes) v |= (uint32_t)b[off + k] << (8 * k);
    return v;
}

// x mod 1023 * 2^32 for x < 2^64: the low word stays, the high word is reduced mod 1023
__device__ __forceinline__ uint64_t mod_full(uint64_t x) { return (uint64_t)((uint32_t)(x >> 32) % 1023u) << 32 | (uint32_t)x; }

constexpr int CHIP_WORDS = 34;  // the chip sequence twice over, bits 0 .. 1087: a window starts at bit b <= 1022 and ends at b + 31
}  // namespace

__global__ __launch_bounds__(64 * REFINE_WAVES) void k_refine(RefineArgs a) {
    __shared__ uint32_t s_chips[CHIP_WORDS];
    __shared__ unsigned long long s_part[REFINE_WAVES][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t t = blockIdx.x;
    const gpsacq_peak pk = a.peaks[t];
    int32_t block = (int32_t)t, prn = (int32_t)(t % 32);
    if (a.tasks) block = a.tasks[t].block, prn = a.tasks[t].prn;

    // 1. the NCO words of gpsacq_handoff_engine, 2. what is no hit.  Every lane of the workgroup decides the same.
    const double L1 = 1575.42e6, CPS = 1.023e6;
    const double lo_dop = a.step_hz > 0 ? pk.lo_shift * a.step_hz : pk.lo_shift * a.fs / 40000.0;
    const double ca_dop = lo_dop / L1 * CPS;
    const double lo_f = a.fc + lo_dop, ca_f = CPS + ca_dop;
    bool hit = (double)pk.snr >= a.p.snr_min && pk.ca_shift >= 0 && pk.ca_shift < a.spm && block >= 0 && prn >= 0 && prn < GPSACQ_NUM_SATS &&
               lo_f >= 0 && lo_f < a.fs && ca_f >= 0 && ca_f < a.fs;
    const uint64_t total = (uint64_t)a.n_bytes * 8;  // samples from the aligned base, the `lead` bytes in front included
    uint64_t o = 0;
    uint32_t lo_rate = 0, ca_rate = 0;
    if (hit) {
        o = 8ull * a.lead + 8ull * (uint64_t)block * a.stride;  // stride <= 2^31: no overflow
        lo_rate = (uint32_t)(lo_f / a.fs * 4294967296.0);
        ca_rate = (uint32_t)(ca_f / a.fs * 4294967296.0);
        hit = o < total && ca_rate != 0;
    }
    if (!hit) {
        if (threadIdx.x == 0) a.out[t] = gpsacq_fine{GPSACQ_FINE_NO_HIT, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
        return;
    }
    if (threadIdx.x < CHIP_WORDS) {  // bit i of word k: chip (32 k + i) mod 1023
        const uint32_t* c = a.chips + prn * 32;
        uint32_t w = 0;
        for (uint32_t i = 0; i < 32; ++i) {
            const uint32_t q = (32u * threadIdx.x + i) % 1023u;
            w |= ((c[q >> 5] >> (q & 31)) & 1u) << i;
        }
        s_chips[threadIdx.x] = w;
    }
    __syncthreads();

    // 3. window and segments
    const uint64_t spm = (uint64_t)a.spm;
    const uint64_t fit = (uint64_t)a.p.blocks * 40000ull / spm, have = (total - o) / spm;
    const uint64_t segments = have < fit ? have : fit;

    // 4. sums
    const uint32_t D = (uint32_t)(a.p.half_spacing_chips * 4294967296.0);
    const uint64_t P0 = (uint64_t)pk.ca_shift * ca_rate % FULL;
    uint64_t acc[3] = {0, 0, 0};  // early, prompt, late: the same in every lane of the wave
    for (uint64_t s = wv; s < segments; s += REFINE_WAVES) {
        const uint64_t a0 = o + s * spm, a1 = a0 + spm;  // the segment's samples [a0, a1), counted from the aligned base
        const uint64_t w1 = (a1 - 1) >> 5;
        uint32_t ones[6] = {0, 0, 0, 0, 0, 0};  // IE QE IP QP IL QL: samples whose product is -1
        for (uint64_t wi = (a0 >> 5) + lane; wi <= w1; wi += 64) {
            const uint32_t x = word_at(a.words, a.n_bytes, wi);
            const uint64_t ws = wi << 5;
            const uint32_t b_lo = ws < a0 ? (uint32_t)(a0 - ws) : 0u;        // 0 .. 31
            const uint32_t b_hi = ws + 32 > a1 ? (uint32_t)(a1 - ws) : 32u;  // 1 .. 32
            const uint32_t valid = (b_hi == 32 ? ~0u : (1u << b_hi) - 1u) & ~((1u << b_lo) - 1u);
            // the prompt position of the word's first sample of the segment (window sample j >= 0, j ca_rate < 2^54), carried back
            // to bit 0 of the word modulo the period: bits below b_lo are masked out, the ones from b_lo on get their own position
            uint64_t P = mod_full(P0 + (ws + b_lo - o) * ca_rate);
            const uint64_t back = (uint64_t)b_lo * ca_rate;  // < 2^37 < FULL
            P = P >= back ? P - back : P + FULL - back;
            uint32_t ph = (uint32_t)(ws - o) * lo_rate;  // modulo 2^32 also where the word starts before the window
            // the window of 32 chips from late's chip at bit 0, and the prompt position relative to it: rel - D >= 0 and
            // rel + D + 31 ca_rate < 32 * 2^32, so every chip index below is the high word of a sum that does not wrap
            const uint64_t L0 = P >= D ? P - D : P + FULL - D;
            const uint32_t cb = (uint32_t)(L0 >> 32);  // 0 .. 1022
            const uint32_t win = __funnelshift_r(s_chips[cb >> 5], s_chips[(cb >> 5) + 1], cb & 31);
            uint64_t rel = (uint64_t)(uint32_t)L0 + D;
            uint32_t cm = 0, sp = 0, em = 0, pm = 0, lm = 0;  // sp: the samples where -sin is POSITIVE (bit 31 of the phase)
#pragma unroll
            for (int b = 0; b < 32; ++b) {
                cm |= ((ph + 0x40000000u) >> 31) << b;  // bit31 ^ bit30
                sp |= (ph >> 31) << b;
                em |= ((win >> (uint32_t)((rel + D) >> 32)) & 1u) << b;
                pm |= ((win >> (uint32_t)(rel >> 32)) & 1u) << b;
                lm |= ((win >> (uint32_t)((rel - D) >> 32)) & 1u) << b;
                ph += lo_rate;
                rel += ca_rate;
            }
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
            const int64_t I = (int64_t)a.spm - 2 * (int64_t)(pkd[q] & 0xFFFF), Q = (int64_t)a.spm - 2 * (int64_t)(pkd[q] >> 16);
            acc[q] += (uint64_t)(I * I + Q * Q);
        }
    }
    if (lane == 0)
        for (int q = 0; q < 3; ++q) s_part[wv][q] = acc[q];
    __syncthreads();
    if (threadIdx.x != 0) return;

    // 5. estimate, 6. usable
    gpsacq_fine r = {0, (int32_t)segments, lo_rate, ca_rate, 0, 0, 0, 0.0, 0.0};
    for (int w = 0; w < REFINE_WAVES; ++w) r.early += s_part[w][0], r.prompt += s_part[w][1], r.late += s_part[w][2];
    if (segments < fit) r.flags |= GPSACQ_FINE_SHORT;
    if (segments < (uint64_t)a.p.min_segments) r.flags |= GPSACQ_FINE_FEW;
    if (r.early + r.late == 0) {
        r.flags |= GPSACQ_FINE_NO_POWER;
    } else {
        const double d = (double)D / 4294967296.0, aE = sqrt((double)r.early), aL = sqrt((double)r.late);
        r.offset_chips = (1.0 - d) * (aE - aL) / (aE + aL);
        double pos = (double)P0 / 4294967296.0 + r.offset_chips;
        if (pos < 0.0) pos += 1023.0;
        else if (pos >= 1023.0) pos -= 1023.0;
        r.tx_frac = pos / 1.023e6;
        if (!(r.tx_frac < 1e-3)) r.tx_frac = 0.0;
    }
    a.out[t] = r;
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
    hipLaunchKernelGGL(k_refine, dim3((unsigned)a.n_tasks), dim3(64 * REFINE_WAVES), 0, s, a);
}

void launch_coarse_obs_fine(const CoarseObsFineArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_coarse_obs_fine, dim3((unsigned)((a.n_obs + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, s, a);
}

}  // namespace acq
