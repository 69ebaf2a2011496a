// capture_words.hpp -- the word loop of the kernels that go back to the 1-bit capture at a search peak, once: refine_kernels.hip
// (k_refine), doppler_kernels.hip (k_fine_dop) and aided_kernels.hip (k_aided, at a predicted peak) include it; capture_groups.hpp, the
// 8-bit IQ counterpart, builds on its chip sequence in LDS, mod_full, Window and code_window.  A segment of the window is walked in the 32-sample
// words of the capture's 4-byte-aligned base; window_of() is steps 1 to 3 of the text (NCO words, no hit, segments); per word word_pos() reads the samples (the capture's last bytes one at a time, nothing
// at or beyond n_bytes), masks the bits before and after the segment, carries the code position back to the word's bit 0 and cuts
// the ONE 32-chip window that holds every chip of the word out of the chip sequence in LDS; word_masks() then builds the carrier
// and chip masks one sample at a time from the two NCOs.  k_refine's head comment has the reasoning; "Fine code phases" of
// include/gpsacq.h, steps 3 and 4, is the text.  The capture comes as the BitCaptureArgs of refine_launch.hpp; what lanes of a wave
// do with each other (wave_sync, shfl_xor64, wave_sum) is wave_ops.hpp's, and what follows the sums snapshot_records.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "refine_launch.hpp"
#include "wave_ops.hpp"

namespace acq {

constexpr uint64_t FULL = 1023ull << 32;  // one code period, chips * 2^32
constexpr int CHIP_WORDS = 34;  // the chip sequence twice over, bits 0 .. 1087: a window starts at bit b <= 1022 and ends at b + 31

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

// the chips of PRN index prn (chips: [32][32] chip words) twice over into s_chips[CHIP_WORDS]: bit i of word k is chip
// (32 k + i) mod 1023.  The first CHIP_WORDS threads of the workgroup write; the caller's barrier follows
__device__ __forceinline__ void chips_to_lds(const uint32_t* chips, int prn, uint32_t* s_chips) {
    if (threadIdx.x < CHIP_WORDS) {
        const uint32_t* c = chips + prn * 32;
        uint32_t w = 0;
        for (uint32_t i = 0; i < 32; ++i) {
            const uint32_t q = (32u * threadIdx.x + i) % 1023u;
            w |= ((c[q >> 5] >> (q & 31)) & 1u) << i;
        }
        s_chips[threadIdx.x] = w;
    }
}

// steps 1 to 3 of "Fine code phases", PER TASK: the NCO words of gpsacq_handoff_engine, what is no hit, the window's segments.
// Every lane of the workgroup decides the same
struct Window {
    bool hit;
    int32_t prn;
    uint32_t lo_rate, ca_rate;
    uint64_t o, total;       // the window's first sample and the samples that may be read, both from the aligned base
    uint64_t fit, segments;  // the segments of a whole window, and of this one
};

// step 1's Dopplers of a peak on the engine's grid: lo_dop, and ca_f = 1.023e6 + ca_dop, every operation rounded by itself
__device__ __forceinline__ void peak_dopplers(const gpsacq_peak& pk, double fs, double step_hz, double& lo_dop, double& ca_f) {
#pragma clang fp contract(off)  // the NCO words are the host's to the bit
    const double L1 = 1575.42e6, CPS = 1.023e6;
    lo_dop = step_hz > 0 ? pk.lo_shift * step_hz : pk.lo_shift * fs / 40000.0;
    const double ca_dop = lo_dop / L1 * CPS;
    ca_f = CPS + ca_dop;
}

// step 3 of a hit whose o, total and ca_rate are set: the start inside the capture, the segments of a whole window and of this one
__device__ __forceinline__ void window_segments(Window& w, int spm, int blocks) {
    w.hit = w.o < w.total && w.ca_rate != 0;
    if (!w.hit) return;
    const uint64_t have = (w.total - w.o) / (uint64_t)spm;
    w.fit = (uint64_t)blocks * 40000ull / (uint64_t)spm;
    w.segments = have < w.fit ? have : w.fit;
}

// base_hz is what the fine Doppler takes off the replica's frequency: c.fc here.  capture_groups.hpp has the overload for an
// IqCaptureArgs
__device__ __forceinline__ Window window_of(const gpsacq_peak& pk, const BitCaptureArgs& c, size_t t, double snr_min, int blocks, double& base_hz) {
#pragma clang fp contract(off)  // the NCO words are the host's to the bit
    Window w = {false, (int32_t)(t % 32), 0, 0, 0, (uint64_t)c.n_bytes * 8, 0, 0};
    int32_t block = (int32_t)t;
    if (c.tasks) block = c.tasks[t].block, w.prn = c.tasks[t].prn;
    double lo_dop, ca_f;
    peak_dopplers(pk, c.fs, c.step_hz, lo_dop, ca_f);
    const double lo_f = c.fc + lo_dop;
    base_hz = c.fc;
    w.hit = (double)pk.snr >= snr_min && pk.ca_shift >= 0 && pk.ca_shift < c.spm && block >= 0 && w.prn >= 0 && w.prn < GPSACQ_NUM_SATS && lo_f >= 0 &&
            lo_f < c.fs && ca_f >= 0 && ca_f < c.fs;
    if (!w.hit) return w;
    w.o = 8ull * c.lead + 8ull * (uint64_t)block * c.stride;  // stride <= 2^31: no overflow
    w.lo_rate = (uint32_t)(lo_f / c.fs * 4294967296.0);
    w.ca_rate = (uint32_t)(ca_f / c.fs * 4294967296.0);
    window_segments(w, c.spm, blocks);
    return w;
}

// the code side of one unit of a segment (a 32-sample word here, a 16-byte group of capture_groups.hpp): the ONE 32-chip window that
// holds every chip of the unit, and the prompt position of the unit's sample 0 relative to it
struct CodeWindow {
    uint32_t win;  // 32 chips from late's chip at sample 0
    uint64_t rel;  // the prompt position of sample 0 relative to the window's first chip, chips * 2^32
};

// j: the window sample index of the unit's first sample that belongs to the segment (j >= 0, j ca_rate < 2^54), which is the
// unit's sample b_lo; P0: the prompt position of window sample 0; D: early's and late's distance from prompt (0: prompt only)
__device__ __forceinline__ CodeWindow code_window(uint64_t j, uint32_t b_lo, uint64_t P0, uint32_t D, uint32_t ca_rate, const uint32_t* s_chips) {
    // the prompt position of sample b_lo, carried back to sample 0 of the unit modulo the period: samples below b_lo are masked
    // out, the ones from b_lo on get their own position
    uint64_t P = mod_full(P0 + j * ca_rate);
    const uint64_t back = (uint64_t)b_lo * ca_rate;  // < 2^37 < FULL
    P = P >= back ? P - back : P + FULL - back;
    // the window of 32 chips from late's chip at sample 0, and the prompt position relative to it: rel - D >= 0 and
    // rel + D + 31 ca_rate < 32 * 2^32, so every chip index is the high word of a sum that does not wrap
    const uint64_t L0 = P >= D ? P - D : P + FULL - D;
    const uint32_t cb = (uint32_t)(L0 >> 32);  // 0 .. 1022
    CodeWindow c;
    c.win = __funnelshift_r(s_chips[cb >> 5], s_chips[(cb >> 5) + 1], cb & 31);
    c.rel = (uint64_t)(uint32_t)L0 + D;
    return c;
}

// one word of a segment
struct WordPos {
    uint32_t x;      // the 32 samples
    uint32_t valid;  // the bits that belong to the segment
    uint32_t ph;     // carrier phase of bit 0
    uint32_t win;    // 32 chips from late's chip at bit 0
    uint64_t rel;    // the prompt position of bit 0 relative to the window's first chip, chips * 2^32
};

// word wi of the segment [a0, a1) (samples counted from the aligned base) of a window that starts at sample o with the prompt
// position P0; D: early's and late's distance from prompt (0: prompt only)
__device__ __forceinline__ WordPos word_pos(const uint32_t* words, size_t n_bytes, uint64_t wi, uint64_t a0, uint64_t a1, uint64_t o, uint64_t P0,
                                            uint32_t D, uint32_t lo_rate, uint32_t ca_rate, const uint32_t* s_chips) {
    WordPos w;
    w.x = word_at(words, n_bytes, wi);
    const uint64_t ws = wi << 5;
    const uint32_t b_lo = ws < a0 ? (uint32_t)(a0 - ws) : 0u;        // 0 .. 31
    const uint32_t b_hi = ws + 32 > a1 ? (uint32_t)(a1 - ws) : 32u;  // 1 .. 32
    w.valid = (b_hi == 32 ? ~0u : (1u << b_hi) - 1u) & ~((1u << b_lo) - 1u);
    w.ph = (uint32_t)(ws - o) * lo_rate;  // modulo 2^32 also where the word starts before the window
    const CodeWindow c = code_window(ws + b_lo - o, b_lo, P0, D, ca_rate, s_chips);
    w.win = c.win;
    w.rel = c.rel;
    return w;
}

// the masks of a word, one sample at a time: cm the cos bits, sp the samples where -sin is POSITIVE (bit 31 of the phase), pm the
// prompt chips and, with ELP, em and lm the early and late chips
template <bool ELP>
__device__ __forceinline__ void word_masks(const WordPos& w, uint32_t D, uint32_t lo_rate, uint32_t ca_rate, uint32_t& cm, uint32_t& sp, uint32_t& em,
                                           uint32_t& pm, uint32_t& lm) {
    uint32_t ph = w.ph;
    uint64_t rel = w.rel;
    cm = sp = em = pm = lm = 0;
    // every mask is a chain of funnel shifts: the new sample's bit comes in at bit 31 and the older ones move down, so after 32
    // samples sample b sits at bit b.  (A chain, not 32 independent bits or-ed together: those the compiler is free to collect at
    // the end of the word, 160 live registers.)
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        cm = __funnelshift_r(cm, (ph + 0x40000000u) >> 31, 1);  // bit31 ^ bit30
        sp = __funnelshift_r(sp, ph >> 31, 1);
        if (ELP) em = __funnelshift_r(em, w.win >> (uint32_t)((rel + D) >> 32), 1);
        pm = __funnelshift_r(pm, w.win >> (uint32_t)(rel >> 32), 1);
        if (ELP) lm = __funnelshift_r(lm, w.win >> (uint32_t)((rel - D) >> 32), 1);
        ph += lo_rate;
        rel += ca_rate;
    }
}

}  // namespace acq
