// obs_kernels.hip -- the observables of include/gpsacq.h ("Observables"): the uncorrected transmit time of every tracked satellite
// at a batch of receive instants, from the records of the tracking channels.  Integers up to the one fp64 division of tx_frac.
//
// k_code_pos: one wave64 per channel.  pos_t = ca_pos + sum over u >= t of ((1023 << 32) - n_u ca_rate_u), mod 2^64, is a suffix
// sum over up to ~10^5 epochs: the wave walks the row from its end in chunks of 64 x OBS_RUN epochs -- each lane sums its own run
// of OBS_RUN consecutive epochs, one shuffle scan adds the runs to its right, a 64-bit carry holds everything past the chunk -- so
// an 81 800-epoch row is 320 passes of six shuffle steps, not 81 800 dependent steps; the loads of a pass do not depend on the
// carry, so they overlap the scan of the pass before.  k_observe: one lane per (instant, channel); the epoch that holds the
// instant is found by bisection over the records' `sample` fields (at most 31 steps, the lanes of a wave are neighbouring instants
// of one channel and walk the same path).  No LDS, no barrier, no atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "obs_launch.hpp"

namespace acq {

namespace {
constexpr uint64_t CODE_PERIOD = (uint64_t)1023 << 32;      // one code period of the prompt position, chips * 2^32
constexpr double MS_PER_POS = 4393751543808000.0;           // 1023 * 2^32 * 1000: position units per second
constexpr int64_t OBS_WEEK_MS = 604800000;
}  // namespace

__global__ __launch_bounds__(OBS_BLOCK) void k_code_pos(CodePosArgs a) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    const ObsChan ch = a.chan[c];
    const int n = ch.n;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    uint64_t* pos = a.pos + (size_t)c * (size_t)a.max_epochs;
    constexpr int CHUNK = OBS_BLOCK * OBS_RUN;
    uint64_t carry = ch.ca_pos;  // pos at the first epoch past the chunk
    for (int base = (n - 1) / CHUNK * CHUNK; base >= 0 && n > 0; base -= CHUNK) {
        const int t0 = base + lane * OBS_RUN;
        // this lane's run: the samples that bound its epochs, then the suffix sums inside the run
        uint64_t smp[OBS_RUN + 1];
#pragma unroll
        for (int j = 0; j <= OBS_RUN; ++j) smp[j] = t0 + j < n ? rec[t0 + j].sample : ch.next_sample;
        uint64_t suf[OBS_RUN];
        uint64_t run = 0;
#pragma unroll
        for (int j = OBS_RUN - 1; j >= 0; --j) {
            if (t0 + j < n) run += CODE_PERIOD - (smp[j + 1] - smp[j]) * (uint64_t)rec[t0 + j].ca_rate;
            suf[j] = run;
        }
        // inclusive suffix scan of the run totals over the wave
        uint64_t incl = run;
#pragma unroll
        for (int off = 1; off < OBS_BLOCK; off <<= 1) {
            const uint64_t v = __shfl_down((unsigned long long)incl, off, OBS_BLOCK);
            if (lane + off < OBS_BLOCK) incl += v;
        }
        const uint64_t right = carry + (incl - run);  // everything past this lane's run
#pragma unroll
        for (int j = 0; j < OBS_RUN; ++j)
            if (t0 + j < n) pos[t0 + j] = right + suf[j];
        carry += __shfl((unsigned long long)incl, 0, OBS_BLOCK);
    }
}

__global__ __launch_bounds__(OBS_BLOCK) void k_observe(ObserveArgs a) {
    const size_t i = (size_t)blockIdx.x * OBS_BLOCK + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= a.n_fix) return;
    const ObsChan ch = a.chan[c];
    const uint64_t R = a.first_rx_sample + (uint64_t)i * a.rx_step;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    gpsacq_obs o;
    o.eph = o.valid = o.tx_ms = o.reserved = 0;
    o.tx_frac = o.weight = 0.0;
    if (ch.tag_valid != 0 && ch.n > 0 && R < ch.next_sample && R >= rec[0].sample) {
        // the last record whose sample is <= R: rec[lo].sample <= R < rec[hi].sample (hi == n: next_sample)
        int lo = 0, hi = ch.n;
        for (int k = 0; k < 32 && hi - lo > 1; ++k) {
            const int mid = lo + (hi - lo) / 2;
            if (rec[mid].sample <= R) lo = mid;
            else hi = mid;
        }
        const uint64_t P = a.pos[(size_t)c * (size_t)a.max_epochs + lo] + (R - rec[lo].sample) * (uint64_t)rec[lo].ca_rate;
        int64_t ms = ((int64_t)ch.tag_ms + ((int64_t)ch.first_epoch + lo - (int64_t)ch.tag_epoch)) % OBS_WEEK_MS;
        if (ms < 0) ms += OBS_WEEK_MS;
        o.eph = ch.tag_eph;
        o.valid = 1;
        o.tx_ms = (int32_t)ms;
        o.tx_frac = (double)P / MS_PER_POS;
        o.weight = 1.0;
    }
    a.out[i * (size_t)a.n_chans + c] = o;
}

void launch_code_pos(const CodePosArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_code_pos, dim3((unsigned)n_chans), dim3(OBS_BLOCK), 0, s, a);
}

void launch_observe(const ObserveArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_observe, dim3((unsigned)((a.n_fix + OBS_BLOCK - 1) / OBS_BLOCK), (unsigned)a.n_chans), dim3(OBS_BLOCK), 0, s, a);
}

}  // namespace acq
