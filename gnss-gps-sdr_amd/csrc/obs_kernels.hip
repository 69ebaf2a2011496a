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
//
// "Carrier observables" of the same header: k_carrier_acc is k_code_pos turned round -- a forward prefix sum A_{t+1} = A_t + n_t d_t
// of the Doppler part of the carrier NCO word, the same chunks of 64 x OBS_RUN epochs, the scan with __shfl_up, the carry running
// forward.  n_t d_t is a full 64 x 64 -> 64-bit product (a few v_mad_u64_u32 / v_mul_lo_u32; four per lane and pass, next to
// eight 40-byte-strided loads it does not show).  k_observe_rate: one lane per (instant, channel), three bisections (R_a, R,
// R_b); the Doppler is one fp64 product and one fp64 quotient in separate statements, nothing for the compiler to contract.
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

__global__ __launch_bounds__(OBS_BLOCK) void k_carrier_acc(CarrierAccArgs a) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    const RateChan ch = a.chan[c];
    const int n = ch.n;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    int64_t* acc = a.acc + (size_t)c * ((size_t)a.max_epochs + 1);
    constexpr int CHUNK = OBS_BLOCK * OBS_RUN;
    if (lane == 0) acc[0] = 0;
    uint64_t carry = 0;  // A at the first epoch of the chunk, mod 2^64
    for (int base = 0; base < n; base += CHUNK) {
        const int t0 = base + lane * OBS_RUN;
        uint64_t smp[OBS_RUN + 1];
#pragma unroll
        for (int j = 0; j <= OBS_RUN; ++j) smp[j] = t0 + j < n ? rec[t0 + j].sample : ch.next_sample;
        // inclusive prefix sums inside this lane's run
        uint64_t pre[OBS_RUN];
        uint64_t run = 0;
#pragma unroll
        for (int j = 0; j < OBS_RUN; ++j) {
            if (t0 + j < n) {
                const uint64_t d = (uint64_t)(int64_t)(int32_t)(rec[t0 + j].lo_rate - ch.nom_word);
                run += (smp[j + 1] - smp[j]) * d;
            }
            pre[j] = run;
        }
        // inclusive prefix scan of the run totals over the wave
        uint64_t incl = run;
#pragma unroll
        for (int off = 1; off < OBS_BLOCK; off <<= 1) {
            const uint64_t v = __shfl_up((unsigned long long)incl, off, OBS_BLOCK);
            if (lane >= off) incl += v;
        }
        const uint64_t left = carry + (incl - run);  // everything before this lane's run
#pragma unroll
        for (int j = 0; j < OBS_RUN; ++j)
            if (t0 + j < n) acc[t0 + j + 1] = (int64_t)(left + pre[j]);
        carry += __shfl((unsigned long long)incl, OBS_BLOCK - 1, OBS_BLOCK);
    }
}

namespace {
// A(X) of the model for rec[0].sample <= X < next_sample: the last record whose sample is <= X, then the interpolation
__device__ __forceinline__ uint64_t acc_at(const gpsacq_track_record* rec, const int64_t* acc, int n, uint32_t nom_word, uint64_t X) {
    int lo = 0, hi = n;
    for (int k = 0; k < 32 && hi - lo > 1; ++k) {
        const int mid = lo + (hi - lo) / 2;
        if (rec[mid].sample <= X) lo = mid;
        else hi = mid;
    }
    const uint64_t d = (uint64_t)(int64_t)(int32_t)(rec[lo].lo_rate - nom_word);
    return (uint64_t)acc[lo] + (X - rec[lo].sample) * d;
}
}  // namespace

__global__ __launch_bounds__(OBS_BLOCK) void k_observe_rate(ObserveRateArgs a) {
    const size_t i = (size_t)blockIdx.x * OBS_BLOCK + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= a.n_fix) return;
    const RateChan ch = a.chan[c];
    const uint64_t R = a.first_rx_sample + (uint64_t)i * a.rx_step;
    const uint64_t W = a.avg_samples, half = W / 2;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    const int64_t* acc = a.acc + (size_t)c * ((size_t)a.max_epochs + 1);
    gpsacq_rate_obs o;
    o.valid = o.reserved = 0;
    o.adr = 0;
    o.doppler_hz = o.weight = 0.0;
    // R_a <= R <= R_b: R_a at or past record 0 and R_b before next_sample put all three inside the records
    if (ch.n > 0 && R >= half && R - half >= rec[0].sample && R - half < ch.next_sample && W < ch.next_sample - (R - half)) {
        const uint64_t Ra = R - half, Rb = Ra + W;
        const int64_t D = (int64_t)(acc_at(rec, acc, ch.n, ch.nom_word, Rb) - acc_at(rec, acc, ch.n, ch.nom_word, Ra));
        const double num = __dmul_rn((double)D, a.fs);
        const double den = __dmul_rn((double)W, 4294967296.0);
        o.valid = 1;
        o.adr = (int64_t)acc_at(rec, acc, ch.n, ch.nom_word, R);
        o.doppler_hz = __ddiv_rn(num, den);
        o.weight = 1.0;
    }
    a.out[i * (size_t)a.n_chans + c] = o;
}

void launch_carrier_acc(const CarrierAccArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_carrier_acc, dim3((unsigned)n_chans), dim3(OBS_BLOCK), 0, s, a);
}

void launch_observe_rate(const ObserveRateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_observe_rate, dim3((unsigned)((a.n_fix + OBS_BLOCK - 1) / OBS_BLOCK), (unsigned)a.n_chans), dim3(OBS_BLOCK), 0, s, a);
}

void launch_code_pos(const CodePosArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_code_pos, dim3((unsigned)n_chans), dim3(OBS_BLOCK), 0, s, a);
}

void launch_observe(const ObserveArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_observe, dim3((unsigned)((a.n_fix + OBS_BLOCK - 1) / OBS_BLOCK), (unsigned)a.n_chans), dim3(OBS_BLOCK), 0, s, a);
}

}  // namespace acq
