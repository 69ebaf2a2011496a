// smooth_kernels.hip -- "Carrier-smoothed observables" of include/gpsacq.h: code-minus-carrier per instant, a phase-lock test, slip
// resets and a box-window Hatch filter, from the records of the tracking channels.  Integers up to the one fp64 division of tx_frac.
//
// k_lock_acc: one wave64 per channel, k_carrier_acc's idiom (obs_kernels.hip): forward prefix sums of ip^2 - qp^2 and ip^2 + qp^2
// over the epochs, chunks of 64 x SMOOTH_RUN epochs, runs per lane, one __shfl_up scan per sum, a 64-bit carry each.  k_cmc: one
// lane per (instant, channel); ONE bisection gives t, and from it P (k_code_pos's pos), A(R) (k_carrier_acc's acc), Z, and the lock
// test as two differences of the lock sums.  k_smooth_scan: one wave64 per channel over the instants, the same chunks: the prefix
// sum S of Z mod 2^64 and a max-scan of the segment starts (the start flag of instant i needs only instant i-1's Z and state, so
// the loads of a pass do not depend on the carry).  k_smooth_out: one lane per (instant, channel): the window sum as a difference
// of two S, two signed floor divisions, the shifted position folded into its code period, the two records.
// No LDS, no barrier, no atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smooth_launch.hpp"

namespace acq {

namespace {
constexpr uint64_t SM_FULL = (uint64_t)1023 << 32;      // one code period of the prompt position, chips * 2^32
constexpr double SM_MS_PER_POS = 4393751543808000.0;    // 1023 * 2^32 * 1000: position units per second
constexpr int64_t SM_WEEK_MS = 604800000;
constexpr int64_t SM_AID_RATIO = 1540;                  // carrier cycles per chip

// signed division rounded toward minus infinity, b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
}  // namespace

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_lock_acc(LockAccArgs a) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = a.chan[c].n;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    int64_t* out_n = a.lock_n + (size_t)c * ((size_t)a.max_epochs + 1);
    int64_t* out_d = a.lock_d + (size_t)c * ((size_t)a.max_epochs + 1);
    constexpr int CHUNK = SMOOTH_BLOCK * SMOOTH_RUN;
    if (lane == 0) out_n[0] = 0, out_d[0] = 0;
    uint64_t carry_n = 0, carry_d = 0;  // the sums at the first epoch of the chunk, mod 2^64
    for (int base = 0; base < n; base += CHUNK) {
        const int t0 = base + lane * SMOOTH_RUN;
        // inclusive prefix sums inside this lane's run
        uint64_t pre_n[SMOOTH_RUN], pre_d[SMOOTH_RUN];
        uint64_t run_n = 0, run_d = 0;
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j) {
            if (t0 + j < n) {
                const int64_t ip = rec[t0 + j].ip, qp = rec[t0 + j].qp;
                const uint64_t i2 = (uint64_t)(ip * ip), q2 = (uint64_t)(qp * qp);
                run_n += i2 - q2;
                run_d += i2 + q2;
            }
            pre_n[j] = run_n, pre_d[j] = run_d;
        }
        // inclusive prefix scans of the run totals over the wave
        uint64_t incl_n = run_n, incl_d = run_d;
#pragma unroll
        for (int off = 1; off < SMOOTH_BLOCK; off <<= 1) {
            const uint64_t vn = __shfl_up((unsigned long long)incl_n, off, SMOOTH_BLOCK);
            const uint64_t vd = __shfl_up((unsigned long long)incl_d, off, SMOOTH_BLOCK);
            if (lane >= off) incl_n += vn, incl_d += vd;
        }
        const uint64_t left_n = carry_n + (incl_n - run_n), left_d = carry_d + (incl_d - run_d);  // everything before this lane's run
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j)
            if (t0 + j < n) {
                out_n[t0 + j + 1] = (int64_t)(left_n + pre_n[j]);
                out_d[t0 + j + 1] = (int64_t)(left_d + pre_d[j]);
            }
        carry_n += __shfl((unsigned long long)incl_n, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
        carry_d += __shfl((unsigned long long)incl_d, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
    }
}

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_cmc(CmcArgs a) {
    const size_t i = (size_t)blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= a.n_fix) return;
    const SmoothChan ch = a.chan[c];
    const uint64_t R = a.first_rx_sample + (uint64_t)i * a.rx_step;
    const gpsacq_track_record* rec = a.records + (size_t)c * (size_t)a.max_epochs;
    uint64_t Z = 0, P = 0;
    int32_t t = 0, state = SMOOTH_INVALID;
    if (ch.tag_valid != 0 && ch.n > 0 && R < ch.next_sample && R >= rec[0].sample) {
        // the last record whose sample is <= R: rec[lo].sample <= R < rec[hi].sample (hi == n: next_sample)
        int lo = 0, hi = ch.n;
        for (int k = 0; k < 32 && hi - lo > 1; ++k) {
            const int mid = lo + (hi - lo) / 2;
            if (rec[mid].sample <= R) lo = mid;
            else hi = mid;
        }
        t = lo;
        const uint64_t dt = R - rec[lo].sample;
        P = a.pos[(size_t)c * (size_t)a.max_epochs + lo] + dt * (uint64_t)rec[lo].ca_rate;
        const uint64_t d = (uint64_t)(int64_t)(int32_t)(rec[lo].lo_rate - ch.nom_word);
        const uint64_t A = (uint64_t)a.acc[(size_t)c * ((size_t)a.max_epochs + 1) + lo] + dt * d;
        const uint64_t ep = (uint64_t)((int64_t)ch.first_epoch + (int64_t)lo);
        const uint64_t code = (uint64_t)SM_AID_RATIO * (ep * SM_FULL + P - (R - rec[0].sample) * (uint64_t)ch.cw);
        state = SMOOTH_LOCKED;
        if (a.lock_epochs > 0) {
            state = SMOOTH_RAW;
            if (lo >= a.lock_epochs - 1) {
                const size_t row = (size_t)c * ((size_t)a.max_epochs + 1);
                const uint64_t N = (uint64_t)a.lock_n[row + lo + 1] - (uint64_t)a.lock_n[row + lo + 1 - a.lock_epochs];
                const uint64_t D = (uint64_t)a.lock_d[row + lo + 1] - (uint64_t)a.lock_d[row + lo + 1 - a.lock_epochs];
                if ((int64_t)D > 0 && (int64_t)(N * (uint64_t)a.lock_den) >= (int64_t)(D * (uint64_t)a.lock_num)) state = SMOOTH_LOCKED;
            }
        }
        if (state == SMOOTH_LOCKED) Z = a.invert ? code + A : code - A;
    }
    const size_t idx = (size_t)c * a.n_fix + i;
    a.z[idx] = Z;
    a.p[idx] = P;
    a.t[idx] = t;
    a.state[idx] = state;
}

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_smooth_scan(SmoothScanArgs a) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t n = (int64_t)a.n_fix;
    const uint64_t* z = a.z + (size_t)c * a.n_fix;
    const int32_t* state = a.state + (size_t)c * a.n_fix;
    uint64_t* sum = a.sum + (size_t)c * (a.n_fix + 1);
    int32_t* seg = a.seg + (size_t)c * a.n_fix;
    constexpr int CHUNK = SMOOTH_BLOCK * SMOOTH_RUN;
    if (lane == 0) sum[0] = 0;
    uint64_t carry = 0;      // S at the first instant of the chunk
    int32_t carry_seg = -1;  // the latest segment start before the chunk
    for (int64_t base = 0; base < n; base += CHUNK) {
        const int64_t i0 = base + (int64_t)lane * SMOOTH_RUN;
        // this lane's run and the instant before it
        uint64_t zz[SMOOTH_RUN + 1];
        int32_t st[SMOOTH_RUN + 1];
#pragma unroll
        for (int j = 0; j <= SMOOTH_RUN; ++j) {
            const int64_t i = i0 + j - 1;
            const bool in = i >= 0 && i < n;
            zz[j] = in ? z[i] : 0;
            st[j] = in ? state[i] : SMOOTH_INVALID;
        }
        // inclusive prefix sums and the running latest start inside the run
        uint64_t pre[SMOOTH_RUN];
        int32_t sg[SMOOTH_RUN];
        uint64_t run = 0;
        int32_t run_seg = -1;
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j) {
            run += zz[j + 1];  // 0 where the instant is not locked or past the end
            const int64_t d = (int64_t)(zz[j + 1] - zz[j]);
            // no short circuit: every operand is in registers already, and the selects keep the unrolled body free of branches
            const bool jumped = (a.jump > 0) & ((d > a.jump) | (d < -a.jump));
            const bool start = (st[j + 1] == SMOOTH_LOCKED) & ((st[j] != SMOOTH_LOCKED) | jumped);
            run_seg = start ? (int32_t)(i0 + j) : run_seg;
            pre[j] = run;
            sg[j] = run_seg;
        }
        // inclusive scans of the run totals over the wave: a sum and a maximum
        uint64_t incl = run;
        int32_t incl_seg = run_seg;
#pragma unroll
        for (int off = 1; off < SMOOTH_BLOCK; off <<= 1) {
            const uint64_t v = __shfl_up((unsigned long long)incl, off, SMOOTH_BLOCK);
            const int32_t w = __shfl_up(incl_seg, off, SMOOTH_BLOCK);
            if (lane >= off) {
                incl += v;
                incl_seg = w > incl_seg ? w : incl_seg;
            }
        }
        const uint64_t left = carry + (incl - run);  // everything before this lane's run
        const int32_t below = __shfl_up(incl_seg, 1, SMOOTH_BLOCK);
        const int32_t left_seg = lane > 0 && below > carry_seg ? below : carry_seg;
#pragma unroll
        for (int j = 0; j < SMOOTH_RUN; ++j)
            if (i0 + j < n) {
                sum[i0 + j + 1] = left + pre[j];
                seg[i0 + j] = sg[j] > left_seg ? sg[j] : left_seg;
            }
        carry += __shfl((unsigned long long)incl, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
        const int32_t last_seg = __shfl(incl_seg, SMOOTH_BLOCK - 1, SMOOTH_BLOCK);
        carry_seg = last_seg > carry_seg ? last_seg : carry_seg;
    }
}

__global__ __launch_bounds__(SMOOTH_BLOCK) void k_smooth_out(SmoothOutArgs a) {
    const size_t i = (size_t)blockIdx.x * SMOOTH_BLOCK + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= a.n_fix) return;
    const SmoothChan ch = a.chan[c];
    const size_t idx = (size_t)c * a.n_fix + i;
    const int32_t state = a.state[idx];
    gpsacq_obs o;
    o.eph = o.valid = o.tx_ms = o.reserved = 0;
    o.tx_frac = o.weight = 0.0;
    gpsacq_smooth_info f;
    f.window = f.flags = 0;
    f.cmc = f.corr = 0;
    if (state != SMOOTH_INVALID) {
        int64_t Ps = (int64_t)a.p[idx];  // < 1023 * 2^32
        int64_t k = 0;
        if (state == SMOOTH_LOCKED) {
            const uint64_t* z = a.z + (size_t)c * a.n_fix;
            const uint64_t* sum = a.sum + (size_t)c * (a.n_fix + 1);
            const int64_t s = a.seg[idx] > 0 ? a.seg[idx] : 0;  // 0 <= s <= i: a locked instant lies in a segment
            const int64_t len = (int64_t)i - s + 1;
            const int32_t m = len < a.window ? (int32_t)len : a.window;
            const int64_t D = (int64_t)((sum[i + 1] - sum[i + 1 - m]) - (uint64_t)m * z[i]);
            const int64_t q = floor_div(D, m);
            Ps += floor_div(q, SM_AID_RATIO);
            k = floor_div(Ps, (int64_t)SM_FULL);
            Ps -= k * (int64_t)SM_FULL;
            f.window = m;
            f.flags = (s == (int64_t)i ? GPSACQ_SMOOTH_RESET : 0) | (m == a.window ? GPSACQ_SMOOTH_FULL : 0);
            f.cmc = (int64_t)(z[i] - z[s]);
            f.corr = q;
        } else {
            f.flags = GPSACQ_SMOOTH_UNLOCKED;
        }
        int64_t ms = ((int64_t)ch.tag_ms + ((int64_t)ch.first_epoch + a.t[idx] + k - (int64_t)ch.tag_epoch)) % SM_WEEK_MS;
        if (ms < 0) ms += SM_WEEK_MS;
        o.eph = ch.tag_eph;
        o.valid = 1;
        o.tx_ms = (int32_t)ms;
        o.tx_frac = (double)Ps / SM_MS_PER_POS;
        o.weight = 1.0;
    }
    a.out[i * (size_t)a.n_chans + c] = o;
    if (a.info) a.info[i * (size_t)a.n_chans + c] = f;
}

void launch_lock_acc(const LockAccArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_lock_acc, dim3((unsigned)n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

void launch_cmc(const CmcArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_cmc, dim3((unsigned)((a.n_fix + SMOOTH_BLOCK - 1) / SMOOTH_BLOCK), (unsigned)a.n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

void launch_smooth_scan(const SmoothScanArgs& a, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(k_smooth_scan, dim3((unsigned)n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

void launch_smooth_out(const SmoothOutArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_smooth_out, dim3((unsigned)((a.n_fix + SMOOTH_BLOCK - 1) / SMOOTH_BLOCK), (unsigned)a.n_chans), dim3(SMOOTH_BLOCK), 0, s, a);
}

}  // namespace acq
