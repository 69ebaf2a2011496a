// track_iq_kernels.hip -- tracking channels on an 8-bit IQ capture kept at full amplitude (include/gpsacq.h, "Tracking channels on
// an 8-bit IQ capture", multi-bit mode), and the generator of such captures.  No reference counterpart: the reference's channels
// are 1-bit ("Homemade GPS Receiver"); its rtl-sdr / HackRF flow (README.md:83-115) quantises to 1 bit before anything runs.
//
// k_track_iq has the shape of track_kernels.hip::k_track -- one wave64 per channel, TRACK_WAVES channels per workgroup, no barrier
// in the epoch loop, every lane running the same integer loop update, lane 0 storing -- and differs in the inner loop: each epoch's
// samples are cut into 16-byte groups of the window (8 samples: I0 Q0 I1 Q1 ...), lane l takes groups l, l + 64, ...  A dword holds
// two samples; against a weight dword (h C, -h S, h C', -h S') a 4 x int8 dot product (v_dot4_i32_i8) gives two samples of
// I_X = sum h (v_i C - v_q S), against (h S, h C, ...) two samples of Q_X = sum h (v_i S + v_q C).  Weights are +1, -1 or 0 (a
// sample outside the epoch).  GPSACQ_IQ_U8 bytes are XORed with 0x80 first (byte ^ 0x80 read as int8 = byte - 128); the removed
// mean is a correction -dc * sum(weights) that costs two more dot products per dword and only when it is not zero.  All arithmetic
// is integer: the result does not depend on the order of the sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_iq_launch.hpp"
#include "track_launch.hpp"

namespace acq {

static constexpr uint64_t kFull = 1023ull << 32;  // one code period, chips * 2^32

// group g of the window: 16 bytes, or what the window still holds of them (zeros beyond)
__device__ __forceinline__ uint4 load_group(const uint8_t* iq, size_t n_bytes, uint64_t g) {
    const size_t off = (size_t)g * 16;
    if (off + 16 <= n_bytes) return *reinterpret_cast<const uint4*>(iq + off);
    uint32_t v[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; ++k)
        if (off + k < n_bytes) v[k >> 2] |= (uint32_t)iq[off + k] << (8 * (k & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ bool outside(uint64_t v, uint64_t nom, int64_t win) {
    const int64_t d = (int64_t)(v - nom);
    return d > win || d < -win;
}

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) { return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false); }

__global__ __launch_bounds__(64 * TRACK_WAVES) void k_track_iq(TrackIqArgs a) {
    __shared__ uint32_t s_chips[TRACK_WAVES][32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * TRACK_WAVES + wv;
    const bool live = c < a.n_chans;
    gpsacq_track_chan st = live ? a.chans[c] : gpsacq_track_chan{};
    if (live && lane < 32) s_chips[wv][lane] = a.chips[(st.prn - 1) * 32 + lane];
    __syncthreads();  // the only barrier: the chip table is in place
    if (!live) return;
    const uint32_t* chips = s_chips[wv];
    const gpsacq_track_params& p = a.prm;
    const uint64_t win_end = a.first_sample + a.n_samples;
    const size_t iq_bytes = 2 * a.n_samples;
    const bool dc = a.dc_i != 0 || a.dc_q != 0;
    const uint64_t lo_nom = (uint64_t)st.lo_nom, ca_nom = (uint64_t)st.ca_nom;
    uint64_t lo_int = (uint64_t)st.lo_int, ca_int = (uint64_t)st.ca_int;
    int t = 0;
    for (; t < a.max_epochs && st.status == GPSACQ_TRACK_OK; ++t) {
        const uint64_t n = (kFull - st.ca_pos + st.ca_rate - 1) / st.ca_rate;
        if (n < (uint64_t)p.min_epoch || n > (uint64_t)p.max_epoch) {
            st.status = GPSACQ_TRACK_LOST;
            break;
        }
        if (st.next_sample + n > win_end) break;
        const uint64_t o = st.next_sample - a.first_sample;  // window-relative start
        const uint64_t g0 = o >> 3, g1 = (o + n - 1) >> 3;
        int acc[6] = {0, 0, 0, 0, 0, 0};   // IE QE IP QP IL QL before the mean correction
        int sc[3] = {0, 0, 0}, ss[3] = {0, 0, 0};  // sum h C, sum -h S per E, P, L (only with a mean to remove)
        for (uint64_t gi = g0 + lane; gi <= g1; gi += 64) {
            const uint4 raw = load_group(a.iq, iq_bytes, gi);
            const uint32_t x[4] = {raw.x ^ a.flip, raw.y ^ a.flip, raw.z ^ a.flip, raw.w ^ a.flip};
            const int j0 = (int)((int64_t)(gi * 8) - (int64_t)o);  // epoch sample index of the group's first sample (> -8, < max_epoch)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t wi[3] = {0, 0, 0}, wq[3] = {0, 0, 0};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = j0 + 2 * d + h;
                    const bool ok = k >= 0 && k < (int)n;
                    const uint32_t kk = ok ? (uint32_t)k : 0u;
                    const uint32_t ph = st.lo_phase + kk * st.lo_rate;
                    const uint64_t P = st.ca_pos + (uint64_t)kk * st.ca_rate;
                    const int ip = (int)(P >> 32), f = (int)((uint32_t)P >> 31);
                    int ie = ip + f, il = ip - 1 + f;
                    ie = ie == 1023 ? 0 : ie;
                    il = il < 0 ? 1022 : il;
                    const uint32_t chip[3] = {(chips[ie >> 5] >> (ie & 31)) & 1u, (chips[ip >> 5] >> (ip & 31)) & 1u,
                                              (chips[il >> 5] >> (il & 31)) & 1u};
                    const uint32_t cb = ((ph >> 31) ^ (ph >> 30)) & 1u, sb = (~ph >> 31) & 1u;
                    const uint32_t keep = ok ? 0xFFFFu : 0u;
#pragma unroll
                    for (int X = 0; X < 3; ++X) {
                        const uint32_t bc = chip[X] ^ cb, bs = chip[X] ^ sb;  // 1: h C = -1, h S = -1
                        // bytes +1 (0x01) / -1 (0xFF): (h C, -h S) for the I arm, (h S, h C) for the Q arm
                        const uint32_t pi = (0xFF01u + 0xFEu * bc - 0xFE00u * bs) & keep;
                        const uint32_t pq = (0x0101u + 0xFEu * bs + 0xFE00u * bc) & keep;
                        wi[X] |= pi << (16 * h);
                        wq[X] |= pq << (16 * h);
                    }
                }
#pragma unroll
                for (int X = 0; X < 3; ++X) {
                    acc[2 * X] = dot4(x[d], wi[X], acc[2 * X]);
                    acc[2 * X + 1] = dot4(x[d], wq[X], acc[2 * X + 1]);
                    if (dc) {
                        sc[X] = dot4(wi[X], 0x00010001u, sc[X]);
                        ss[X] = dot4(wi[X], 0x01000100u, ss[X]);
                    }
                }
            }
        }
        if (dc) {
            // I_X = sum h ((a_i - dc_i) C - (a_q - dc_q) S),  Q_X = sum h ((a_i - dc_i) S + (a_q - dc_q) C);  ss holds sum -h S
#pragma unroll
            for (int X = 0; X < 3; ++X) {
                acc[2 * X] -= a.dc_i * sc[X] + a.dc_q * ss[X];
                acc[2 * X + 1] += a.dc_i * ss[X] - a.dc_q * sc[X];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += __shfl_xor(acc[q], m, 64);
        const int32_t IE = acc[0], QE = acc[1], IP = acc[2], QP = acc[3], IL = acc[4], QL = acc[5];
        if (lane == 0) {
            const size_t r = (size_t)c * a.max_epochs + t;
            if (a.prompt) {
                a.prompt[2 * r] = IP;
                a.prompt[2 * r + 1] = QP;
            }
            if (a.records) {
                gpsacq_track_record rec;
                rec.sample = st.next_sample;
                rec.ie = IE, rec.qe = QE, rec.ip = IP, rec.qp = QP, rec.il = IL, rec.ql = QL;
                rec.lo_rate = st.lo_rate, rec.ca_rate = st.ca_rate;
                a.records[r] = rec;
            }
        }
        // from here on the epoch update of k_track, line for line (the model text is the same)
        st.lo_phase += (uint32_t)n * st.lo_rate;
        st.ca_pos = st.ca_pos + n * st.ca_rate - kFull;
        st.next_sample += n;
        st.epoch += 1;
        const int k = st.epoch;
        // AGC
        if (p.agc_period > 0 && k % p.agc_period == 0) {
            st.pwr[st.pwr_pos] = (int64_t)IP * IP + (int64_t)QP * QP;
            st.pwr_pos = (st.pwr_pos + 1) & 7;
            int64_t S = 0;
            for (int i = 0; i < 8; ++i) S += st.pwr[i];
            if (st.gain_adj) {
                if (S < 8 * p.agc_lo) st.gain_adj = 0;
            } else if (S > 8 * p.agc_hi) {
                st.gain_adj = -1;
            }
        }
        // carrier: FLL pull-in, then Costas
        if (st.fll_left > 0) {
            const int64_t dot = (int64_t)st.prev_ip * IP + (int64_t)st.prev_qp * QP;
            const int64_t cross = (int64_t)st.prev_ip * QP - (int64_t)st.prev_qp * IP;
            const int64_t e = dot > 0 ? cross : (dot < 0 ? -cross : 0);
            lo_int += (uint64_t)e << p.fll_k;
            st.lo_rate = (uint32_t)(lo_int >> 32);
            st.fll_left -= 1;
        } else {
            const int64_t e = (int64_t)IP * QP;
            lo_int += (uint64_t)e << (p.lo_ki + st.gain_adj);
            st.lo_rate = (uint32_t)((lo_int + ((uint64_t)e << (p.lo_kp + st.gain_adj))) >> 32);
        }
        st.prev_ip = IP;
        st.prev_qp = QP;
        // code: early-minus-late power
        {
            const int64_t e = ((int64_t)IE * IE + (int64_t)QE * QE) - ((int64_t)IL * IL + (int64_t)QL * QL);
            ca_int += (uint64_t)e << p.ca_ki;
            st.ca_rate = (uint32_t)((ca_int + ((uint64_t)e << p.ca_kp)) >> 32);
        }
        // code-aided carrier reset
        if (k == p.aid_epoch) {
            lo_int = lo_nom + (ca_int - ca_nom) * 1540ull;
            st.lo_rate = (uint32_t)(lo_int >> 32);
        }
        if (outside(lo_int, lo_nom, p.lo_window) || outside((uint64_t)st.lo_rate << 32, lo_nom, p.lo_window) ||
            outside(ca_int, ca_nom, p.ca_window) || outside((uint64_t)st.ca_rate << 32, ca_nom, p.ca_window))
            st.status = GPSACQ_TRACK_LOST;
    }
    st.lo_int = (int64_t)lo_int;
    st.ca_int = (int64_t)ca_int;
    if (lane == 0) {
        a.chans[c] = st;
        a.n_epochs[c] = t;
    }
}

void launch_track_iq(const TrackIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_track_iq, dim3((unsigned)((a.n_chans + TRACK_WAVES - 1) / TRACK_WAVES)), dim3(64 * TRACK_WAVES), 0, s, a);
}

// ---------------------------------------------------------------------------------------
// 8-bit complex capture at a residual IF: gen_kernels.hip::k_generate's law (chips, navigation bits and noise as functions of the
// absolute sample index) with a complex carrier and both Box-Muller outputs as the two noise streams:
//   y[m] = sigma (n_I + j n_Q) + sum_k a_k nav_k c_k[...] exp(2 pi i ((if + fd_k) / fs m + theta_k)),  I + jQ = clamp(rint(scale y))
// One complex sample per thread.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser: counter-based noise
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_generate_iq8(GenIqArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_samples) return;
    const uint64_t m = a.first_sample + i;
    const uint64_t h = mix64(a.seed ^ (m * 0x9e3779b97f4a7c15ull));
    const float u1 = ((float)(uint32_t)(h >> 32) + 1.0f) * 2.3283064e-10f;  // (0, 1]
    const float u2 = (float)(uint32_t)h * 2.3283064e-10f;
    const float r = a.noise_sigma * sqrtf(-2.0f * __logf(u1));
    float yi = r * __cosf(6.2831853f * u2), yq = r * __sinf(6.2831853f * u2);
    for (int s = 0; s < a.n_sats; ++s) {
        const GenSat sat = a.sats[s];
        const double rr = ((double)m + sat.code_phase) * sat.chips_per_sample;
        const long long q = (long long)floor(rr);
        int idx = (int)(q % 1023);
        if (idx < 0) idx += 1023;
        float chip = ((a.chips[sat.sv * 32 + (idx >> 5)] >> (idx & 31)) & 1u) ? -1.0f : 1.0f;
        if (a.nav) {
            long long b = q / 20460;
            if (q < 0 && b * 20460 != q) --b;
            b %= a.n_nav;
            if (b < 0) b += a.n_nav;
            chip *= (float)a.nav[(size_t)s * a.n_nav + (size_t)b];
        }
        double ph = sat.cycles_per_sample * (double)m + sat.carrier_phase;
        ph -= floor(ph);
        float sn, cs;
        sincospif(2.0f * (float)ph, &sn, &cs);
        yi += sat.amplitude * chip * cs;
        yq += sat.amplitude * chip * sn;
    }
    const float vi = fminf(fmaxf(rintf(a.scale * yi), -127.0f), 127.0f), vq = fminf(fmaxf(rintf(a.scale * yq), -127.0f), 127.0f);
    uchar2 o2;
    o2.x = (unsigned char)((int)vi + a.offset);
    o2.y = (unsigned char)((int)vq + a.offset);
    reinterpret_cast<uchar2*>(a.iq)[i] = o2;
}

void launch_generate_iq8(const GenIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_generate_iq8, dim3((unsigned)((a.n_samples + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace acq
