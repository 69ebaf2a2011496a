// snapq_iq_kernels.hip -- "Snapshot signal quality on an 8-bit IQ capture" of include/gpsacq.h: the measured noise floor of every
// fine record of a multi-bit gpsacq_refine_iq8, floor = 2 * sum (v_i^2 + v_q^2) over the record's window, and with it the C/N0 and
// the weight of "Snapshot signal quality".
//
// A window is 16 blocks (1.28 MB) by default, eight tasks share a block and neighbouring windows overlap, so the sum is not walked
// per task: the capture is read ONCE per call and the tasks add up what that pass left.
// k_iq_energy: one wave64 per chunk of SNAPQ_CHUNK samples, the chunks of a wave a grid stride apart.  Lane l takes the 16-byte
// groups (8 samples) l, l + 64, ... of the chunk: one 16-byte load, the bytes XORed with 0x80 for GPSACQ_IQ_U8, and per dword one
// 4 x int8 dot product with itself (the squares of two samples, both arms) and, only where a mean is removed, two with 0x00010001 /
// 0x01000100 (the plain sums of the I and of the Q bytes).  int32 per lane (a chunk holds at most 2048 * 2^14 = 2^25), xor shuffles
// over the wave, and lane 0 writes E[c] = S2 - 2 (dc_i S_i + dc_q S_q) + n (dc_i^2 + dc_q^2) as uint64.  Only WHOLE chunks: every byte
// read lies below 2 * n_samples.  One writer per chunk; no atomics, no LDS, no barrier, no float.
// k_snap_floor: one wave64 per task, SNAPQ_IQ_WAVES per workgroup.  The window [o, o + segments * spm) is a head up to the next
// chunk boundary, whole chunks and a tail; the wave sums the E entries of the whole chunks, lane l the entries l, l + 64, ..., and
// reads only head and tail from the capture, by groups as above with the bytes of every sample outside the range cleared AFTER the
// XOR (a GPSACQ_IQ_U8 byte that is not there reads 0x80 = -128 after it).  A window inside one chunk is a single range.  Lane 0
// writes the floor.  In sign mode the floor is 2 * spm * segments and nothing else is read.
// k_snap_quality_iq: one lane per (fix, channel): snapq_device.hpp's snap_quality_info, k_snap_quality's arithmetic, with the floor
// k_snap_floor wrote.  Built with -ffp-contract=off (Makefile), like snapq_kernels.hip.
// Every loop is bounded by kernel arguments; every global store is a plain C++ store of a lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iq_groups.hpp"
#include "snapq_device.hpp"
#include "snapq_iq_launch.hpp"
#include "wave_ops.hpp"

namespace acq {

namespace {

constexpr int CHUNK_GROUPS = SNAPQ_CHUNK / 8;
static_assert((SNAPQ_CHUNK & (SNAPQ_CHUNK - 1)) == 0 && SNAPQ_CHUNK % 512 == 0 && SNAPQ_CHUNK <= 16384, "a chunk's sum of squares must fit int32");

// the three sums of one lane: squares of both arms, the I bytes, the Q bytes
struct Sums {
    int s2, si, sq;
};

__device__ __forceinline__ void add_dword(uint32_t v, bool dc, Sums& s) {
    s.s2 = dot4(v, v, s.s2);
    if (dc) {
        s.si = dot4(v, 0x00010001u, s.si);
        s.sq = dot4(v, 0x01000100u, s.sq);
    }
}

__device__ __forceinline__ Sums wave_sums(Sums s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s.s2 += __shfl_xor(s.s2, m, 64);
        s.si += __shfl_xor(s.si, m, 64);
        s.sq += __shfl_xor(s.sq, m, 64);
    }
    return s;
}

// sum of (x_i - dc_i)^2 + (x_q - dc_q)^2 over n samples from the sums of x: exact in 64-bit integers (|dc| <= 128, n < 2^47)
__device__ __forceinline__ uint64_t energy_of(const Sums& s, uint64_t n, int32_t dc_i, int32_t dc_q) {
    int64_t e = s.s2;
    if (dc_i != 0 || dc_q != 0)
        e += -2 * ((int64_t)dc_i * s.si + (int64_t)dc_q * s.sq) + (int64_t)n * ((int64_t)dc_i * dc_i + (int64_t)dc_q * dc_q);
    return (uint64_t)e;
}

// the samples [a0, a1) of the capture, a1 <= n_samples, fewer than 2 * SNAPQ_CHUNK of them: lane l the groups l, l + 64, ...
__device__ __forceinline__ void range_sums(const SnapIqCapture& c, uint64_t a0, uint64_t a1, int lane, bool dc, Sums& s) {
    if (a0 >= a1) return;
    const size_t iq_bytes = 2 * c.n_samples;
    const uint64_t g1 = (a1 - 1) >> 3;
    for (uint64_t gi = (a0 >> 3) + lane; gi <= g1; gi += 64) {
        const uint4 raw = load_group(c.iq, iq_bytes, gi);
        const uint32_t x[4] = {raw.x ^ c.flip, raw.y ^ c.flip, raw.z ^ c.flip, raw.w ^ c.flip};
        const uint64_t gs = gi << 3;
        const uint32_t b_lo = gs < a0 ? (uint32_t)(a0 - gs) : 0u;      // 0 .. 7
        const uint32_t b_hi = gs + 8 > a1 ? (uint32_t)(a1 - gs) : 8u;  // 1 .. 8
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
            const uint32_t keep = (2 * d >= b_lo && 2 * d < b_hi ? 0x0000FFFFu : 0u) | (2 * d + 1 >= b_lo && 2 * d + 1 < b_hi ? 0xFFFF0000u : 0u);
            add_dword(x[d] & keep, dc, s);
        }
    }
}

// steps 1 of the section: is record r of task t one of this capture, and which window [o, o + n) has it.  capture == false
// (sign mode): step 1 of "Snapshot signal quality" alone.  Every lane of a wave decides the same.
__device__ __forceinline__ bool snap_window(const SnapWindowArgs& w, size_t t, const gpsacq_fine& r, bool capture, uint64_t& o, uint64_t& n) {
    o = n = 0;
    if ((r.flags & FINE_UNUSABLE) || r.segments <= 0) return false;
    if (!capture) return true;
    int32_t block = (int32_t)t;
    if (w.tasks) block = w.tasks[t].block;
    if (block < 0) return false;
    o = (uint64_t)block * (uint64_t)(w.stride / 2);  // stride <= 2^31: no overflow
    n = (uint64_t)r.segments * (uint64_t)w.spm;      // below 2^47
    return o <= (uint64_t)w.n_samples && n <= (uint64_t)w.n_samples - o;
}

}  // namespace

__global__ __launch_bounds__(64 * SNAPQ_IQ_WAVES) void k_iq_energy(IqEnergyArgs a) {
    const int lane = threadIdx.x & 63;
    const bool dc = a.c.dc_i != 0 || a.c.dc_q != 0;
    const size_t waves = (size_t)gridDim.x * SNAPQ_IQ_WAVES;
    for (size_t c = (size_t)blockIdx.x * SNAPQ_IQ_WAVES + (threadIdx.x >> 6); c < a.n_chunks; c += waves) {
        const uint4* src = reinterpret_cast<const uint4*>(a.c.iq) + c * CHUNK_GROUPS;  // chunk c ends at byte 2 (c + 1) SNAPQ_CHUNK <= 2 n_samples
        Sums s = {0, 0, 0};
#pragma unroll
        for (int g = 0; g < CHUNK_GROUPS / 64; ++g) {
            const uint4 raw = src[g * 64 + lane];
            add_dword(raw.x ^ a.c.flip, dc, s);
            add_dword(raw.y ^ a.c.flip, dc, s);
            add_dword(raw.z ^ a.c.flip, dc, s);
            add_dword(raw.w ^ a.c.flip, dc, s);
        }
        s = wave_sums(s);
        if (lane == 0) a.energy[c] = energy_of(s, SNAPQ_CHUNK, a.c.dc_i, a.c.dc_q);
    }
}

__global__ __launch_bounds__(64 * SNAPQ_IQ_WAVES) void k_snap_floor(SnapFloorArgs a) {
    const int lane = threadIdx.x & 63;
    const size_t t = (size_t)blockIdx.x * SNAPQ_IQ_WAVES + (threadIdx.x >> 6);
    if (t >= a.w.n_tasks) return;
    const gpsacq_fine r = a.w.fine[t];
    uint64_t o, n, floor = 0;
    if (snap_window(a.w, t, r, !a.sign, o, n)) {
        if (a.sign) {
            floor = 2 * (uint64_t)a.w.spm * (uint64_t)r.segments;
        } else {
            const bool dc = a.c.dc_i != 0 || a.c.dc_q != 0;
            const uint64_t end = o + n;
            const uint64_t c0 = (o + SNAPQ_CHUNK - 1) / SNAPQ_CHUNK, c1 = end / SNAPQ_CHUNK;  // the whole chunks c0 .. c1 - 1; c1 <= n_chunks
            Sums s = {0, 0, 0};
            uint64_t whole = 0, edge = n;  // edge: the samples read from the capture
            if (c0 <= c1) {
                range_sums(a.c, o, c0 * SNAPQ_CHUNK, lane, dc, s);    // head, empty where o is a chunk boundary
                range_sums(a.c, c1 * SNAPQ_CHUNK, end, lane, dc, s);  // tail, empty where end is one
                for (uint64_t c = c0 + lane; c < c1; c += 64) whole += a.energy[c];
                edge = (c0 * SNAPQ_CHUNK - o) + (end - c1 * SNAPQ_CHUNK);
            } else {
                range_sums(a.c, o, end, lane, dc, s);  // no chunk boundary inside the window
            }
            floor = 2 * (wave_sum(whole) + energy_of(wave_sums(s), edge, a.c.dc_i, a.c.dc_q));
        }
    }
    if (lane == 0) a.floor[t] = floor;
}

__global__ __launch_bounds__(SNAPQ_BLOCK) void k_snap_quality_iq(SnapQualityIqArgs a) {
    const size_t i = (size_t)blockIdx.x * SNAPQ_BLOCK + threadIdx.x;
    if (i >= a.w.n_tasks) return;
    const gpsacq_fine r = a.w.fine[i];
    uint64_t o, n;
    const bool record = snap_window(a.w, i, r, true, o, n);
    const gpsacq_quality_info f = snap_quality_info(r, record, record ? a.floor[i] : 0, a.w.spm, a.fs, a.par);
    a.info[i] = f;
    if (a.obs && a.obs[i].valid != 0) a.obs[i].weight = f.weight;
}

void launch_iq_energy(const IqEnergyArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return;
    const size_t blocks = (a.n_chunks + SNAPQ_IQ_WAVES - 1) / SNAPQ_IQ_WAVES;
    hipLaunchKernelGGL(k_iq_energy, dim3((unsigned)(blocks < ((size_t)1 << 20) ? blocks : ((size_t)1 << 20))), dim3(64 * SNAPQ_IQ_WAVES), 0, s, a);
}

void launch_snap_floor(const SnapFloorArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_snap_floor, dim3((unsigned)((a.w.n_tasks + SNAPQ_IQ_WAVES - 1) / SNAPQ_IQ_WAVES)), dim3(64 * SNAPQ_IQ_WAVES), 0, s, a);
}

void launch_snap_quality_iq(const SnapQualityIqArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_snap_quality_iq, dim3((unsigned)((a.w.n_tasks + SNAPQ_BLOCK - 1) / SNAPQ_BLOCK)), dim3(SNAPQ_BLOCK), 0, s, a);
}

}  // namespace acq
