// iq_groups.hpp -- the pieces of the dot-product correlator on interleaved 8-bit I, Q bytes that its two users share:
// track_iq_kernels.hip (IqCorr, the multi-bit tracking channels) and capture_groups.hpp (the snapshot kernels on an IQ capture).
// A 16-byte group holds 8 samples (I0 Q0 I1 Q1 ...), a dword two; against a weight dword (h C, -h S, h C', -h S') a 4 x int8 dot
// product (v_dot4_i32_i8) gives two samples of I_X = sum h (v_i C - v_q S), against (h S, h C, ...) two samples of
// Q_X = sum h (v_i S + v_q C).  Weights are +1, -1 or 0 (a sample that does not count).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace acq {

// group g of the window: 16 bytes, or what the window still holds of them (zeros beyond)
__device__ __forceinline__ uint4 load_group(const uint8_t* iq, size_t n_bytes, uint64_t g) {
    const size_t off = (size_t)g * 16;
    if (off + 16 <= n_bytes) return *reinterpret_cast<const uint4*>(iq + off);
    uint32_t v[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; ++k)
        if (off + k < n_bytes) v[k >> 2] |= (uint32_t)iq[off + k] << (8 * (k & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) { return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false); }

// the two weight bytes of one sample for the I arm (h C, -h S) and for the Q arm (h S, h C), +1 (0x01) / -1 (0xFF); bc, bs: 1 where
// h C = -1, resp. h S = -1; keep: 0xFFFF, or 0 for a sample that does not count
__device__ __forceinline__ void weight_bytes(uint32_t bc, uint32_t bs, uint32_t keep, uint32_t& pi, uint32_t& pq) {
    pi = (0xFF01u + 0xFEu * bc - 0xFE00u * bs) & keep;
    pq = (0x0101u + 0xFEu * bs + 0xFE00u * bc) & keep;
}

}  // namespace acq
