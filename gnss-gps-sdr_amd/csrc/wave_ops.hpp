// wave_ops.hpp -- what the lanes of one wave64 do with each other in the snapshot kernels, once: the wave-local LDS hand-over, the
// 64-bit xor shuffle and the sum built on it, and the two small integer helpers their reductions share (the sum of two squares,
// the larger of two (power, tag) keys).  capture_words.hpp includes it, so every kernel that goes back to a capture has it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acq {

// the lanes of ONE wave hand LDS to each other: the wave's LDS operations execute in program order, so all that is needed is
// that the compiler keeps them in it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v of lane ^ m: 32-bit shuffles of the two halves
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return (uint64_t)hi << 32 | lo;
}

// the sum of v over the wave, in every lane, modulo 2^64
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor64(v, m);
    return v;
}

__device__ __forceinline__ uint64_t sq2(int64_t a, int64_t b) { return (uint64_t)(a * a + b * b); }

// the larger of two keys (power, tag): the power first, then the tag
__device__ __forceinline__ void key_max(uint64_t& pw, uint32_t& tag, uint64_t opw, uint32_t otag) {
    if (opw > pw || (opw == pw && otag > tag)) pw = opw, tag = otag;
}

}  // namespace acq
