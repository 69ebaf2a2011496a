// snapq_kernels.hip -- "Snapshot signal quality" of include/gpsacq.h: the C/N0 of a fine code-phase record from its prompt power
// over the analytic noise floor of a +-1 stream, and from it the weight of the record's observation.  Integers up to the
// conversions of sig and floor; then two divisions, one product, one log10, one more division.
//
// k_snap_quality: one lane per (fix, channel), SNAPQ_BLOCK lanes per workgroup, a bounds check on the flat index.  No LDS, no
// barrier, no atomics, no loop.  Reads 56 bytes, writes the 48-byte info and, where the observation is valid, the 8 bytes of its
// weight.
// Steps 2 (sig, noise) to 7 are snapq_device.hpp's snap_quality_info, which k_snap_quality_iq (snapq_iq_kernels.hip) calls too.
// Built with -ffp-contract=off (Makefile): every step is one IEEE operation, so lin and weight are the reference's to the bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snapq_device.hpp"
#include "snapq_launch.hpp"

namespace acq {

__global__ __launch_bounds__(SNAPQ_BLOCK) void k_snap_quality(SnapQualityArgs a) {
    const size_t i = (size_t)blockIdx.x * SNAPQ_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_fine r = a.fine[i];
    const bool record = !(r.flags & FINE_UNUSABLE) && r.segments > 0;          // step 1
    const uint64_t floor = record ? 2 * (uint64_t)a.spm * (uint64_t)r.segments : 0;  // step 2, the analytic floor
    const gpsacq_quality_info f = snap_quality_info(r, record, floor, a.spm, a.fs, a.par);
    a.info[i] = f;
    if (a.obs && a.obs[i].valid != 0) a.obs[i].weight = f.weight;
}

void launch_snap_quality(const SnapQualityArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_snap_quality, dim3((unsigned)((a.n_obs + SNAPQ_BLOCK - 1) / SNAPQ_BLOCK)), dim3(SNAPQ_BLOCK), 0, s, a);
}

}  // namespace acq
