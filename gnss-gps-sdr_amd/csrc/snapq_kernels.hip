// snapq_kernels.hip -- "Snapshot signal quality" of include/gpsacq.h: the C/N0 of a fine code-phase record from its prompt power
// over the analytic noise floor of a +-1 stream, and from it the weight of the record's observation.  Integers up to the
// conversions of sig and floor; then two divisions, one product, one log10, one more division.
//
// k_snap_quality: one lane per (fix, channel), SNAPQ_BLOCK lanes per workgroup, a bounds check on the flat index.  No LDS, no
// barrier, no atomics, no loop.  Reads 56 bytes, writes the 48-byte info and, where the observation is valid, the 8 bytes of its
// weight.
// Built with -ffp-contract=off (Makefile): every step is one IEEE operation, so lin and weight are the reference's to the bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snapq_launch.hpp"

namespace acq {

namespace {
constexpr int FINE_UNUSABLE = GPSACQ_FINE_NO_HIT | GPSACQ_FINE_NO_POWER | GPSACQ_FINE_FEW;
}  // namespace

__global__ __launch_bounds__(SNAPQ_BLOCK) void k_snap_quality(SnapQualityArgs a) {
    const size_t i = (size_t)blockIdx.x * SNAPQ_BLOCK + threadIdx.x;
    if (i >= a.n_obs) return;
    const gpsacq_fine r = a.fine[i];
    gpsacq_quality_info f;
    f.epochs = 0;
    f.flags = GPSACQ_QUALITY_NO_RECORD;
    f.sig = f.noise = 0;
    f.lin = f.cn0_dbhz = f.weight = 0.0;
    if (!(r.flags & FINE_UNUSABLE) && r.segments > 0) {
        const uint64_t floor = 2 * (uint64_t)a.spm * (uint64_t)r.segments;
        const uint64_t sig = r.prompt > floor ? r.prompt - floor : 0;
        int32_t flags = r.segments < a.par.min_segments ? GPSACQ_QUALITY_SHORT : 0;
        double lin = 0.0, db = 0.0;
        if (sig == 0) {
            flags |= GPSACQ_QUALITY_NO_POWER;
        } else {
            const double snr = (double)sig / (double)floor;
            lin = snr * (a.fs / (double)a.spm);
            db = 10.0 * log10(lin);
        }
        double weight = 0.0;
        const bool gated = (flags & (GPSACQ_QUALITY_NO_POWER | GPSACQ_QUALITY_SHORT)) != 0 || lin < a.par.cn0_min_lin;
        if (!gated) {
            const double w = lin / a.par.cn0_ref_lin;
            weight = w < 1.0 ? w : 1.0;
        }
        f.epochs = r.segments;
        f.flags = flags;
        f.sig = sig;
        f.noise = floor;
        f.lin = lin;
        f.cn0_dbhz = db;
        f.weight = weight;
    }
    a.info[i] = f;
    if (a.obs && a.obs[i].valid != 0) a.obs[i].weight = f.weight;
}

void launch_snap_quality(const SnapQualityArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_snap_quality, dim3((unsigned)((a.n_obs + SNAPQ_BLOCK - 1) / SNAPQ_BLOCK)), dim3(SNAPQ_BLOCK), 0, s, a);
}

}  // namespace acq
