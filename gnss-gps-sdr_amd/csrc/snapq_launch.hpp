// snapq_launch.hpp -- argument block and launcher of "Snapshot signal quality" of include/gpsacq.h: snapq_kernels.hip's
// k_snap_quality (one lane per (fix, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

static constexpr int SNAPQ_BLOCK = 256;  // lanes of a k_snap_quality workgroup

struct SnapQualityArgs {
    const gpsacq_fine* fine;  // [n_fix][n_chans] (device)
    size_t n_obs;             // n_fix * n_chans
    int spm;                  // samples per millisecond, gpsacq_info.num_lags
    double fs;
    gpsacq_snap_quality_params par;  // checked
    gpsacq_obs* obs;                 // [n_fix][n_chans] (device) in-out, or NULL
    gpsacq_quality_info* info;       // [n_fix][n_chans] (device)
};
void launch_snap_quality(const SnapQualityArgs& a, hipStream_t s);

}  // namespace acq
