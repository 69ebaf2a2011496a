// quality_launch.hpp -- argument blocks and launchers of "Signal quality per observation" of include/gpsacq.h: quality_kernels.hip's
// k_quality_acc (one wave64 per channel) and k_quality_out (one lane per (instant, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "smooth_launch.hpp"  // SMOOTH_BLOCK, SMOOTH_RUN: k_quality_acc walks the epochs in k_lock_acc's chunks

namespace acq {

// what the kernels read of one channel
struct QualityChan {
    uint64_t next_sample;  // end of the last record
    int32_t n;             // records of this channel, 0 .. max_epochs
    int32_t tag_valid;
};  // 16 bytes

struct QualityAccArgs {
    const QualityChan* chan;             // [n_chans] (device)
    const gpsacq_track_record* records;  // [n_chans][max_epochs] (device)
    int max_epochs;
    // [n_chans][max_epochs + 1] each (device): the sums over u < t of |ip_u|, ip_u^2 + qp_u^2, ip_u^2 - qp_u^2 mod 2^64, written for t <= n
    uint64_t* sum_a;
    uint64_t* sum_d;
    uint64_t* sum_n;
};
void launch_quality_acc(const QualityAccArgs& a, int n_chans, hipStream_t s);

struct QualityOutArgs {
    const QualityChan* chan;
    const gpsacq_track_record* records;
    const uint64_t* sum_a;  // k_quality_acc's output
    const uint64_t* sum_d;
    const uint64_t* sum_n;
    int max_epochs;
    int n_chans;  // 1 .. GPSACQ_FIX_MAX_SATS
    uint64_t first_rx_sample, rx_step;
    size_t n_fix;
    gpsacq_quality_params par;  // checked
    gpsacq_obs* obs;            // [n_fix][n_chans] (device) in-out, or NULL
    gpsacq_quality_info* info;  // [n_fix][n_chans] (device)
};
void launch_quality_out(const QualityOutArgs& a, hipStream_t s);

}  // namespace acq
