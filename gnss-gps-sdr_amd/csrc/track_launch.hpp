// track_launch.hpp -- argument block and launcher of track_kernels.hip (the tracking channels of include/gpsacq.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

constexpr int TRACK_WAVES = 4;  // channels (one wave64 each) per workgroup

struct TrackArgs {
    const uint8_t* bits;          // window of the capture (device, 4-byte aligned): samples first_sample .. + 8 n_bytes - 1
    size_t n_bytes;
    uint64_t first_sample;
    gpsacq_track_chan* chans;     // [n_chans] in / out (device)
    int n_chans;
    gpsacq_track_params prm;
    const uint32_t* chips;        // [32][32] C/A chips, bit i of word i / 32 (device)
    int32_t* prompt;              // [n_chans][max_epochs][2] or nullptr
    gpsacq_track_record* records; // [n_chans][max_epochs] or nullptr
    int max_epochs;
    int32_t* n_epochs;            // [n_chans] epochs run (device)
};
void launch_track(const TrackArgs& a, hipStream_t s);

}  // namespace acq
