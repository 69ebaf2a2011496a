// track_launch.hpp -- argument blocks and launchers of the tracking channels of include/gpsacq.h: track_kernels.hip (1-bit stream)
// and track_iq_kernels.hip (8-bit IQ capture at full amplitude).  Both kernels run track_channel.hpp's loop on TrackCommon.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

constexpr int TRACK_WAVES = 4;  // channels (one wave64 each) per workgroup

// what the channel loop reads and writes, whatever the samples are
struct TrackCommon {
    uint64_t first_sample;        // the window holds samples first_sample .. first_sample + n_samples - 1 of the capture
    uint64_t n_samples;
    gpsacq_track_chan* chans;     // [n_chans] in / out (device)
    int n_chans;
    gpsacq_track_params prm;
    const uint32_t* chips;        // [32][32] C/A chips, bit i of word i / 32 (device)
    int32_t* prompt;              // [n_chans][max_epochs][2] or nullptr
    gpsacq_track_record* records; // [n_chans][max_epochs] or nullptr
    int max_epochs;
    int32_t* n_epochs;            // [n_chans] epochs run (device)
};

struct TrackArgs : TrackCommon {
    const uint8_t* bits;          // the window (device, 4-byte aligned), n_samples = 8 n_bytes
    size_t n_bytes;
};
void launch_track(const TrackArgs& a, hipStream_t s);

struct TrackIqArgs : TrackCommon {
    const uint8_t* iq;            // the window (device, 16-byte aligned), I,Q bytes
    uint32_t flip;                // 0x80808080 for GPSACQ_IQ_U8 (byte ^ 0x80 = the int8 value of byte - 128), 0 for GPSACQ_IQ_S8
    int32_t dc_i, dc_q;           // nearbyint(mean) when the mean is removed, else 0
};
void launch_track_iq(const TrackIqArgs& a, hipStream_t s);

}  // namespace acq
