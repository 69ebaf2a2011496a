// track_iq_launch.hpp -- argument blocks and launchers of track_iq_kernels.hip (multi-bit complex tracking channels and the
// 8-bit IQ capture generator of include/gpsacq.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "gen_launch.hpp"

namespace acq {

struct TrackIqArgs {
    const uint8_t* iq;            // window of the capture (device, 16-byte aligned): samples first_sample .. + n_samples - 1, I,Q bytes
    size_t n_samples;
    uint64_t first_sample;
    uint32_t flip;                // 0x80808080 for GPSACQ_IQ_U8 (byte ^ 0x80 = the int8 value of byte - 128), 0 for GPSACQ_IQ_S8
    int32_t dc_i, dc_q;           // nearbyint(mean) when the mean is removed, else 0
    gpsacq_track_chan* chans;     // [n_chans] in / out (device)
    int n_chans;
    gpsacq_track_params prm;
    const uint32_t* chips;        // [32][32] C/A chips, bit i of word i / 32 (device)
    int32_t* prompt;              // [n_chans][max_epochs][2] or nullptr
    gpsacq_track_record* records; // [n_chans][max_epochs] or nullptr
    int max_epochs;
    int32_t* n_epochs;            // [n_chans] epochs run (device)
};
void launch_track_iq(const TrackIqArgs& a, hipStream_t s);

struct GenIqArgs {
    uint8_t* iq;          // [2 * n_samples] interleaved I, Q
    size_t n_samples;
    uint64_t first_sample;
    uint64_t seed;
    const GenSat* sats;   // device; cycles_per_sample = (if_hz + fd) / fs
    int n_sats;
    float noise_sigma, scale;
    int offset;           // 128 for GPSACQ_IQ_U8, 0 for GPSACQ_IQ_S8
    const int8_t* nav;    // [n_sats][n_nav] navigation bits +-1 (device), or nullptr
    int n_nav;
    const uint32_t* chips; // [32][32] C/A chips, bit i of word i / 32 (device): the table of the tracking channels
};
void launch_generate_iq8(const GenIqArgs& a, hipStream_t s);

}  // namespace acq
