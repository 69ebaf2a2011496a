// obs_launch.hpp -- argument blocks and launchers of the observables of include/gpsacq.h ("Observables"): obs_kernels.hip's
// k_code_pos (one wave64 per channel) and k_observe (one lane per (instant, channel)), and of "Carrier observables":
// k_carrier_acc (one wave64 per channel) and k_observe_rate (one lane per (instant, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

constexpr int OBS_BLOCK = 64;  // lanes per workgroup of both kernels: one wave
constexpr int OBS_RUN = 4;     // k_code_pos: consecutive epochs per lane, so one pass of the wave covers 256 epochs

// what the kernels read of one channel: the state after the tracking call, the epoch count, and the time tag
struct ObsChan {
    uint64_t ca_pos;       // pos_n
    uint64_t next_sample;  // end of the last record
    int32_t n;             // records of this channel, 0 .. max_epochs
    int32_t first_epoch;   // chans[c].epoch - n
    int32_t tag_epoch, tag_ms, tag_eph, tag_valid;
};  // 40 bytes

struct CodePosArgs {
    const ObsChan* chan;                 // [n_chans] (device)
    const gpsacq_track_record* records;  // [n_chans][max_epochs] (device)
    int max_epochs;
    uint64_t* pos;  // [n_chans][max_epochs] (device): pos_t of the model, written for t < n
};
void launch_code_pos(const CodePosArgs& a, int n_chans, hipStream_t s);

struct ObserveArgs {
    const ObsChan* chan;
    const gpsacq_track_record* records;
    const uint64_t* pos;
    int max_epochs;
    int n_chans;  // 1 .. GPSACQ_FIX_MAX_SATS
    uint64_t first_rx_sample, rx_step;
    size_t n_fix;
    gpsacq_obs* out;  // [n_fix][n_chans] (device)
};
void launch_observe(const ObserveArgs& a, hipStream_t s);

// what the carrier kernels read of one channel
struct RateChan {
    uint64_t next_sample;  // end of the last record
    int32_t n;             // records of this channel, 0 .. max_epochs
    uint32_t nom_word;     // carrier NCO word of zero Doppler
};  // 16 bytes

struct CarrierAccArgs {
    const RateChan* chan;                // [n_chans] (device)
    const gpsacq_track_record* records;  // [n_chans][max_epochs] (device)
    int max_epochs;
    int64_t* acc;  // [n_chans][max_epochs + 1] (device): A_t of the model, written for t <= n
};
void launch_carrier_acc(const CarrierAccArgs& a, int n_chans, hipStream_t s);

struct ObserveRateArgs {
    const RateChan* chan;
    const gpsacq_track_record* records;
    const int64_t* acc;
    int max_epochs;
    int n_chans;  // 1 .. GPSACQ_FIX_MAX_SATS
    uint64_t first_rx_sample, rx_step, avg_samples;
    double fs;
    size_t n_fix;
    gpsacq_rate_obs* out;  // [n_fix][n_chans] (device)
};
void launch_observe_rate(const ObserveRateArgs& a, hipStream_t s);

}  // namespace acq
