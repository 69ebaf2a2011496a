// smooth_launch.hpp -- argument blocks and launchers of "Carrier-smoothed observables" of include/gpsacq.h: smooth_kernels.hip's
// k_lock_acc and k_smooth_scan (one wave64 per channel), k_cmc and k_smooth_out (one lane per (instant, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

constexpr int SMOOTH_BLOCK = 64;  // lanes per workgroup of all four kernels: one wave
constexpr int SMOOTH_RUN = 4;     // k_lock_acc, k_smooth_scan: consecutive epochs / instants per lane, 256 per pass of the wave

// the state of an instant, as k_cmc leaves it for the two kernels after it
constexpr int32_t SMOOTH_INVALID = 0, SMOOTH_RAW = 1, SMOOTH_LOCKED = 2;

// what the kernels read of one channel
struct SmoothChan {
    uint64_t next_sample;  // end of the last record
    int32_t n;             // records of this channel, 0 .. max_epochs
    int32_t first_epoch;   // chans[c].epoch - n
    int32_t tag_epoch, tag_ms, tag_eph, tag_valid;
    uint32_t cw;           // nominal code word
    uint32_t nom_word;     // carrier NCO word of zero Doppler
};  // 40 bytes

struct LockAccArgs {
    const SmoothChan* chan;              // [n_chans] (device)
    const gpsacq_track_record* records;  // [n_chans][max_epochs] (device)
    int max_epochs;
    int64_t* lock_n;  // [n_chans][max_epochs + 1] (device): sum over u < t of ip_u^2 - qp_u^2, written for t <= n
    int64_t* lock_d;  // the same of ip_u^2 + qp_u^2
};
void launch_lock_acc(const LockAccArgs& a, int n_chans, hipStream_t s);

struct CmcArgs {
    const SmoothChan* chan;
    const gpsacq_track_record* records;
    const uint64_t* pos;    // k_code_pos's output: [n_chans][max_epochs]
    const int64_t* acc;     // k_carrier_acc's output: [n_chans][max_epochs + 1]
    const int64_t* lock_n;  // k_lock_acc's output; not read when lock_epochs == 0
    const int64_t* lock_d;
    int max_epochs;
    int n_chans;  // 1 .. GPSACQ_FIX_MAX_SATS
    uint64_t first_rx_sample, rx_step;
    size_t n_fix;
    int32_t lock_epochs, lock_num, lock_den, invert;
    // channel-major [n_chans][n_fix] (device): Z (0 where the instant is not locked), P, t and the state of every instant
    uint64_t* z;
    uint64_t* p;
    int32_t* t;
    int32_t* state;
};
void launch_cmc(const CmcArgs& a, hipStream_t s);

struct SmoothScanArgs {
    const uint64_t* z;
    const int32_t* state;
    size_t n_fix;
    int64_t jump;
    uint64_t* sum;  // [n_chans][n_fix + 1] (device): S_k of the model
    int32_t* seg;   // [n_chans][n_fix] (device): s_i of the model at every locked instant
};
void launch_smooth_scan(const SmoothScanArgs& a, int n_chans, hipStream_t s);

struct SmoothOutArgs {
    const SmoothChan* chan;
    const uint64_t* z;
    const uint64_t* p;
    const int32_t* t;
    const int32_t* state;
    const uint64_t* sum;
    const int32_t* seg;
    int n_chans;
    size_t n_fix;
    int32_t window;
    gpsacq_obs* out;           // [n_fix][n_chans] (device)
    gpsacq_smooth_info* info;  // [n_fix][n_chans] (device), or NULL
};
void launch_smooth_out(const SmoothOutArgs& a, hipStream_t s);

}  // namespace acq
