// refine_launch.hpp -- argument blocks and launchers of "Fine code phases: search peaks refined below a sample" of include/gpsacq.h:
// refine_kernels.hip's k_refine (one workgroup per task) and k_coarse_obs_fine (one lane per (fix, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"

namespace acq {

static constexpr int REFINE_WAVES = 4;  // wave64s of a k_refine workgroup; wave w takes segments w, w + 4, ...
// k_refine keeps the chips of a 32-sample word in one 32-chip window: early's last chip is at most 2 + 31 ca_rate / 2^32 chips past
// late's first, so the code NCO must stay at or below 0.9 chips per sample (29.9 < 32).  A hit has fc + lo_dop < fs, hence
// lo_dop < fs and ca_rate / 2^32 < 1.023e6 / fs + 1 / 1540: the host checks that bound once, for the engine's fs (fs >= 1.138 MHz).
static constexpr double REFINE_MAX_CHIPS_PER_SAMPLE = 0.9;

// a 1-bit capture as the snapshot kernels are told of it, ONCE: its tasks and peaks, the chip table and the engine's grid.  RefineArgs,
// FineDopArgs (doppler_launch.hpp), AidedArgs and AidedCohArgs (aided_launch.hpp) carry it as `c`, gpsacq_nav.cpp's capture_args
// fills it; IqCaptureArgs of snapshot_iq_launch.hpp is its counterpart for an 8-bit IQ capture
struct BitCaptureArgs {
    const uint32_t* words;  // the capture from its 4-byte-aligned base (device): the caller's pointer rounded down
    size_t n_bytes;         // bytes that may be read from `words` (the caller's n_bytes + lead)
    uint32_t lead;          // bytes between `words` and the caller's pointer, 0..3
    size_t stride;          // bytes between blocks
    const gpsacq_task* tasks;  // [n_tasks] (device), or NULL: task t = (block t, PRN t % 32)
    const gpsacq_peak* peaks;  // [n_tasks] (device); the aided searches' peaks_in, which may be NULL
    size_t n_tasks;
    const uint32_t* chips;  // [32][32] C/A chip words (device)
    double fc, fs, step_hz;  // step_hz: the engine's Doppler grid step, 0 on the reference grid (lo_shift in FFT bins)
    int spm;                 // samples per millisecond, <= 65535
};

// a fine record with one of these flags gives no observation and no quality (k_coarse_obs_fine, snapq_device.hpp)
static constexpr int FINE_UNUSABLE = GPSACQ_FINE_NO_HIT | GPSACQ_FINE_NO_POWER | GPSACQ_FINE_FEW;

struct RefineArgs {
    BitCaptureArgs c;
    gpsacq_refine_params p;
    gpsacq_fine* out;  // [n_tasks] (device)
};
void launch_refine(const RefineArgs& a, hipStream_t s);

struct CoarseObsFineArgs {
    const gpsacq_peak* peaks;  // [n_fix][chans] (device)
    const gpsacq_fine* fine;   // [n_fix][chans]
    size_t n_obs;              // n_fix * chans
    int chans;                 // 1 .. GPSACQ_FIX_MAX_SATS
    double fs, snr_min;
    gpsacq_obs* out;  // [n_fix][chans] (device)
};
void launch_coarse_obs_fine(const CoarseObsFineArgs& a, hipStream_t s);

}  // namespace acq
