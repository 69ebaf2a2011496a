// doppler_launch.hpp -- argument blocks and launchers of "Cold snapshot fixes: fine Doppler and a Doppler-only position solver" of
// include/gpsacq.h: doppler_kernels.hip's k_fine_dop (one workgroup per task), k_rate_obs_fine (one lane per (fix, channel)) and
// k_doppler_fix (one lane per fix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nav_launch.hpp"
#include "refine_launch.hpp"

namespace acq {

static constexpr int DOP_WAVES = 4;  // wave64s of a k_fine_dop workgroup; wave w takes segments w, w + 4, ...
// k_fine_dop keeps every segment's (I, Q) in LDS: 64 blocks * 40000 / 1137 samples per millisecond (the smallest engine
// gpsacq_refine accepts) are 2251 segments; the host refuses a window of more (18 KB)
static constexpr int DOP_MAX_SEGMENTS = 2304;

struct FineDopArgs {
    BitCaptureArgs c;
    gpsacq_dopfine_params p;
    gpsacq_dopfine* out;  // [n_tasks] (device)
};
void launch_fine_dop(const FineDopArgs& a, hipStream_t s);

struct RateObsFineArgs {
    const gpsacq_peak* peaks;       // [n_fix][chans] (device)
    const gpsacq_dopfine* dopfine;  // [n_fix][chans]
    size_t n_obs;                   // n_fix * chans
    double snr_min;
    gpsacq_rate_obs* out;  // [n_fix][chans] (device)
};
void launch_rate_obs_fine(const RateObsFineArgs& a, hipStream_t s);

struct DopplerFixArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;            // [n_fix][sats] (device): eph and valid are read
    const gpsacq_rate_obs* rate_obs;  // [n_fix][sats]
    const int32_t* rx_ms;             // [n_fix]
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_doppler_fix_params p;
    double* tau;                 // [n_fix][sats] scratch: the light time of a usable column, -1 for any other
    gpsacq_doppler_fix* out;     // [n_fix] (device)
    gpsacq_coarse_prior* prior;  // [n_fix], or NULL
};
void launch_doppler_fix(const DopplerFixArgs& a, hipStream_t s);

}  // namespace acq
