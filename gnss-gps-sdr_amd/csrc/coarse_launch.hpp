// coarse_launch.hpp -- argument blocks and launchers of "Coarse-time fixes: positions from code phases alone" of include/gpsacq.h:
// coarse_kernels.hip's k_coarse_obs (one lane per (fix, channel)) and k_coarse_fix (one lane per fix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nav_launch.hpp"

namespace acq {

struct CoarseObsArgs {
    const gpsacq_peak* peaks;  // [n_fix][chans] (device)
    size_t n_obs;              // n_fix * chans
    int chans;                 // 1 .. GPSACQ_FIX_MAX_SATS
    double fs, snr_min;
    gpsacq_obs* out;  // [n_fix][chans] (device)
};
void launch_coarse_obs(const CoarseObsArgs& a, hipStream_t s);

struct CoarseFixArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;             // [n_fix][sats] (device)
    const gpsacq_coarse_prior* prior;  // [n_fix]
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_coarse_params p;
    gpsacq_fix* out;           // [n_fix] (device)
    gpsacq_coarse_info* info;  // [n_fix]
    gpsacq_obs* work;          // [n_fix][sats]: the caller's obs_out or engine scratch; never obs itself
};
void launch_coarse_fix(const CoarseFixArgs& a, hipStream_t s);

}  // namespace acq
