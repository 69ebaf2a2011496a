// coarse_launch.hpp -- argument blocks and launchers of "Coarse-time fixes: positions from code phases alone" of include/gpsacq.h:
// coarse_kernels.hip's k_coarse_obs (one lane per (fix, channel)) and k_coarse_fix (one lane per fix) -- and of "Coarse-time fix
// integrity": k_coarse_exclude (sixteen lanes per fix), which runs behind k_coarse_fix.
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

constexpr int COARSE_GROUP = 16;  // lanes of k_coarse_exclude per fix: four fixes per wave64
static_assert(NAV_BLOCK % COARSE_GROUP == 0 && GPSACQ_FIX_MAX_SATS <= COARSE_GROUP, "a fix's group lies inside one workgroup");

struct CoarseRaimArgs {
    CoarseFixArgs fix;  // as k_coarse_fix had them: out and info hold FULL's records, which the winning lane overwrites; work is unread
    gpsacq_raim_params r;
    gpsacq_fix_raim* raim;  // [n_fix] (device)
    gpsacq_obs* cand;       // [n_fix][sats][sats] (device scratch): candidate k of fix f works in row f * sats + k
    gpsacq_obs* obs_out;    // [n_fix][sats] (device), or NULL: where the winning lane copies its row
};
void launch_coarse_exclude(const CoarseRaimArgs& a, hipStream_t s);

}  // namespace acq
