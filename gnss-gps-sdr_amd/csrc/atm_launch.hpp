// atm_launch.hpp -- argument blocks and launchers of "Atmosphere, elevation mask and DOP" of include/gpsacq.h: fix_kernels.hip's
// k_sat_view (one lane per observation) and k_fix_atm (one lane per fix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nav_launch.hpp"

namespace acq {

struct SatViewArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;          // [n_fix][sats] (device)
    const gpsacq_sat_state* state;  // [n_fix][sats], k_sat_state's output for obs
    const gpsacq_fix* fix;          // [n_fix]
    size_t n_obs;                   // n_fix * sats
    int sats;                       // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_atm_params p;
    gpsacq_sat_view* out;  // [n_fix][sats] (device)
};
void launch_sat_view(const SatViewArgs& a, hipStream_t s);

struct FixAtmArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;          // [n_fix][sats] (device)
    const gpsacq_sat_state* state;  // [n_fix][sats], k_sat_state's output for obs
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_atm_params p;
    gpsacq_fix* out;      // [n_fix] (device)
    gpsacq_fix_dop* dop;  // [n_fix] (device)
};
void launch_fix_atm(const FixAtmArgs& a, hipStream_t s);

}  // namespace acq
