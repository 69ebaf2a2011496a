// raim_launch.hpp -- argument block and launchers of "Fix integrity: residual test and single-satellite exclusion" of
// include/gpsacq.h: fix_kernels.hip's k_raim_detect (one lane per fix) and k_raim_exclude (sixteen lanes per fix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nav_launch.hpp"

namespace acq {

constexpr int RAIM_GROUP = 16;  // lanes of k_raim_exclude per fix: four fixes per wave64
static_assert(NAV_BLOCK % RAIM_GROUP == 0 && GPSACQ_FIX_MAX_SATS <= RAIM_GROUP, "a fix's group lies inside one workgroup");

// what k_raim_detect leaves in engine scratch for k_raim_exclude.  `go` is written for EVERY row; the rest only where go != 0
struct RaimRow {
    double x, y, z, bias;  // the full solution's state; bias: metres of light time taken off t0
    double t0;
    double delay[GPSACQ_FIX_MAX_SATS];  // the delays of the full solution's last round
    double stat_full;
    uint32_t mask;  // S: the usable observations the elevation mask left
    int32_t go;     // 1: the row goes on to EXCLUDE
    int32_t steps;  // of FULL
    int32_t n_masked;
};  // 160 bytes

struct RaimArgs {
    const NavEph* eph;
    int n_eph;
    const gpsacq_obs* obs;          // [n_fix][sats] (device)
    const gpsacq_sat_state* state;  // [n_fix][sats], k_sat_state's output for obs
    size_t n_fix;
    int sats;  // 1 .. GPSACQ_FIX_MAX_SATS
    gpsacq_atm_params p;
    gpsacq_raim_params r;
    gpsacq_fix* out;        // [n_fix] (device)
    gpsacq_fix_dop* dop;    // [n_fix] (device)
    gpsacq_fix_raim* raim;  // [n_fix] (device)
    RaimRow* rows;          // [n_fix] (device scratch)
};
void launch_raim_detect(const RaimArgs& a, hipStream_t s);
void launch_raim_exclude(const RaimArgs& a, hipStream_t s);

}  // namespace acq
