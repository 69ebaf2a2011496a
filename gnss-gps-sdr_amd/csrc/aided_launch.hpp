// aided_launch.hpp -- argument blocks and launchers of "Aided acquisition: predicted code phase and Doppler, windowed search" of
// include/gpsacq.h: aided_kernels.hip's k_aid_predict (one lane per (fix, channel)) and k_aided (one workgroup per task).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "nav_launch.hpp"
#include "refine_launch.hpp"

namespace acq {

static constexpr int AIDED_WAVES = 4;        // wave64s of a k_aided workgroup; wave w takes segments w, w + 4, ...
static constexpr int AIDED_MAX_CODE_HALF = 127;  // W: 2 W + 1 <= 255 hypotheses, at most AIDED_PASSES passes of 64 lanes
static constexpr int AIDED_MAX_DOP_HALF = 8;     // K
static constexpr int AIDED_PASSES = 4;

struct AidPredictArgs {
    const NavEph* eph;  // [n_eph] (device)
    int n_eph;
    const gpsacq_fix* fix;  // [n_fix] (device)
    const gpsacq_vel* vel;  // [n_fix] (device), or NULL: at rest
    size_t n_fix;
    int chans;             // 1 .. GPSACQ_FIX_MAX_SATS
    double fs, step_hz;    // step_hz: gpsacq_info.doppler_step_hz
    int spm, kmax;         // samples per millisecond; the grid is -kmax .. +kmax
    gpsacq_aid_params p;
    gpsacq_aid* out;  // [n_fix][chans] (device)
};
void launch_aid_predict(const AidPredictArgs& a, hipStream_t s);

struct AidedArgs {
    BitCaptureArgs c;
    int kmax;               // the grid is -kmax .. +kmax
    const gpsacq_aid* aid;  // [n_tasks] (device)
    gpsacq_aided_params p;
    gpsacq_aided* out;             // [n_tasks] (device)
    gpsacq_peak* peaks_out;        // [n_tasks]
    unsigned long long* powers;    // [n_tasks][2 K + 1][2 W + 1], or NULL
};
void launch_aided(const AidedArgs& a, hipStream_t s);

// ---- "Coherent aided acquisition" of include/gpsacq.h: k_aided_coh (one workgroup per task) and k_aid_instant (one lane per fix)
static constexpr int COH_MAX_CODE_HALF = 31;  // W: 2 W + 1 <= 63 hypotheses, one pass of 64 lanes
static constexpr int COH_MAX_FINE_HALF = 7;   // F
static constexpr int COH_MAX_FINE_STEP = 512; // u, in 1/1024 cycle per segment
static constexpr int COH_MAX_Z = 5120;        // entries of the z matrix in LDS: fit * (2 W + 1) at most
static constexpr int COH_TABLE = 1024;        // entries of the rotation table: C[0 .. 1023], then S[0 .. 1023]
// the key is power << 20 | 31 - d << 15 | 15 - g << 11 | 31 - e << 6 | 63 - h: the power may take 44 bits
static constexpr int COH_KEY_SHIFT = 20;
static_assert(2 * AIDED_MAX_DOP_HALF + 1 <= 32 && 2 * COH_MAX_FINE_HALF + 1 <= 16 && 2 * COH_MAX_CODE_HALF + 1 <= 64, "the key's fields");

// AidedArgs with this section's parameters and record, and the rotation table
struct AidedCohArgs {
    BitCaptureArgs c;
    int kmax;
    const gpsacq_aid* aid;         // [n_tasks] (device)
    const int16_t* table;          // [2 * COH_TABLE] (device): gpsacq_aided_coh_table's
    gpsacq_aided_coh_params p;
    gpsacq_aided_coh* out;         // [n_tasks] (device)
    gpsacq_peak* peaks_out;        // [n_tasks]
    unsigned long long* powers;    // [n_tasks][2 K + 1][2 F + 1][M][2 W + 1], or NULL
};
void launch_aided_coh(const AidedCohArgs& a, hipStream_t s);

struct AidInstantArgs {
    const gpsacq_fix* fix;            // [n_fix] (device)
    const gpsacq_coarse_info* info;   // [n_fix]
    const gpsacq_coarse_prior* prior; // [n_fix]
    size_t n_fix;
    gpsacq_fix* out;                  // [n_fix]; may be fix itself
};
void launch_aid_instant(const AidInstantArgs& a, hipStream_t s);

}  // namespace acq
