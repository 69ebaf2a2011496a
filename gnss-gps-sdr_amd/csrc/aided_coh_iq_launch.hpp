// aided_coh_iq_launch.hpp -- argument block and launcher of "Coherent aided acquisition on an 8-bit IQ capture" of include/gpsacq.h,
// multi-bit mode: aided_coh_iq_kernels.hip's k_aided_coh_iq<M> (one workgroup per task).  Sign mode runs k_aided_coh of
// aided_launch.hpp on the converted capture and needs nothing from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aided_launch.hpp"
#include "snapshot_iq_launch.hpp"

namespace acq {

static constexpr int AIDED_COH_IQ_WAVES = 4;  // wave64s of a workgroup; wave w takes segments w, w + 4, ...
// the prefix array of a wave as aided_iq_walk.hpp's segment_sums_by_parts takes it: W <= 31, so one pass of 64 lanes and 64 slots
// in front; a chunk of 512 samples keeps the kernel's LDS below half a CU's
struct AidedCohIqGeometry {
    static constexpr int CHUNK = 512, PAD = 64;
};
static constexpr int AIDED_COH_IQ_SLOTS = AidedCohIqGeometry::PAD + AidedCohIqGeometry::CHUNK + 64;  // A[k] in slot PAD + k, k = -63 .. n + 2 W - 1
static constexpr int AIDED_COH_IQ_LIST = AidedCohIqGeometry::CHUNK + 64;                             // transitions of a chunk's stream: at most n + 2 W - 1 <= 573
static_assert(2 * COH_MAX_CODE_HALF <= AidedCohIqGeometry::PAD - 2 && ((AidedCohIqGeometry::CHUNK + 2 * COH_MAX_CODE_HALF - 1 + 3) & ~3) <= AIDED_COH_IQ_LIST && AidedCohIqGeometry::CHUNK % 8 == 0, "the pads");

struct AidedCohIqArgs {
    IqCaptureArgs c;
    int kmax;                     // the grid is -kmax .. +kmax
    const gpsacq_aid* aid;        // [n_tasks] (device)
    const int16_t* table;         // [2 * COH_TABLE] (device): gpsacq_aided_coh_table's
    gpsacq_aided_coh_params p;
    gpsacq_aided_coh* out;        // [n_tasks] (device)
    gpsacq_peak* peaks_out;       // [n_tasks]
    unsigned long long* powers;   // [n_tasks][2 K + 1][2 F + 1][M][2 W + 1], or NULL
};
void launch_aided_coh_iq(const AidedCohIqArgs& a, hipStream_t s);

}  // namespace acq
