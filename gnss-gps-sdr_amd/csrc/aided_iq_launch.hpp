// aided_iq_launch.hpp -- argument block and launcher of "Aided acquisition on an 8-bit IQ capture" of include/gpsacq.h, multi-bit
// mode: aided_iq_kernels.hip's k_aided_iq (one workgroup per task).  Sign mode runs k_aided of aided_launch.hpp on the converted
// capture and needs nothing from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aided_launch.hpp"
#include "snapshot_iq_launch.hpp"

namespace acq {

static constexpr int AIDED_IQ_WAVES = 4;     // wave64s of a k_aided_iq workgroup; wave w takes segments w, w + 4, ...
static constexpr int AIDED_IQ_CHUNK = 1024;  // samples whose prefix sums a wave holds in LDS at a time (a multiple of 8)
static constexpr int AIDED_IQ_PAD = 256;     // slots in front of the prefix sums: 2 W <= 254 zeros and A[0]
static constexpr int AIDED_IQ_SLOTS = AIDED_IQ_PAD + AIDED_IQ_CHUNK + 256;  // A[k] sits in slot AIDED_IQ_PAD + k, k = -2 W .. n + 2 W - 1
static constexpr int AIDED_IQ_LIST = AIDED_IQ_CHUNK + 256;                  // transitions of a chunk's stream: at most n + 2 W - 1 <= 1277
static_assert(2 * AIDED_MAX_CODE_HALF <= AIDED_IQ_PAD - 2 && AIDED_IQ_CHUNK % 8 == 0 && AIDED_IQ_LIST % 4 == 0, "the pads");
static_assert(AIDED_IQ_CHUNK + 2 * AIDED_MAX_CODE_HALF < (1 << 15), "a list entry: 15 bits of position, one of sign");

// the prefix array of a k_aided_iq wave as aided_iq_walk.hpp's segment_sums_by_parts takes it
struct AidedIqGeometry {
    static constexpr int CHUNK = AIDED_IQ_CHUNK, PAD = AIDED_IQ_PAD;
};

struct AidedIqArgs {
    IqCaptureArgs c;
    int kmax;               // the grid is -kmax .. +kmax
    const gpsacq_aid* aid;  // [n_tasks] (device)
    gpsacq_aided_params p;
    gpsacq_aided* out;           // [n_tasks] (device)
    gpsacq_peak* peaks_out;      // [n_tasks]
    unsigned long long* powers;  // [n_tasks][2 K + 1][2 W + 1], or NULL
};
void launch_aided_iq(const AidedIqArgs& a, hipStream_t s);

}  // namespace acq
