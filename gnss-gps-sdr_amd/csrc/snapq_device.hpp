// snapq_device.hpp -- steps 2 (sig, noise) to 7 of "Snapshot signal quality" of include/gpsacq.h, once: the info record of a fine
// record from its prompt power and a noise floor.  snapq_kernels.hip's k_snap_quality calls it with the analytic floor of a +-1
// stream, snapq_iq_kernels.hip's k_snap_quality_iq with the measured floor of "Snapshot signal quality on an 8-bit IQ capture".
// Integers up to the conversions of sig and floor; then two divisions, one product, one log10, one more division.  Both files are
// built with -ffp-contract=off: every step is one IEEE operation, so lin and weight are the reference's to the bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "refine_launch.hpp"  // FINE_UNUSABLE, step 1's mask

namespace acq {

// record == false is step 1, NO RECORD: the flag and zeros.  floor == 0 (only a measured floor can be: an all-zero window) is
// GPSACQ_QUALITY_NO_POWER with sig = 0.
__device__ __forceinline__ gpsacq_quality_info snap_quality_info(const gpsacq_fine& r, bool record, uint64_t floor, int spm, double fs,
                                                                 const gpsacq_snap_quality_params& par) {
    gpsacq_quality_info f;
    f.epochs = 0;
    f.flags = GPSACQ_QUALITY_NO_RECORD;
    f.sig = f.noise = 0;
    f.lin = f.cn0_dbhz = f.weight = 0.0;
    if (record) {
        const uint64_t sig = floor != 0 && r.prompt > floor ? r.prompt - floor : 0;
        int32_t flags = r.segments < par.min_segments ? GPSACQ_QUALITY_SHORT : 0;
        double lin = 0.0, db = 0.0;
        if (sig == 0) {
            flags |= GPSACQ_QUALITY_NO_POWER;
        } else {
            const double snr = (double)sig / (double)floor;
            lin = snr * (fs / (double)spm);
            db = 10.0 * log10(lin);
        }
        double weight = 0.0;
        const bool gated = (flags & (GPSACQ_QUALITY_NO_POWER | GPSACQ_QUALITY_SHORT)) != 0 || lin < par.cn0_min_lin;
        if (!gated) {
            const double w = lin / par.cn0_ref_lin;
            weight = w < 1.0 ? w : 1.0;
        }
        f.epochs = r.segments;
        f.flags = flags;
        f.sig = sig;
        f.noise = floor;
        f.lin = lin;
        f.cn0_dbhz = db;
        f.weight = weight;
    }
    return f;
}

}  // namespace acq
