// snapq_iq_launch.hpp -- argument blocks and launchers of "Snapshot signal quality on an 8-bit IQ capture" of include/gpsacq.h:
// snapq_iq_kernels.hip's k_iq_energy (one wave64 per chunk of the capture), k_snap_floor (one wave64 per task) and
// k_snap_quality_iq (one lane per (fix, channel)).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "snapq_launch.hpp"

namespace acq {

static constexpr int SNAPQ_CHUNK = 1024;    // samples of a chunk of k_iq_energy: a power of two, a multiple of 512 (64 lanes x 8 samples)
static constexpr int SNAPQ_IQ_WAVES = 4;    // wave64s of a workgroup of k_iq_energy and k_snap_floor

// the capture and the sample's law, as IqCaptureArgs has them
struct SnapIqCapture {
    const uint8_t* iq;   // interleaved I, Q bytes (device), 16-byte aligned
    size_t n_samples;    // bytes at or beyond 2 * n_samples are not read
    uint32_t flip;       // 0x80808080 for GPSACQ_IQ_U8, 0 for GPSACQ_IQ_S8
    int32_t dc_i, dc_q;  // nearbyint of the mean where it is removed, else 0; |dc| <= 128
};

struct IqEnergyArgs {
    SnapIqCapture c;
    size_t n_chunks;     // n_samples / SNAPQ_CHUNK: whole chunks only
    uint64_t* energy;    // [n_chunks] (device): sum of v_i^2 + v_q^2 over chunk c
};
void launch_iq_energy(const IqEnergyArgs& a, hipStream_t s);

// which window a record has: block * (stride / 2) .. + segments * spm, where the record is one of this capture
struct SnapWindowArgs {
    const gpsacq_task* tasks;  // [n_tasks] (device), or NULL: task t = (block t, PRN t % 32)
    const gpsacq_fine* fine;   // [n_tasks] (device)
    size_t n_tasks;
    size_t n_samples;
    size_t stride;  // bytes between blocks
    int spm;
};

struct SnapFloorArgs {
    SnapIqCapture c;
    SnapWindowArgs w;
    const uint64_t* energy;  // k_iq_energy's; not read in sign mode
    size_t n_chunks;
    int sign;                // GPSACQ_SAMPLES_SIGN: floor = 2 * spm * segments, the capture is not read
    uint64_t* floor;         // [n_tasks] (device)
};
void launch_snap_floor(const SnapFloorArgs& a, hipStream_t s);

struct SnapQualityIqArgs {
    SnapWindowArgs w;
    const uint64_t* floor;  // [n_tasks] (device): k_snap_floor's
    double fs;
    gpsacq_snap_quality_params par;  // checked
    gpsacq_obs* obs;                 // [n_tasks] (device) in-out, or NULL
    gpsacq_quality_info* info;       // [n_tasks] (device)
};
void launch_snap_quality_iq(const SnapQualityIqArgs& a, hipStream_t s);

}  // namespace acq
