// snapshot_iq_launch.hpp -- argument blocks and launchers of "Snapshot chain on an 8-bit IQ capture" of include/gpsacq.h, multi-bit
// mode: snapshot_iq_kernels.hip's k_refine_iq and k_fine_dop_iq (one workgroup per task each).  Sign mode runs the 1-bit kernels of
// refine_launch.hpp and doppler_launch.hpp on the converted capture and needs nothing from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "doppler_launch.hpp"
#include "refine_launch.hpp"

namespace acq {

static constexpr int SNAP_IQ_WAVES = 4;  // wave64s of a workgroup of either kernel; wave w takes segments w, w + 4, ...

// an 8-bit IQ capture as the snapshot kernels are told of it, ONCE (BitCaptureArgs of refine_launch.hpp is the 1-bit one): the
// capture, its tasks and peaks, the chip table, the engine's grid and the sample's law
struct IqCaptureArgs {
    const uint8_t* iq;   // interleaved I, Q bytes (device), 16-byte aligned
    size_t n_samples;    // bytes at or beyond 2 * n_samples are not read
    size_t stride;       // bytes between blocks, a multiple of 16
    const gpsacq_task* tasks;  // [n_tasks] (device), or NULL: task t = (block t, PRN t % 32)
    const gpsacq_peak* peaks;  // [n_tasks] (device); the aided searches' peaks_in, which may be NULL
    size_t n_tasks;
    const uint32_t* chips;  // [32][32] C/A chip words (device)
    double fs, step_hz;    // step_hz: the engine's Doppler grid step, 0 on the reference grid (lo_shift in FFT bins)
    double mix_hz, fc_lo;   // f = lo_dop - mix_hz + fc_lo: fc_lo is the engine's fc, 0 for GPSACQ_SAMPLES_COMPLEX
    int spm;                // samples per millisecond, <= 65535
    uint32_t flip;          // 0x80808080 for GPSACQ_IQ_U8 (byte ^ 0x80 read as int8 = byte - 128), 0 for GPSACQ_IQ_S8
    int32_t dc_i, dc_q;     // nearbyint of the mean where it is removed, else 0; |dc| <= 128
};

struct RefineIqArgs {
    IqCaptureArgs c;
    gpsacq_refine_params p;
    gpsacq_fine* out;  // [n_tasks] (device)
};
void launch_refine_iq(const RefineIqArgs& a, hipStream_t s);

struct FineDopIqArgs {
    IqCaptureArgs c;
    gpsacq_dopfine_params p;  // a window of at most DOP_MAX_SEGMENTS segments (checked by the host)
    gpsacq_dopfine* out;      // [n_tasks] (device)
};
void launch_fine_dop_iq(const FineDopIqArgs& a, hipStream_t s);

}  // namespace acq
