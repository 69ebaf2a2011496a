// gpsacq_engine.hpp -- what the translation units of libgpsacq.so that work on an engine share: the engine itself, the error and
// scratch helpers, and the few internal functions that cross files.  Private to the library: not installed, nothing here is
// exported (the library is built with hidden visibility), and no layout in it is part of the ABI of include/gpsacq.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpsacq.h"
#include "acq_launch.hpp"
#include "gen_launch.hpp"
#include "nav_launch.hpp"
#include "obs_launch.hpp"
#include "quality_launch.hpp"
#include "raim_launch.hpp"
#include "smooth_launch.hpp"

// sets this thread's gpsacq_last_error() text from a printf format and returns `code` (gpsacq_engine.cpp)
int fail(int code, const char* fmt, ...);
#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? GPSACQ_ERR_NOMEM : GPSACQ_ERR_DEVICE, \
                                          "%s: %s", #expr, hipGetErrorString(e_));                    \
    } while (0)

struct gpsacq_engine {
    gpsacq_params p{};
    int dmax = 0, ndop = 0, dop_first = 0, nlags = 0, mc = 0, halo = 0, crow = 0;  // searched bins: dop_first .. +ndop-1
    int n_acc = 1, acc_step = 0;  // non-coherent accumulation (gpsacq_set_noncoherent)
    // Doppler grid (gpsacq_set_doppler_step): step = bin * dstride / sub, points -kmax..+kmax; sub = dstride = 1 is the reference's
    int sub = 1, dstride = 1, kmax = 0;
    acq::cf* d_lutc = nullptr;  // [sub][8][256] look-up tables of k_fwd2
    bool creep_comp = false;      // re-align accumulated blocks by the code creep of each Doppler bin
    bool block_align = false;     // re-align accumulated blocks by the code phase between their starts (any stride)
    int cus = 0;
    char name[64] = {0};
    hipStream_t stream = nullptr;
    // stage events of the last kTimingRing searches (asynchronous callers read a finished search's
    // times while the next one runs)
    static const int kTimingRing = 8;
    hipEvent_t ev[kTimingRing][4] = {};
    int ring_launches[kTimingRing] = {};
    int64_t ring_cells[kTimingRing] = {};
    long searches = 0;  // searches enqueued so far; search k uses ring slot k % kTimingRing
    // constants
    acq::cf *d_t1 = nullptr, *d_t2 = nullptr, *d_bq = nullptr, *d_tn = nullptr;
    acq::cf* d_fold = nullptr;  // the folded-rotation tables of k_corr<..., FOLD> (acq_tables.hpp TablesFold)
    unsigned char* d_rho = nullptr;
    uint8_t *d_cos = nullptr, *d_sin = nullptr;
    uint64_t *d_cos_t = nullptr, *d_sin_t = nullptr;  // bit-transposed masks for k_fwd
    acq::cf* d_code = nullptr;  // [32 + patch_cap][8][crow]
    size_t patch_cap = 0;
    int32_t* d_patch_blocks = nullptr;
    // scratch (grown on demand)
    uint8_t* d_bits = nullptr;
    size_t bits_cap = 0;
    acq::cf* d_dpp = nullptr;
    size_t dpp_cap = 0;  // in blocks
    acq::Task* d_tasks = nullptr;
    acq::Cell* d_cells = nullptr;
    acq::Cell* d_parts = nullptr;  // partial cells of multi-pass searches (more than 10000 lags)
    acq::Peak* d_peaks = nullptr;
    size_t task_cap = 0, cell_cap = 0, peak_cap = 0, parts_cap = 0;
    // 8-bit IQ ingestion scratch
    uint8_t* d_iq = nullptr;
    size_t iq_cap = 0;
    uint8_t* d_iqbits = nullptr;
    size_t iqbits_cap = 0;
    float* d_pdump = nullptr;  // non-coherent + creep re-alignment at fs > 10 MHz: per-lag power sums, [cell][nlags]
    size_t pdump_cap = 0;
    float* d_fsamp = nullptr;  // multi-bit path: the batch's samples as complex floats, LO applied ([block][40000][2])
    size_t fsamp_cap = 0;
    unsigned long long* d_sums = nullptr;
    // capture generator scratch
    acq::GenSat* d_sats = nullptr;
    size_t sats_cap = 0;
    uint8_t* d_gen = nullptr;
    size_t gen_cap = 0;
    int8_t* d_nav = nullptr;  // navigation bits of gpsacq_generate_nav_range
    size_t nav_cap = 0;
    // tracking channels (gpsacq_track*)
    uint32_t* d_track_chips = nullptr;  // [32][32] C/A chips
    gpsacq_track_chan* d_chans = nullptr;
    size_t chans_cap = 0;
    int32_t* d_track_n = nullptr;
    size_t track_n_cap = 0;
    int32_t* d_prompt = nullptr;
    size_t prompt_cap = 0;
    gpsacq_track_record* d_records = nullptr;
    size_t records_cap = 0;
    hipEvent_t tiq_ev[3] = {};  // gpsacq_track_iq8*: before the conversion, between it and the channels, after them
    bool tiq_timed = false;
    // navigation solver (gpsacq_sat_states*, gpsacq_fix_batch*)
    acq::NavEph* d_nav_eph = nullptr;  // the call's ephemeris table
    size_t nav_eph_cap = 0;
    gpsacq_obs* d_nav_obs = nullptr;  // host-buffer forms: observations and results
    size_t nav_obs_cap = 0;
    gpsacq_sat_state* d_nav_state = nullptr;  // k_sat_state's output, k_fix's input
    size_t nav_state_cap = 0;
    gpsacq_fix* d_nav_fix = nullptr;
    size_t nav_fix_cap = 0;
    hipEvent_t nav_ev[3] = {};  // gpsacq_fix_batch*: before k_sat_state, between the kernels, after k_fix
    bool nav_timed = false;
    // observables (gpsacq_observables*, gpsacq_fix_track_device)
    acq::ObsChan* d_obs_chan = nullptr;  // the call's channels as the kernels read them
    size_t obs_chan_cap = 0;
    uint64_t* d_obs_pos = nullptr;  // k_code_pos's output, k_observe's input: [n_chans][max_epochs]
    size_t obs_pos_cap = 0;
    gpsacq_track_record* d_obs_rec = nullptr;  // host-buffer form: the records
    size_t obs_rec_cap = 0;
    hipEvent_t obs_ev[3] = {};  // before k_code_pos, between the kernels, after k_observe
    bool obs_timed = false;
    // carrier observables and velocity (gpsacq_rate_observables*, gpsacq_vel_batch*, gpsacq_pvt_track_device)
    acq::RateChan* d_rate_chan = nullptr;
    size_t rate_chan_cap = 0;
    int64_t* d_rate_acc = nullptr;  // k_carrier_acc's output, k_observe_rate's input: [n_chans][max_epochs + 1]
    size_t rate_acc_cap = 0;
    gpsacq_rate_obs* d_rate_obs = nullptr;  // host-buffer forms and gpsacq_pvt_track_device's scratch
    size_t rate_obs_cap = 0;
    gpsacq_sat_rate* d_sat_rate = nullptr;  // k_sat_state_rate's output
    size_t sat_rate_cap = 0;
    gpsacq_vel* d_vel = nullptr;
    size_t vel_cap = 0;
    hipEvent_t rate_ev[3] = {};  // before k_carrier_acc, between the kernels, after k_observe_rate
    hipEvent_t vel_ev[3] = {};   // before k_sat_state_rate, between it and k_vel, after k_vel
    bool rate_timed = false, vel_timed = false;
    // atmosphere-corrected fixes (gpsacq_sat_views*, gpsacq_fix_atm_batch*)
    gpsacq_fix_dop* d_atm_dop = nullptr;  // host-buffer form, and where the caller wants no DOP
    size_t atm_dop_cap = 0;
    gpsacq_sat_view* d_atm_view = nullptr;  // host-buffer forms
    size_t atm_view_cap = 0;
    hipEvent_t atm_ev[4] = {};  // before k_sat_state, between it and k_fix_atm, after k_fix_atm, after k_sat_view
    bool atm_timed = false, atm_views = false;
    // fix integrity (gpsacq_fix_raim_batch*)
    acq::RaimRow* d_raim_rows = nullptr;  // k_raim_detect's hand-over to k_raim_exclude: [n_fix]
    size_t raim_rows_cap = 0;
    gpsacq_fix_raim* d_raim = nullptr;  // host-buffer form
    size_t raim_cap = 0;
    hipEvent_t raim_ev[4] = {};  // before k_sat_state, between it and k_raim_detect, after k_raim_detect, after k_raim_exclude
    bool raim_timed = false;
    // carrier-smoothed observables (gpsacq_smooth_observables*, gpsacq_fix_smooth_track_device)
    acq::SmoothChan* d_smooth_chan = nullptr;
    size_t smooth_chan_cap = 0;
    int64_t* d_smooth_lock = nullptr;  // k_lock_acc's two outputs: [2][n_chans][max_epochs + 1]
    size_t smooth_lock_cap = 0;
    uint64_t* d_smooth_q = nullptr;  // channel-major 64-bit rows: Z and P [n_chans][n_fix] each, then S [n_chans][n_fix + 1]
    size_t smooth_q_cap = 0;
    int32_t* d_smooth_w = nullptr;  // channel-major 32-bit rows, [n_chans][n_fix] each: t, the state, s_i
    size_t smooth_w_cap = 0;
    gpsacq_smooth_info* d_smooth_info = nullptr;  // host-buffer form
    size_t smooth_info_cap = 0;
    hipEvent_t smooth_ev[5] = {};  // before k_lock_acc, then after each of k_lock_acc, k_cmc, k_smooth_scan, k_smooth_out
    bool smooth_timed = false;
    // signal quality (gpsacq_quality_observables*, gpsacq_fix_quality_track_device)
    acq::QualityChan* d_quality_chan = nullptr;
    size_t quality_chan_cap = 0;
    uint64_t* d_quality_sums = nullptr;  // k_quality_acc's three outputs: [3][n_chans][max_epochs + 1]
    size_t quality_sums_cap = 0;
    gpsacq_quality_info* d_quality_info = nullptr;  // host-buffer form, and where the caller of the chain wants no info
    size_t quality_info_cap = 0;
    hipEvent_t quality_ev[3] = {};  // before k_quality_acc, between the kernels, after k_quality_out
    bool quality_timed = false;
    // coarse-time fixes (gpsacq_coarse_obs*, gpsacq_coarse_fix_batch*, gpsacq_coarse_fix_peaks_device)
    gpsacq_peak* d_coarse_peaks = nullptr;  // host-buffer form of gpsacq_coarse_obs
    size_t coarse_peaks_cap = 0;
    gpsacq_obs* d_coarse_obs = nullptr;  // k_coarse_obs's output where the caller of the chain wants no observations
    size_t coarse_obs_cap = 0;
    gpsacq_obs* d_coarse_work = nullptr;  // k_coarse_fix's whole milliseconds where the caller wants no obs_out, and the host-buffer form
    size_t coarse_work_cap = 0;
    gpsacq_coarse_prior* d_coarse_prior = nullptr;  // host-buffer form
    size_t coarse_prior_cap = 0;
    gpsacq_coarse_info* d_coarse_info = nullptr;  // host-buffer form
    size_t coarse_info_cap = 0;
    hipEvent_t coarse_ev[4] = {};  // before and after k_coarse_obs, before and after k_coarse_fix
    bool coarse_obs_timed = false, coarse_fix_timed = false;
    // fine code phases (gpsacq_refine*, gpsacq_coarse_obs_fine*, gpsacq_coarse_fix_fine_device)
    uint8_t* d_refine_bits = nullptr;  // host-buffer form of gpsacq_refine: the capture, its tasks and peaks
    size_t refine_bits_cap = 0;
    gpsacq_task* d_refine_tasks = nullptr;
    size_t refine_tasks_cap = 0;
    gpsacq_peak* d_refine_peaks = nullptr;  // also the peaks of the host-buffer form of gpsacq_coarse_obs_fine
    size_t refine_peaks_cap = 0;
    gpsacq_fine* d_fine = nullptr;  // host-buffer forms, and k_refine's output where the caller of the chain wants no records
    size_t fine_cap = 0;
    hipEvent_t refine_ev[4] = {};  // before and after k_refine, before and after k_coarse_obs_fine
    bool refine_timed = false, refine_obs_timed = false;
    // cold snapshot fixes (gpsacq_fine_doppler*, gpsacq_rate_obs_fine*, gpsacq_doppler_fix_batch*, gpsacq_cold_fix_device); the
    // host-buffer forms stage the capture, tasks and peaks in the d_refine_* buffers above and the observations in d_nav_obs / d_rate_obs
    gpsacq_dopfine* d_dopfine = nullptr;  // host-buffer forms, and k_fine_dop's output where the caller of the chain wants no records
    size_t dopfine_cap = 0;
    double* d_dop_tau = nullptr;  // k_doppler_fix's light times between its passes: [n_fix][sats]
    size_t dop_tau_cap = 0;
    int32_t* d_dop_rx_ms = nullptr;  // host-buffer form
    size_t dop_rx_ms_cap = 0;
    gpsacq_doppler_fix* d_dop_fix = nullptr;  // host-buffer form
    size_t dop_fix_cap = 0;
    gpsacq_coarse_prior* d_dop_prior = nullptr;  // host-buffer form, and the chain's priors where the caller wants none
    size_t dop_prior_cap = 0;
    hipEvent_t dop_ev[6] = {};  // before and after k_fine_dop, k_rate_obs_fine, k_doppler_fix
    bool dop_fine_timed = false, dop_obs_timed = false, dop_fix_timed = false;
    // k_corr<..., PERSIST>: the hand-out state of a launch (9 counters 64 bytes apart, then [8][slots] task slots), zeroed before it
    int* d_persist = nullptr;
    size_t persist_cap = 0;
    bool persist = false;
    // cached default schedule (task t = block t, PRN t % 32; with ref_quirks also its patch list: blocks 0, 32, 64, ...)
    size_t sched_tasks = 0;
    bool sched_valid = false;
    // pipelined host-buffer searches (gpsacq_pipe_*): a second stream for the uploads, per-slot pinned staging and device buffers
    hipStream_t copy_stream = nullptr;
    struct PipeSlot {
        uint8_t* h_in = nullptr;   // pinned
        size_t h_cap = 0;
        uint8_t* d_in = nullptr;
        size_t d_cap = 0;
        acq::Peak* d_peaks = nullptr;
        acq::Peak* h_peaks = nullptr;   // pinned
        size_t peak_cap = 0;
        hipEvent_t uploaded = nullptr, done = nullptr;
        bool busy = false;
        size_t n_tasks = 0;
    } pipe[GPSACQ_PIPE_SLOTS];
};

// what a search transforms: the 1-bit stream gps_test reads, or an 8-bit IQ capture converted while it is staged
struct Capture {
    bool iq8 = false;
    const uint8_t* d_src = nullptr;  // device pointer
    size_t stride = 0;               // bytes per block in d_src
    acq::IqConv iq{};
    size_t iq_first = 0, iq_total = ~(size_t)0;
    int multibit = 0;  // 8-bit IQ kept at full amplitude (float samples) instead of its sign: 1 the real-IF value, 2 the complex sample
};

// Scratch buffers grow on demand, stream-ordered (hipFreeAsync / hipMallocAsync on the engine's stream): work already
// enqueued keeps the old buffer until it has run, and no device-wide synchronisation happens in mid-stream.  They grow by at
// least half so that a caller creeping up in batch size does not reallocate every call.
template <class T> static int grow(T*& p, size_t& cap, size_t need, hipStream_t stream, size_t elem_bytes = sizeof(T)) {
    if (need <= cap) return GPSACQ_OK;
    need = std::max(need, cap + cap / 2);
    if (p) HIPCHK(hipFreeAsync(p, stream));
    p = nullptr;
    cap = 0;
    HIPCHK(hipMallocAsync((void**)&p, need * elem_bytes, stream));
    cap = need;
    return GPSACQ_OK;
}

// gpsacq_engine.cpp
int iq8_capture(const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t stride, Capture* out);
int iq8_to_bits_enqueue(gpsacq_engine* e, const uint8_t* d_iq, size_t n_samples, const acq::IqConv& conv, size_t first_sample, uint8_t* d_bits);
// gpsacq_track.cpp
int ensure_track_chips(gpsacq_engine* e);
