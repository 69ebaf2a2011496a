// gpsacq_engine.hpp -- what the translation units of libgpsacq.so that work on an engine share: the error helpers, the two owning
// types every kernel family builds on (Scratch<T>, a device buffer; Stages<N>, the events that time a chain of kernels), the
// engine itself, and the few internal functions that cross files.  Private to the library: not installed, nothing here is
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

// A device buffer that belongs to the engine: the pointer, its capacity in elements, and the hipFree when the engine goes.  Reads
// as the plain pointer wherever one is expected.  Null and empty until grown or allocated, and again after a failed attempt.
template <class T> struct Scratch {
    T* p = nullptr;
    size_t cap = 0;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
    operator T*() const { return p; }
    // Scratch grows on demand, stream-ordered (hipFreeAsync / hipMallocAsync on the engine's stream): work already enqueued keeps
    // the old buffer until it has run, and no device-wide synchronisation happens in mid-stream.  It grows by at least half so
    // that a caller creeping up in batch size does not reallocate every call.
    int grow(size_t need, hipStream_t stream, size_t elem_bytes = sizeof(T)) {
        if (need <= cap) return GPSACQ_OK;
        need = std::max(need, cap + cap / 2);
        if (p) HIPCHK(hipFreeAsync(p, stream));
        p = nullptr;
        cap = 0;
        HIPCHK(hipMallocAsync((void**)&p, need * elem_bytes, stream));
        cap = need;
        return GPSACQ_OK;
    }
    // the tables that are allocated once (or rarely): exactly n elements, device-synchronous
    hipError_t alloc(size_t n) {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t he = hipMalloc((void**)&p, n * sizeof(T));
        if (he == hipSuccess) cap = n;
        return he;
    }
    void swap(Scratch& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};

// The events around the stages of one chain of kernels: ev[k - 1] .. ev[k] bracket stage k.  `done` says that the last chain was
// enqueued whole; a chain that failed half way leaves it false, and its *_last_ms then reports that nothing ran.
template <int N> struct Stages {
    hipEvent_t ev[N] = {};
    bool done = false;
    Stages() = default;
    Stages(const Stages&) = delete;
    Stages& operator=(const Stages&) = delete;
    ~Stages() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    int begin(hipStream_t stream) {
        for (hipEvent_t& x : ev)
            if (!x) HIPCHK(hipEventCreate(&x));
        done = false;
        return mark(0, stream);
    }
    int mark(int k, hipStream_t stream) {
        HIPCHK(hipEventRecord(ev[k], stream));
        return GPSACQ_OK;
    }
    int finish() {
        HIPCHK(hipGetLastError());
        done = true;
        return GPSACQ_OK;
    }
    bool ran() const { return done; }
    int wait() const {
        HIPCHK(hipEventSynchronize(ev[N - 1]));
        return GPSACQ_OK;
    }
    // the time between two events into *ms; a null ms is accepted
    int elapsed(int from, int to, float* ms) const {
        if (ms) HIPCHK(hipEventElapsedTime(ms, ev[from], ev[to]));
        return GPSACQ_OK;
    }
};

struct gpsacq_engine {
    gpsacq_params p{};
    int dmax = 0, ndop = 0, dop_first = 0, nlags = 0, mc = 0, halo = 0, crow = 0;  // searched bins: dop_first .. +ndop-1
    int n_acc = 1, acc_step = 0;  // non-coherent accumulation (gpsacq_set_noncoherent)
    // Doppler grid (gpsacq_set_doppler_step): step = bin * dstride / sub, points -kmax..+kmax; sub = dstride = 1 is the reference's
    int sub = 1, dstride = 1, kmax = 0;
    Scratch<acq::cf> d_lutc;  // [sub][8][256] look-up tables of k_fwd2
    bool creep_comp = false;      // re-align accumulated blocks by the code creep of each Doppler bin
    bool block_align = false;     // re-align accumulated blocks by the code phase between their starts (any stride)
    int cus = 0;
    char name[64] = {0};
    hipStream_t stream = nullptr;
    // stage events of the last kTimingRing searches (asynchronous callers read a finished search's times while the next one
    // runs): all created with the engine, `done` unused
    static const int kTimingRing = 8;
    Stages<4> ring[kTimingRing];
    int ring_launches[kTimingRing] = {};
    int64_t ring_cells[kTimingRing] = {};
    long searches = 0;  // searches enqueued so far; search k uses ring slot k % kTimingRing
    // constants
    Scratch<acq::cf> d_t1, d_t2, d_bq, d_tn;
    Scratch<acq::cf> d_fold;  // the folded-rotation tables of k_corr<..., FOLD> (acq_tables.hpp TablesFold)
    Scratch<unsigned char> d_rho;
    Scratch<uint8_t> d_cos, d_sin;
    Scratch<uint64_t> d_cos_t, d_sin_t;  // bit-transposed masks for k_fwd
    Scratch<acq::cf> d_code;             // [32 + d_patch_blocks.cap][8][crow]
    Scratch<int32_t> d_patch_blocks;     // its capacity is the number of patched code slots behind the 32 of d_code
    // scratch (grown on demand)
    Scratch<uint8_t> d_bits;
    Scratch<acq::cf> d_dpp;  // capacity in blocks
    Scratch<acq::Task> d_tasks;
    Scratch<acq::Cell> d_cells;
    Scratch<acq::Cell> d_parts;  // partial cells of multi-pass searches (more than 10000 lags)
    Scratch<acq::Peak> d_peaks;
    // 8-bit IQ ingestion scratch
    Scratch<uint8_t> d_iq;
    Scratch<uint8_t> d_iqbits;
    Scratch<float> d_pdump;  // non-coherent + creep re-alignment at fs > 10 MHz: per-lag power sums, [cell][nlags]
    Scratch<float> d_fsamp;  // multi-bit path: the batch's samples as complex floats, LO applied ([block][40000][2])
    Scratch<unsigned long long> d_sums;
    // capture generator scratch
    Scratch<acq::GenSat> d_sats;
    Scratch<uint8_t> d_gen;
    Scratch<int8_t> d_nav;  // navigation bits of gpsacq_generate_nav_range
    // tracking channels (gpsacq_track*)
    Scratch<uint32_t> d_track_chips;  // [32][32] C/A chips
    Scratch<gpsacq_track_chan> d_chans;
    Scratch<int32_t> d_track_n;
    Scratch<int32_t> d_prompt;
    Scratch<gpsacq_track_record> d_records;
    Stages<3> tiq_t;  // gpsacq_track_iq8*: before the conversion, between it and the channels, after them
    // navigation solver (gpsacq_sat_states*, gpsacq_fix_batch*)
    Scratch<acq::NavEph> d_nav_eph;          // the call's ephemeris table
    Scratch<gpsacq_obs> d_nav_obs;           // host-buffer forms: observations and results
    Scratch<gpsacq_sat_state> d_nav_state;  // k_sat_state's output, k_fix's input
    Scratch<gpsacq_fix> d_nav_fix;
    Stages<3> nav_t;  // gpsacq_fix_batch*: before k_sat_state, between the kernels, after k_fix
    // observables (gpsacq_observables*, gpsacq_fix_track_device)
    Scratch<acq::ObsChan> d_obs_chan;        // the call's channels as the kernels read them
    Scratch<uint64_t> d_obs_pos;             // k_code_pos's output, k_observe's input: [n_chans][max_epochs]
    Scratch<gpsacq_track_record> d_obs_rec;  // host-buffer form: the records
    Stages<3> obs_t;  // before k_code_pos, between the kernels, after k_observe
    // carrier observables and velocity (gpsacq_rate_observables*, gpsacq_vel_batch*, gpsacq_pvt_track_device)
    Scratch<acq::RateChan> d_rate_chan;
    Scratch<int64_t> d_rate_acc;          // k_carrier_acc's output, k_observe_rate's input: [n_chans][max_epochs + 1]
    Scratch<gpsacq_rate_obs> d_rate_obs;  // host-buffer forms and gpsacq_pvt_track_device's scratch
    Scratch<gpsacq_sat_rate> d_sat_rate;  // k_sat_state_rate's output
    Scratch<gpsacq_vel> d_vel;
    Stages<3> rate_t;  // before k_carrier_acc, between the kernels, after k_observe_rate
    Stages<3> vel_t;   // before k_sat_state_rate, between it and k_vel, after k_vel
    // atmosphere-corrected fixes (gpsacq_sat_views*, gpsacq_fix_atm_batch*)
    Scratch<gpsacq_fix_dop> d_atm_dop;    // host-buffer form, and where the caller wants no DOP
    Scratch<gpsacq_sat_view> d_atm_view;  // host-buffer forms
    Stages<4> atm_t;  // before k_sat_state, between it and k_fix_atm, after k_fix_atm, after k_sat_view
    bool atm_views = false;
    // fix integrity (gpsacq_fix_raim_batch*)
    Scratch<acq::RaimRow> d_raim_rows;  // k_raim_detect's hand-over to k_raim_exclude: [n_fix]
    Scratch<gpsacq_fix_raim> d_raim;    // host-buffer form
    Stages<4> raim_t;  // before k_sat_state, between it and k_raim_detect, after k_raim_detect, after k_raim_exclude
    // carrier-smoothed observables (gpsacq_smooth_observables*, gpsacq_fix_smooth_track_device)
    Scratch<acq::SmoothChan> d_smooth_chan;
    Scratch<int64_t> d_smooth_lock;  // k_lock_acc's two outputs: [2][n_chans][max_epochs + 1]
    Scratch<uint64_t> d_smooth_q;    // channel-major 64-bit rows: Z and P [n_chans][n_fix] each, then S [n_chans][n_fix + 1]
    Scratch<int32_t> d_smooth_w;     // channel-major 32-bit rows, [n_chans][n_fix] each: t, the state, s_i
    Scratch<gpsacq_smooth_info> d_smooth_info;  // host-buffer form
    Stages<5> smooth_t;  // before k_lock_acc, then after each of k_lock_acc, k_cmc, k_smooth_scan, k_smooth_out
    // signal quality (gpsacq_quality_observables*, gpsacq_fix_quality_track_device)
    Scratch<acq::QualityChan> d_quality_chan;
    Scratch<uint64_t> d_quality_sums;              // k_quality_acc's three outputs: [3][n_chans][max_epochs + 1]
    Scratch<gpsacq_quality_info> d_quality_info;  // host-buffer form, and where the caller of the chain wants no info
    Stages<3> quality_t;  // before k_quality_acc, between the kernels, after k_quality_out
    // coarse-time fixes (gpsacq_coarse_obs*, gpsacq_coarse_fix_batch*, gpsacq_coarse_fix_peaks_device)
    Scratch<gpsacq_peak> d_coarse_peaks;  // host-buffer form of gpsacq_coarse_obs
    Scratch<gpsacq_obs> d_coarse_obs;     // k_coarse_obs's output where the caller of the chain wants no observations
    Scratch<gpsacq_obs> d_coarse_work;    // k_coarse_fix's whole milliseconds where the caller wants no obs_out, and the host-buffer form
    Scratch<gpsacq_coarse_prior> d_coarse_prior;  // host-buffer form
    Scratch<gpsacq_coarse_info> d_coarse_info;    // host-buffer form
    Stages<2> coarse_obs_t, coarse_fix_t;  // around k_coarse_obs, around k_coarse_fix
    // coarse-time fix integrity (gpsacq_coarse_raim_batch*); the host-buffer form stages as gpsacq_coarse_fix_batch does, the raim
    // records in d_raim
    Scratch<gpsacq_obs> d_coarse_cand;  // k_coarse_exclude's candidates, a work row each: [n_fix][sats][sats]
    Stages<3> coarse_raim_t;  // before k_coarse_fix, between it and k_coarse_exclude, after k_coarse_exclude
    // fine code phases (gpsacq_refine*, gpsacq_coarse_obs_fine*, gpsacq_coarse_fix_fine_device)
    Scratch<uint8_t> d_refine_bits;  // host-buffer form of gpsacq_refine: the capture, its tasks and peaks
    Scratch<gpsacq_task> d_refine_tasks;
    Scratch<gpsacq_peak> d_refine_peaks;  // also the peaks of the host-buffer form of gpsacq_coarse_obs_fine
    Scratch<gpsacq_fine> d_fine;  // host-buffer forms, and k_refine's output where the caller of the chain wants no records
    Stages<2> refine_t, refine_obs_t;  // around k_refine, around k_coarse_obs_fine
    // snapshot signal quality (gpsacq_snap_quality*, gpsacq_coarse_fix_quality_device); the host-buffer form stages its records in
    // d_fine and its observations in d_coarse_obs
    Scratch<gpsacq_quality_info> d_snapq_info;  // host-buffer form, and where the caller of the chain wants no info
    Stages<2> snapq_t;                          // around k_snap_quality
    // cold snapshot fixes (gpsacq_fine_doppler*, gpsacq_rate_obs_fine*, gpsacq_doppler_fix_batch*, gpsacq_cold_fix_device); the
    // host-buffer forms stage the capture, tasks and peaks in the d_refine_* buffers above and the observations in d_nav_obs / d_rate_obs
    Scratch<gpsacq_dopfine> d_dopfine;  // host-buffer forms, and k_fine_dop's output where the caller of the chain wants no records
    Scratch<double> d_dop_tau;          // k_doppler_fix's light times between its passes: [n_fix][sats]
    Scratch<int32_t> d_dop_rx_ms;       // host-buffer form
    Scratch<gpsacq_doppler_fix> d_dop_fix;     // host-buffer form
    Scratch<gpsacq_coarse_prior> d_dop_prior;  // host-buffer form, and the chain's priors where the caller wants none
    Stages<2> dop_fine_t, dop_obs_t, dop_fix_t;  // around k_fine_dop, k_rate_obs_fine, k_doppler_fix
    // snapshot chain on an 8-bit IQ capture (gpsacq_refine_iq8*, gpsacq_fine_doppler_iq8*, the two *_iq8_device chains): the capture
    // of the host-buffer forms goes into d_iq, sign mode's 1-bit stream into d_iqbits, tasks, peaks and records as the 1-bit forms'
    Stages<2> snapiq_conv_t, snapiq_refine_t, snapiq_dop_t;  // around the conversion, the fine-record kernel, the fine-Doppler kernel
    // aided acquisition (gpsacq_aid_predict*, gpsacq_aided_search*, gpsacq_aided_peaks_device); the host-buffer forms stage fixes and
    // velocities in d_nav_fix / d_vel and the capture, tasks and input peaks in the d_refine_* buffers above
    Scratch<gpsacq_aid> d_aid;  // host-buffer forms, and k_aid_predict's output where the caller of the chain wants no records
    Scratch<gpsacq_aided> d_aided;       // host-buffer form
    Scratch<gpsacq_peak> d_aided_peaks;  // host-buffer form: the output peaks
    Scratch<unsigned long long> d_aided_powers;  // host-buffer form: [n_tasks][2 K + 1][2 W + 1]
    Stages<2> aid_predict_t, aided_t;  // around k_aid_predict, around k_aided
    // aided acquisition on an 8-bit IQ capture (gpsacq_aided_search_iq8*, gpsacq_aided_peaks_iq8_device): the capture of the
    // host-buffer form goes into d_iq, sign mode's 1-bit stream into d_iqbits, everything else as the 1-bit forms'
    Stages<2> aidiq_conv_t, aidiq_predict_t, aidiq_search_t;  // around the conversion, k_aid_predict, k_aided_iq (sign mode: k_aided)
    // coherent aided acquisition (gpsacq_aided_coh_search*, gpsacq_aid_instant*, gpsacq_aided_coh_peaks_device); the host-buffer forms
    // stage as the aided ones do, the coarse-time records in d_coarse_info / d_coarse_prior
    Scratch<int16_t> d_coh_table;            // the rotation table, C then S, made once
    Scratch<gpsacq_aided_coh> d_aided_coh;   // host-buffer form
    Scratch<unsigned long long> d_coh_powers;  // host-buffer form: [n_tasks][2 K + 1][2 F + 1][M][2 W + 1]
    Scratch<gpsacq_fix> d_fix_instant;       // k_aid_instant's output: host-buffer form, and where the caller of the chain wants no fixes
    Stages<4> aided_coh_t;  // before k_aid_instant, between it and k_aid_predict, between that and k_aided_coh, after it
    int aided_coh_ran = 0;  // bit k: stage k + 1 ran a kernel in the last call
    // coherent aided acquisition on an 8-bit IQ capture (gpsacq_aided_coh_search_iq8*, gpsacq_aided_coh_peaks_iq8_device): the capture
    // of the host-buffer form goes into d_iq, sign mode's 1-bit stream into d_iqbits, everything else as the 1-bit forms'
    Stages<2> aidcohiq_conv_t;  // around the conversion (sign mode)
    Stages<4> aidcohiq_t;       // as aided_coh_t, the search being k_aided_coh_iq (sign mode: k_aided_coh)
    int aidcohiq_ran = 0;       // bit k: stage k + 1 ran a kernel in the last call
    // snapshot signal quality on an 8-bit IQ capture (gpsacq_snap_floor_iq8*, gpsacq_snap_quality_iq8*,
    // gpsacq_coarse_fix_quality_iq8_device): the capture of the host-buffer forms goes into d_iq, tasks, records, observations and
    // info as the 1-bit forms'
    Scratch<uint64_t> d_chunk_energy;  // k_iq_energy's E: one entry per whole chunk of the capture
    Scratch<uint64_t> d_snap_floor;    // host-buffer forms, and k_snap_floor's output where the caller wants no floors
    Stages<2> snapqiq_floor_t, snapqiq_quality_t;  // around k_iq_energy and k_snap_floor, around k_snap_quality_iq (sign mode: k_snap_quality)
    // k_corr<..., PERSIST>: the hand-out state of a launch (9 counters 64 bytes apart, then [8][slots] task slots), zeroed before it
    Scratch<int> d_persist;
    bool persist = false;
    // cached default schedule (task t = block t, PRN t % 32; with ref_quirks also its patch list: blocks 0, 32, 64, ...)
    size_t sched_tasks = 0;
    bool sched_valid = false;
    // pipelined host-buffer searches (gpsacq_pipe_*): a second stream for the uploads, per-slot pinned staging and device buffers
    hipStream_t copy_stream = nullptr;
    struct PipeSlot {
        uint8_t* h_in = nullptr;  // pinned
        size_t h_bytes = 0;
        Scratch<uint8_t> d_in;
        Scratch<acq::Peak> d_peaks;      // its capacity is the most blocks a batch of this slot can hold
        acq::Peak* h_peaks = nullptr;  // pinned
        hipEvent_t uploaded = nullptr, done = nullptr;
        bool busy = false;
        size_t n_tasks = 0;
        ~PipeSlot() {
            if (uploaded) (void)hipEventDestroy(uploaded);
            if (done) (void)hipEventDestroy(done);
        }
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

// gpsacq_engine.cpp
int iq8_capture(const gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t stride, Capture* out);
int iq8_to_bits_enqueue(gpsacq_engine* e, const uint8_t* d_iq, size_t n_samples, const acq::IqConv& conv, size_t first_sample, uint8_t* d_bits);
// gpsacq_track.cpp
int ensure_track_chips(gpsacq_engine* e);
