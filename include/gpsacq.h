/*
 * gpsacq.h -- C ABI of the MI355X (gfx950) GPS L1 C/A acquisition engine.
 *
 * This is the drop-in boundary for the hot path of the reference's offline search stage
 * (JiaoXianjun/GNSS-GPS-SDR, c/search_offline.cpp).  Plain C: opaque handle, plain pointers
 * and sizes, int status codes (0 = ok), caller-allocated outputs, no exceptions cross it.
 * The reference has no FFI (it is one C++ translation unit); what a maintainer would bind is
 * the set of functions declared in c/gps_offline.h:87-91, and each entry point below names
 * the reference function whose work it performs:
 *
 *   gpsacq_create            SearchInit()            c/search_offline.cpp:74-110
 *                            (+ the globals FC, FS, max_fo of c/gps_offline.h:23-25)
 *   gpsacq_destroy           SearchFree()            c/search_offline.cpp:114-117
 *   gpsacq_search            Sample() + Correlate()  c/search_offline.cpp:121-165, 169-201
 *                            for a batch of 5120-byte blocks (the body of the
 *                            SearchTask() loop, :239-246)
 *   gpsacq_search_device     same, capture already resident in HBM
 *   gpsacq_peak_keys_device  Correlate()'s ordering of two results, :196-198 (strict '>' over ascending dop), as 64-bit keys whose
 *                            integer MAX merges the per-PRN best of several GPUs / ranks
 *   gpsacq_pipe_*            same, batches in flight: the SearchTask() loop's fread of batch k+1 overlaps the search of batch k
 *   gpsacq_search_iq8        same on an 8-bit IQ capture: what proc_rtl_bin_for_gps.m / proc_hackrf_bin_for_gps.m + gps_test
 *                            do in two steps through a 1-bit file, fused into the forward transform
 *   gpsacq_set_doppler_step  the Doppler grid of Correlate()'s loop, :176,182 (finer or coarser than fs/40000)
 *   gpsacq_set_cell_handout  how the iterations of Correlate()'s `for dop` loop (:176) and of SearchTask()'s `for sv` loop (:239) reach the
 *                            compute units: drawn at run time by persistent workgroups (default) or one workgroup per cell; same results
 *   gpsacq_multi_search_grid the same Correlate() grid cut over several GPUs, peaks merged by one RCCL all-reduce
 *   gpsacq_multi_search_blocks  the SearchTask() run loop (:237-262) cut over several GPUs by whole runs, per-PRN best
 *                            peak merged by one RCCL all-reduce
 *   gpsacq_search_code       SearchCode()            c/search_offline.cpp:205-209
 *   gpsacq_iq8_to_bits       the MATLAB pre-processing that produces gps_test's input from an 8-bit IQ
 *                            capture: proc_rtl_bin_for_gps.m:12-26,31-47, proc_hackrf_bin_for_gps.m:7-19
 *   gpsacq_generate          the role of gps_sig_gen.m (synthetic 1-bit capture; here noise + any PRN set with Doppler)
 *   gpsacq_generate_range    any byte window of that stream (a function of the absolute sample index): what lets every rank of a
 *                            multi-GPU job make its own blocks of the ONE capture all world sizes search
 *   gpsacq_generate_sig      gps_sig_gen.m:8-41 itself (one PRN, navigation bits, raised-cosine BPSK at fs/4), bit-exact
 *   gpsacq_generate_sig_tx   gps_sig_gen.m:21-30, the script's int8 complex-baseband file for HackRF replay
 *   gpsacq_handoff           CHANNEL::Start()'s NCO set-up from a search hit, c/channel.cpp:134-163
 *                            (the first consumer of the search result in the online receiver)
 *   gpsacq_track_start       CHANNEL::Start() + Reset(), c/channel.cpp:104-163: a tracking channel's state from a search hit
 *   gpsacq_track             the FPGA's early/prompt/late integrate-and-dump and the embedded CPU's 1 kHz PI loops
 *                            ("Homemade GPS Receiver", sections "Hardware / software split" and after), plus the host's
 *                            AGC (CHANNEL::CheckPower(), c/channel.cpp:265-288) and code-aided carrier reset (:199-206)
 *   gpsacq_track_iq8         the same channels on an 8-bit IQ capture (README.md:83-115's rtl-sdr / HackRF flow carried on past the search):
 *                            sign mode = the scripts' 1-bit conversion + gpsacq_track, bit for bit; multi-bit mode = complex channels
 *                            that keep the amplitudes and the quadrature arm (no reference counterpart: its channels are 1-bit)
 *   gpsacq_track_start_iq8   CHANNEL::Start() for such a channel: the carrier NCO where the satellite sits in the raw capture
 *   gpsacq_track_default_params_iq8  the loop shifts of c/channel.cpp:104-130 rescaled to the capture's sample RMS
 *   gpsacq_iq8_accumulate_power  sum(y .* conj(y)) of proc_rtl_bin_for_gps.m's y, as exact integers (for that RMS)
 *   gpsacq_generate_iq8_range  gpsacq_generate_nav_range's law written as an 8-bit complex capture at a residual IF (no reference
 *                            counterpart: the reference has no 8-bit generator; rtl-like test files)
 *   gpsacq_nav_bits          the FPGA's NAV bit decision (sign of the I arm over a 20-epoch bit)
 *   gpsacq_nav_subframes     CHANNEL::ParityCheck(), c/channel.cpp:329-353, with the IS-GPS-200 Table 20-XIV parity
 *   gpsacq_generate_nav_range  gpsacq_generate_range with navigation data on every satellite
 *   gpsacq_ephemeris_load    EPHEM::Subframe1/2/3(), c/ephemeris.cpp:36-68, with the fields of IS-GPS-200 Tables 20-I and 20-III
 *   gpsacq_ephemeris_valid   EPHEM::Valid(), c/ephemeris.cpp:177-179 (IODC's eight low bits compared)
 *   gpsacq_sat_states        EPHEM::GetClockCorrection() + GetXYZ(), c/ephemeris.cpp:114-173, for a batch of transmit times
 *   gpsacq_fix_batch         Solve() + LatLonAlt(), c/solve.cpp:137-293, for a batch of receive instants
 *   gpsacq_observables       SNAPSHOT::GetClock(), c/solve.cpp:118-133, for every channel at a batch of receive instants: the
 *                            uncorrected transmit times, read off the records of the tracking channels
 *   gpsacq_time_tag_from_subframe  the TOW term of GetClock() (c/solve.cpp:125): which millisecond of the week a channel epoch is
 *   gpsacq_fix_track_device  GetClock() + Solve() + LatLonAlt() in one go: records -> observations -> fixes without a host copy
 *   gpsacq_sample_spectrum   Sample()'s fwd_buf      c/search_offline.cpp:161 (parity probe)
 *   gpsacq_code_spectrum     SearchInit()'s code[sv] c/search_offline.cpp:105-106 (parity probe)
 *
 * The C++-linkage mirror of the reference API itself (SearchInit/SearchTask/... consuming
 * the caller's FC/FS/max_fo globals) is include/gps_search.h, implemented on top of this ABI.
 */
#ifndef GPSACQ_H
#define GPSACQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared here are exported */
#define GPSACQ_API __attribute__((visibility("default")))

#define GPSACQ_FFT_LEN 40000      /* FFT_LEN, c/gps_offline.h:15 (compile-time in the reference) */
#define GPSACQ_NUM_SATS 32        /* NUM_SATS, c/gps_offline.h:16 */
#define GPSACQ_BLOCK_BYTES 5120   /* bytes consumed per Sample(): 10 packets x 512 B */

/* status codes */
#define GPSACQ_OK 0
#define GPSACQ_ERR_ARG 1          /* bad argument */
#define GPSACQ_ERR_DEVICE 2       /* no usable gfx950 device / HIP runtime error */
#define GPSACQ_ERR_UNSUPPORTED 3  /* parameter outside what the kernels cover: max_fo >= fs/2, ref_quirks + non-coherent */
#define GPSACQ_ERR_NOMEM 4

/* One engine = one device + one HIP stream + its scratch.  An engine is NOT thread-safe (the
 * reference's search stage is a single-instance, non-reentrant module as well, c/search_offline.cpp:55-64):
 * use one engine per host thread / per GPU.  gpsacq_last_error() is per thread. */
typedef struct gpsacq_engine gpsacq_engine;

typedef struct {
    double fc;          /* carrier (2nd IF) frequency in Hz      -- global FC  */
    double fs;          /* sampling rate in Hz                   -- global FS  */
    double max_fo;      /* Doppler search half-range in Hz       -- global max_fo */
    int32_t device;     /* HIP device ordinal */
    int32_t ref_quirks; /* 1: reproduce the reference's fwd_buf overrun, which replaces
                           code[0][0..959] by the block's samples 40000..40959 (PRN index 0
                           only; g++ BSS layout).  0: well-defined behaviour. */
} gpsacq_params;

/* one (block, PRN, Doppler bin): what Correlate()'s inner loop computes (:178-196) */
typedef struct {
    float max_pwr;   /* largest |IFFT|^2 over the first FS/1000 lags */
    int32_t max_i;   /* its lag (first one on ties) */
    float tot_pwr;   /* sum of |IFFT|^2 over those lags */
    float snr;       /* max_pwr / (tot_pwr / lags) */
} gpsacq_cell;

/* one (block, PRN): Correlate()'s return value and out-parameters (:196-200) */
typedef struct {
    float snr;         /* best SNR over the Doppler bins (0 if none > 0) */
    int32_t lo_shift;  /* Doppler bin of the best SNR, in units of fs/40000 Hz */
    int32_t ca_shift;  /* code phase (lag, samples) of the best SNR */
    float max_pwr;     /* max_pwr of that cell */
} gpsacq_peak;

/* one search task: block index into the capture, PRN index 0..31 */
typedef struct {
    int32_t block;
    int32_t prn;
} gpsacq_task;

typedef struct {
    int32_t fft_len;     /* 40000 */
    int32_t dmax;        /* Doppler bins searched are -dmax..+dmax (:176) */
    int32_t num_doppler; /* bins searched per task: 2*dmax+1 unless a window is set */
    int32_t first_doppler; /* first bin searched: -dmax unless a window is set */
    int32_t num_lags;    /* lags scanned per cell (:190) */
    int32_t acc_columns; /* kernel instance in use */
    int32_t device;
    int32_t compute_units;
    char device_name[64];
    /* Doppler grid (gpsacq_set_doppler_step); reference grid: sub = stride = 1, step = fs/40000 */
    int32_t doppler_sub;         /* sub-bin offsets per FFT bin (step = bin / sub) */
    int32_t doppler_stride;      /* or whole bins per grid point (step = bin * stride) */
    int32_t num_doppler_total;   /* grid points of the full +-max_fo range */
    int32_t first_doppler_total; /* index of the lowest one (= -(num_doppler_total - 1) / 2) */
    double doppler_step_hz;      /* lo_shift, first_doppler, Doppler windows are in units of this step */
} gpsacq_info;

/* per-stage device time of the last gpsacq_search* call, milliseconds (HIP events on the
 * engine's stream) and launch counts -- used by bench.py for the roofline line */
typedef struct {
    float ms_total;
    float ms_sample;     /* unpack + mix + forward FFT (both kernels) */
    float ms_correlate;  /* correlate kernel launches only */
    float ms_peaks;
    int32_t correlate_launches;
    int64_t cells;
} gpsacq_timing;

/* SearchInit(): builds the 32 code spectra, LO tables and twiddles on the device. */
GPSACQ_API int gpsacq_create(const gpsacq_params* params, gpsacq_engine** out);
/* SearchFree() */
GPSACQ_API void gpsacq_destroy(gpsacq_engine* e);
/* message of the last failing call on this thread ("" if none) */
GPSACQ_API const char* gpsacq_last_error(void);
GPSACQ_API int gpsacq_get_info(const gpsacq_engine* e, gpsacq_info* info);

/*
 * Search a batch.  `bits`: capture bytes, 1-bit real IF samples packed LSB first; block b
 * starts at bits + b*stride and 5120 bytes of it are read (5000 transformed; the last 120
 * only matter with ref_quirks).  `tasks`: n_tasks (block, prn) pairs, or NULL for the
 * reference's schedule: task t = (block t, prn t % 32) with n_tasks == n_blocks
 * (SearchTask(), :239-246).  Outputs (either may be NULL): cells[n_tasks][num_doppler] in
 * ascending Doppler-bin order, peaks[n_tasks].  Host pointers; returns after completion.
 */
GPSACQ_API int gpsacq_search(gpsacq_engine* e, const uint8_t* bits, size_t n_blocks, size_t stride,
                  const gpsacq_task* tasks, size_t n_tasks, gpsacq_cell* cells, gpsacq_peak* peaks);

/*
 * Same with every buffer already in this device's memory (bits, tasks, cells, peaks are
 * device pointers; tasks may be NULL as above; cells may be NULL).  Work is enqueued on the
 * engine's stream; `sync` != 0 waits for completion.  A device task list is not read by the host:
 * a task whose block or prn is out of range is skipped by the kernel and reported as cells with
 * max_i = -1, snr = 0 (peak: snr = 0) instead of GPSACQ_ERR_ARG.
 */
GPSACQ_API int gpsacq_search_device(gpsacq_engine* e, const void* d_bits, size_t n_blocks, size_t stride,
                         const void* d_tasks, size_t n_tasks, void* d_cells, void* d_peaks, int sync);
/*
 * Pipelined host-buffer searches on the reference schedule (task t = block t against PRN t % 32, the body of SearchTask()'s
 * loop :237-262).  A slot owns a pinned host staging buffer, a device copy and a pinned peak array:
 *   buf = gpsacq_pipe_buffer(e, slot, nbytes)      pinned buffer of >= nbytes (fread the batch straight into it); NULL on error.  A call
 *                                                  that asks for more than the slot holds re-allocates it: pointers from earlier calls
 *                                                  for that slot are then invalid (ask once for the largest batch)
 *   gpsacq_pipe_submit(e, slot, n_blocks, stride, iq)   upload on a second stream + search, returns at once (iq == NULL: 1-bit
 *                                                  blocks `stride` bytes apart; else 8-bit IQ, see gpsacq_search_iq8)
 *   gpsacq_pipe_collect(e, slot, &peaks, &n)       waits for THAT slot's search; peaks stay valid until its next submit
 * Searches run in submit order.  With 2-3 slots the caller's read of batch k+1 and report of batch k-1 overlap batch k.
 */
GPSACQ_API int gpsacq_reserve(gpsacq_engine* e, size_t n_blocks); /* scratch for batches of up to n_blocks blocks, once */
#define GPSACQ_PIPE_SLOTS 3
struct gpsacq_iq8_input;
GPSACQ_API uint8_t* gpsacq_pipe_buffer(gpsacq_engine* e, int slot, size_t nbytes);
GPSACQ_API int gpsacq_pipe_submit(gpsacq_engine* e, int slot, size_t n_blocks, size_t stride, const struct gpsacq_iq8_input* iq);
GPSACQ_API int gpsacq_pipe_collect(gpsacq_engine* e, int slot, const gpsacq_peak** peaks, size_t* n_peaks);

/*
 * Restrict the search to Doppler bins first_bin .. first_bin+n_bins-1 (within -dmax..+dmax).
 * Used to shard one block's PRN x Doppler grid over several GPUs (no reference equivalent: the
 * reference always scans the full range, :176).  cells rows then hold n_bins entries and
 * lo_shift stays an absolute bin number.
 */
GPSACQ_API int gpsacq_set_doppler_window(gpsacq_engine* e, int first_bin, int n_bins);
/*
 * How the correlate kernel's cells reach the compute units (no reference equivalent: Correlate(), c/search_offline.cpp:169-201, is a
 * serial loop).  on != 0 (the default; GPSACQ_CORR_PERSIST=0 in the environment at gpsacq_create turns it off): three resident
 * workgroups per CU draw (task, Doppler point) tickets at run time -- every XCD of the package takes work at its own pace, a task's
 * points (or a ~128-point chunk of a fine grid's task) stay on one XCD.  on == 0: one workgroup per cell, block g on XCD g % 8, as up
 * to round 5.  The cells are the same bit for bit either way (the same arithmetic per cell); only the time differs (3-5 % by box).
 * Applies to the instances that run three workgroups per CU (every coherent search up to fs = 8.25 MHz, and the 12-column
 * non-coherent one without re-alignment); the others ignore it.
 */
GPSACQ_API int gpsacq_set_cell_handout(gpsacq_engine* e, int on);
/*
 * Doppler grid step (extension; the reference's grid is whole FFT bins of fs/40000 Hz, c/search_offline.cpp:176,182,
 * and its front end ignores argv[4]).  step_hz <= 0 or within (bin, 2 bin): the reference grid.  step_hz < bin: the
 * grid is refined to bin / R, R = ceil(bin / step_hz) (the finest grid not coarser than asked): each block is
 * transformed R times, spectrum r being that of the block multiplied by exp(-2 pi i (r/R) n / 40000) -- a carrier
 * offset of r/R of a bin, exact, folded into the forward transform's twiddles -- and grid point k = d R + r pairs
 * spectrum r with the code spectrum shifted by d whole bins.  step_hz >= 2 bin: every S-th bin, S = floor(step_hz /
 * bin).  The range is -K..+K with K = trunc(max_fo / step) like :176.  Afterwards num_doppler / first_doppler /
 * lo_shift / Doppler windows count grid points (Hz = index * gpsacq_info.doppler_step_hz), cells rows hold one
 * record per grid point in ascending frequency, and the Doppler window is reset to the full range.
 * Costs R forward transforms and R x 320 KB of spectra per block; the correlate work per grid point is unchanged.
 */
#define GPSACQ_MAX_DOPPLER_SUB 16
GPSACQ_API int gpsacq_set_doppler_step(gpsacq_engine* e, double step_hz);
/*
 * Non-coherent accumulation (extension; the reference scans one coherent block per cell,
 * c/search_offline.cpp:176-199): every task then sums |IFFT|^2 per lag over n_acc block spectra
 * task.block + k*block_step (k < n_acc) before the peak scan; cells/peaks describe the summed power.
 * Lags only line up if consecutive accumulated blocks start a whole number of C/A periods apart:
 * lay the capture out with stride = gpsacq_aligned_stride(e) bytes (smallest multiple of
 * FS/8000 bytes >= 5120; -1 if FS/1000 is not a multiple of 8).  n_acc = 1 restores the
 * reference behaviour.  With tasks == NULL the schedule is task t = (block t, prn t % 32) for
 * t < n_tasks <= n_blocks - (n_acc-1)*block_step.
 */
GPSACQ_API int gpsacq_set_noncoherent(gpsacq_engine* e, int n_acc, int block_step);
/*
 * Code-creep compensation for the non-coherent mode (off by default).  A carrier offset f -- true
 * Doppler, or the crystal error of a single-oscillator front end such as the rtl-sdr, which is what
 * the +-100 kHz search range is for -- comes with a code-rate offset f/L1, so the correlation peak of
 * accumulated block k sits k * T * f / L1 samples later than block 0's (T = samples between
 * accumulated blocks = block_step * stride * 8): 1.07 samples per block at 40 kHz and fs = 2.8 MHz.
 * With compensation on, block k's powers are moved back by round(k * c * bin) whole samples (modulo
 * the fs/1000 lags) before they are summed, c = T * (fs/40000) / 1575.42e6 in float, bin = the cell's
 * Doppler bin; ca_shift then refers to block 0.  At fs > 10 MHz (more than 10000 lags, searched in
 * several passes of 40 columns) the per-lag sums are kept in device memory -- 4 * fs/1000 bytes per cell, the batch's tasks taken
 * in chunks of at most 1 GB of sums.
 */
GPSACQ_API int gpsacq_set_creep_compensation(gpsacq_engine* e, int on);
/*
 * Block alignment for the non-coherent mode (off by default; SURVEY.md section 8d, configs[3]: "per-block lag re-alignment").
 * Accumulated blocks whose starts are T = block_step * stride * 8 samples apart (stride / 2 for an 8-bit IQ capture) see the
 * code T mod (fs/1000) samples further on each time; with alignment on, block k's powers are moved back by k * (T mod S)
 * samples (modulo the S = fs/1000 lags) before they are summed, so any stride -- the file's own 5120-byte blocks, an IQ
 * capture's 81920 -- accumulates in phase and ca_shift refers to block 0.  gpsacq_aligned_stride() remains the layout that needs
 * no re-alignment (and lets the sums stay in registers).  Needs fs to be a whole number of samples per code period (fs = 1000 S).
 */
GPSACQ_API int gpsacq_set_block_alignment(gpsacq_engine* e, int on);
GPSACQ_API int gpsacq_aligned_stride(const gpsacq_engine* e);
/*
 * The merge keys of the multi-GPU reduction (the reference is one thread, c/search_offline.cpp has no
 * counterpart), made from the peaks of a gpsacq_*_device search on the engine's stream, behind that search, without a host wait:
 *   key = snr bits << 32 | (0xFFFF - (lo_shift + K)) << 16 | ca_shift,  K = -gpsacq_info.first_doppler_total
 * so that integer MAX over keys = "higher SNR, ties to the LOWER Doppler point" -- the strict '>' scan of :196-198.  (SNR >= 0:
 * the keys order the same as signed or unsigned 64-bit integers.)
 *   per_prn != 0: d_keys[32] = the best key of every PRN over the peaks t with t % 32 == PRN (the reference schedule, task t
 *                 <-> PRN t % 32, :239-246): what ONE all-reduce(MAX) of 256 bytes merges between the ranks of the block
 *                 decomposition.  n_peaks == 0 (a rank without work) writes 32 zero keys, neutral for MAX.
 *   per_prn == 0: d_keys[n_peaks], one key per peak (Doppler-slab decomposition: every rank holds every task).
 * Device pointers; d_peaks as written by gpsacq_search_device / gpsacq_search_iq8_device on this engine.
 */
GPSACQ_API int gpsacq_peak_keys_device(gpsacq_engine* e, const void* d_peaks, size_t n_peaks, int per_prn, void* d_keys, int sync);
GPSACQ_API int gpsacq_synchronize(gpsacq_engine* e);
/* stage times of the most recent search (waits for it to finish) ... */
GPSACQ_API int gpsacq_last_timing(const gpsacq_engine* e, gpsacq_timing* t);
/* ... and of the search n_back calls earlier (0 = last; the 8 most recent are kept): lets a caller
 * that enqueues searches with sync = 0 read a finished search's times while the next one runs */
GPSACQ_API int gpsacq_timing_ago(const gpsacq_engine* e, int n_back, gpsacq_timing* t);
/* Measurement aid next to gpsacq_last_timing (no reference counterpart): enqueues, on the engine's stream, a small kernel that writes
 * the shader-cycle counter (s_memtime) of every compute unit to d_stamp[XCC id << 6 | SE id << 4 | CU id] (device memory,
 * GPSACQ_STAMP_SLOTS x 8 bytes; zero it first: a slot no wave reached keeps its zero).  The counter is per compute unit -- its own
 * offset, and it stands still while the CU is clock-gated -- so only differences of the same slot mean anything.  Two calls around
 * a stretch of work that keeps the CUs busy, divided by the time between them, give the average shader clock every CU held over
 * that stretch: what bench.py's box-independent roofline (cycles per cell) is made of. */
#define GPSACQ_STAMP_SLOTS 512
GPSACQ_API int gpsacq_cycle_stamp_device(gpsacq_engine* e, void* d_stamp, int sync);
/* the engine's HIP stream (a hipStream_t) for callers that order their own device work after an
 * asynchronous gpsacq_*_device call with an event instead of a host wait; NULL for a NULL engine */
GPSACQ_API void* gpsacq_stream(gpsacq_engine* e);

/*
 * 8-bit IQ capture -> the 1-bit real-IF stream gpsacq_search() takes.  format GPSACQ_IQ_U8: rtl-sdr
 * (unsigned, offset 128, interleaved I,Q; proc_rtl_bin_for_gps.m:12-16), GPSACQ_IQ_S8: HackRF (signed;
 * proc_hackrf_bin_for_gps.m:7-11).  remove_dc: subtract the complex mean of the whole capture
 * (`y = y - mean(y)`).  mix_hz != 0: take real(y * exp(2 pi i mix_hz n / fs)) (proc_rtl...m:41),
 * else the real part.  fs <= 0: the engine's fs.  Output: ceil(n/8) bytes, sample n in bit n%8 of
 * byte n/8 (MATLAB 'ubit1'), bit = 1 where the value is <= 0.  The _device form takes device
 * pointers (IQ 16-byte aligned) and runs on the engine's stream.
 */
#define GPSACQ_IQ_U8 0
#define GPSACQ_IQ_S8 1
GPSACQ_API int gpsacq_iq8_to_bits(gpsacq_engine* e, const void* iq, size_t n_samples, int format, int remove_dc,
                       double mix_hz, double fs, uint8_t* bits_out);
GPSACQ_API int gpsacq_iq8_to_bits_device(gpsacq_engine* e, const void* d_iq, size_t n_samples, int format, int remove_dc,
                              double mix_hz, double fs, void* d_bits_out, int sync);

/*
 * Search an 8-bit IQ capture directly: README.md:83-115's rtl-sdr / HackRF flow (MATLAB conversion to a 1-bit file, then
 * gps_test on that file) as one call.  The forward transform stages each block from the IQ bytes -- mean removal, mixer,
 * sign, LO quadrature mix and bit transpose in one pass -- so the 1-bit stream is never written; results are identical to
 * gpsacq_iq8_to_bits() followed by gpsacq_search() (same per-sample arithmetic, csrc/iq_convert.hpp).  Block b starts
 * `stride` bytes into `iq` (a multiple of 16, >= 80000; 81920 = the 40960 samples one Sample() call consumes) and its
 * first 40000 samples are transformed.  With ref_quirks the stream is converted to bits first (the patch needs samples
 * 40000..40959 as bits) -- same results, one more pass.
 */
#define GPSACQ_SAMPLES_SIGN 0
#define GPSACQ_SAMPLES_REAL 1
#define GPSACQ_SAMPLES_COMPLEX 2
typedef struct gpsacq_iq8_input {
    int32_t format;          /* GPSACQ_IQ_U8 / GPSACQ_IQ_S8 */
    int32_t remove_dc;       /* subtract (mean_i, mean_q) */
    double mean_i, mean_q;   /* complex mean of the WHOLE capture in sample units (`y - mean(y)`, proc_rtl_bin_for_gps.m:17):
                                integer sums / sample count; gpsacq_iq8_accumulate_sums() for a capture streamed in pieces */
    double mix_hz;           /* 0: real part; else real(y * exp(2 pi i mix_hz n / fs))  (proc_rtl_bin_for_gps.m:41) */
    double fs;               /* sampling rate of the mixer phase; <= 0: the engine's */
    uint64_t first_sample;   /* capture sample index of the buffer's first sample: the mixer's n */
    uint64_t total_samples;  /* samples in the whole capture (bits beyond it read 0); 0: every block handed over is complete */
    int32_t multibit;        /* 0: the sign of each sample, as the scripts write it and gps_test reads it.  1: the samples keep their
                                amplitude ("direct float path"; no reference counterpart -- gps_test only takes 1-bit files): the
                                real-IF value as a float, the quadrature LO of Sample() (:143-153) applied as signs; spares the
                                1-bit quantisation loss.  2 (GPSACQ_SAMPLES_COMPLEX): the capture is at baseband already -- I + jQ
                                is what Sample() builds in fwd_buf (:149-150), e.g. the int8 +-30 file the reference's own
                                c/conv_1bit_bin_to_hackrf_bin.cpp:61-80 writes for HackRF replay, or gps_bin1bit_log2bin.m's +-100 one -- so no LO: the complex samples
                                (less the mean, turned by exp(2 pi i mix_hz n / fs) when a residual IF is named) are transformed
                                as they are; the engine's fc plays no part.  1 and 2: not with ref_quirks; on a Doppler grid finer
                                than a bin the sub-bin turn is applied to the float samples (one copy per sub-bin offset). */
    int32_t reserved;
} gpsacq_iq8_input;
GPSACQ_API int gpsacq_search_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_blocks, size_t stride,
                      const gpsacq_task* tasks, size_t n_tasks, gpsacq_cell* cells, gpsacq_peak* peaks);
GPSACQ_API int gpsacq_search_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_blocks, size_t stride,
                             const void* d_tasks, size_t n_tasks, void* d_cells, void* d_peaks, int sync);
/* adds the exact integer sums of I and Q (offset removed for GPSACQ_IQ_U8) over n_samples of a host buffer to sums[0..1] */
GPSACQ_API int gpsacq_iq8_accumulate_sums(gpsacq_engine* e, const void* iq, size_t n_samples, int format, int64_t sums[2]);

/*
 * Synthetic 1-bit real-IF capture generated on the device (the reference's gps_sig_gen.m writes one
 * noise-free PRN; this is the signal model of SURVEY.md section 8d): white Gaussian noise of standard
 * deviation noise_sigma plus, per satellite, amplitude * C/A chip * cos(2 pi ((fc + doppler)/fs m +
 * carrier_phase)), chips advancing at 1.023e6 (1 + doppler/L1) per second from code_phase_samples;
 * bit = (sum < 0), sample m in bit m % 8 of byte m / 8.  Uses the engine's fc and fs.  Deterministic
 * in (seed, arguments).  A search of the result reports lo_shift = round(doppler * 40000 / fs) and
 * ca_shift = (code_phase + 8 * stride * block) mod (fs / 1000) for block-sized strides.
 *
 * THE GENERATOR'S LAW (gpsacq_generate*, gpsacq_generate_nav_range*, gpsacq_generate_iq8_range*; tests/gen_ref.py restates it from
 * this text).  m is the absolute sample index, a 64-bit unsigned integer, first_sample included; every quantity below is a
 * function of m and the arguments alone.
 *   Rates (host, IEEE double, in this order of operations):
 *       chips_per_sample  = 1.023e6 * (1.0 + doppler_hz / 1575.42e6) / fs
 *       cycles_per_sample = (fc + doppler_hz) / fs          (8-bit generator: if_hz in the place of fc)
 *     amplitude, noise_sigma and scale are floats.
 *   Noise.  h = mix(seed ^ (m * 0x9e3779b97f4a7c15)) in 64-bit unsigned arithmetic, mix being the splitmix64 finaliser
 *       z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  z ^ (z >> 31).
 *     u1 = (float(h >> 32) + 1) * 2^-32, a float in (0, 1] (1 where the float sum rounds up to 2^32); u2 = float(h & 0xffffffff) * 2^-32.
 *     n_I = sqrt(-2 ln u1) cos(2 pi u2), n_Q = sqrt(-2 ln u1) sin(2 pi u2), in float with the fast intrinsics (__logf, __cosf,
 *     __sinf; 2 pi as the float 6.2831853).  The 1-bit generator uses n_I, the 8-bit one both.
 *   Chip count.  q = floor((m + code_phase_samples) * chips_per_sample), a signed 64-bit integer, floor also below zero.  The chip
 *     is chip[q mod 1023] of the PRN (+1 for a C/A bit of 0, -1 for 1), the modulo a true one for q < 0 (q = -1: chip 1022).  The
 *     navigation bit is nav[s * n_nav_bits + (floor(q / 20460) mod n_nav_bits)], floor and modulo true ones for q < 0 as well
 *     (q = -1: bit n_nav_bits - 1).
 *   Carrier.  p = cycles_per_sample * m + carrier_phase_cycles in double, reduced to [0, 1) by p - floor(p), cast to float, and
 *     the carrier is cospif(2 p) (and sinpif(2 p) for Q): exact zeros at the quarter points, exact +-1 at 0 and 1/2.
 *   Sum.  y = noise_sigma * n_I + sum over the satellites in their order of amplitude * nav * chip * cos, in float.
 *   1-bit decision.  bit = (y < 0); a sum of +0 or -0 gives bit 0.
 *   8-bit value.  rintf(scale * y) per arm, ties to even, clamped to [-127, 127] (never -128), plus 128 for GPSACQ_IQ_U8.  The Q
 *     arm is noise_sigma * n_Q + sum amplitude * nav * chip * (+sin).
 *   Precision.  Code position and carrier phase are evaluated in double from the absolute sample index, as a product and a sum,
 *     or fused; their resolution is 2^-52 of their size, e.g. 2e-4 cycle and 2e-4 chip at sample 2^40.  The float cast of the
 *     phase resolves 2^-24 cycle.  Where the exact code position lies within rounding of an integer, or the exact sum within
 *     rounding of zero or of a half-integer, either neighbour may come out.
 */
typedef struct {
    int32_t prn;                 /* 1..32 */
    float amplitude;             /* relative to noise_sigma = 1: 0.151 ~ 45 dB-Hz */
    double doppler_hz;
    double code_phase_samples;
    double carrier_phase_cycles;
} gpsacq_sat;
GPSACQ_API int gpsacq_generate(gpsacq_engine* e, uint8_t* bits_out, size_t n_bytes, const gpsacq_sat* sats, int n_sats,
                    float noise_sigma, uint64_t seed);
GPSACQ_API int gpsacq_generate_device(gpsacq_engine* e, void* d_bits_out, size_t n_bytes, const gpsacq_sat* sats, int n_sats,
                           float noise_sigma, uint64_t seed, int sync);
/* Any byte range of that stream: the n_bytes that start at sample first_sample (a multiple of 8) -- byte first_sample / 8 of what
 * gpsacq_generate() writes for the same seed and satellites, bit for bit (noise and signals are functions of the absolute sample
 * index).  One rank of a multi-GPU job generates exactly its own blocks of THE capture every world size searches. */
GPSACQ_API int gpsacq_generate_range(gpsacq_engine* e, uint8_t* bits_out, size_t n_bytes, uint64_t first_sample, const gpsacq_sat* sats,
                          int n_sats, float noise_sigma, uint64_t seed);
GPSACQ_API int gpsacq_generate_range_device(gpsacq_engine* e, void* d_bits_out, size_t n_bytes, uint64_t first_sample,
                                 const gpsacq_sat* sats, int n_sats, float noise_sigma, uint64_t seed, int sync);

/*
 * The reference's own test signal (gps_sig_gen.m:8-41, the script that wrote gps_sig_tmp.bin), generated on the device:
 * PRN `prn` (1..32), noise-free BPSK with the given navigation bits (+-1, 20 code periods each), 8 samples per chip
 * (fs = 8.184 MHz), raised-cosine shaping (MATLAB rcosine(1, 8)), carrier at fs/4 = 2.046 MHz, 1 bit per sample, LSB first.
 * Arithmetic in double in the script's own order: with the 100 bits of the bundled file (tests/golden/
 * gps_sig_tmp_databits.json; the script draws them with an unseeded rand) the output equals gps_sig_tmp.bin bit for bit.
 * n_bytes must be gpsacq_sig_bytes(n_data_bits) = ceil((n_data_bits * 20 * 1023 * 8 + 48) / 8).  Search it with
 * fc = 2.046e6, fs = 8.184e6.
 */
GPSACQ_API size_t gpsacq_sig_bytes(int n_data_bits);
GPSACQ_API int gpsacq_generate_sig(gpsacq_engine* e, int prn, const int8_t* data_bits, int n_data_bits, uint8_t* bits_out, size_t n_bytes);
/*
 * The script's OTHER output (gps_sig_gen.m:21-30, gps_sig_tmp_for_hackrf_tx.bin -- what README.md section 2.2 replays through a
 * HackRF): the same shaped baseband, the navigation-bit sequence n_repeat times over (5 in the script), times 50, as 8-bit
 * complex samples at IF 0: I = int8(round(x * 50)), Q = 0, interleaved.  The stream has gpsacq_sig_tx_samples(n_data_bits,
 * n_repeat) = n_repeat * n_data_bits * 20 * 1023 * 8 + 48 complex samples (164 MB for the script's 100 bits x 5); any range
 * [first_sample, first_sample + n_samples) of it is written to iq_out[2 * n_samples].  Search it as complex baseband:
 * gpsacq_iq8_input{format = GPSACQ_IQ_S8, remove_dc = 0, multibit = GPSACQ_SAMPLES_COMPLEX} at fs = 8.184e6 (fc plays no part).
 */
GPSACQ_API uint64_t gpsacq_sig_tx_samples(int n_data_bits, int n_repeat);
GPSACQ_API int gpsacq_generate_sig_tx(gpsacq_engine* e, int prn, const int8_t* data_bits, int n_data_bits, int n_repeat,
                           uint64_t first_sample, size_t n_samples, int8_t* iq_out);

/*
 * Acquisition hand-off record: what the tracking channel derives from a search hit
 * (c/channel.cpp:144-163).  Host arithmetic only; no device needed.
 */
typedef struct {
    double lo_dop_hz;   /* carrier Doppler estimate  = lo_shift * fs / 40000                  (:145) */
    double ca_dop_hz;   /* code-rate Doppler         = lo_dop / L1 * 1.023e6                  (:146) */
    uint32_t lo_rate;   /* carrier NCO word          = (fc  + lo_dop) / fs * 2^32             (:149) */
    uint32_t ca_rate;   /* code NCO word             = (CPS + ca_dop) / fs * 2^32             (:150) */
    int32_t ca_shift;   /* code phase after creep    = ca_shift + nearbyint(ca_dop*secs*fs/CPS) (:160) */
    uint32_t ca_pause;  /* NCO pause to align the code generator = (2*spm - ca_shift) % spm, spm = samples
                           per millisecond (the reference hard-codes 20000 / 10000 for its 10 MHz FPGA, :163) */
} gpsacq_handoff_t;
GPSACQ_API int gpsacq_handoff(const gpsacq_peak* peak, double fc, double fs, double secs_since_sample, gpsacq_handoff_t* out);
/* gpsacq_handoff() reads lo_shift in FFT bins of fs / 40000 Hz -- the reference grid.  After gpsacq_set_doppler_step(), and
 * for gpsacq_multi_search_grid() peaks, lo_shift counts grid points of gpsacq_info.doppler_step_hz: pass that step here
 * (step_hz <= 0: FFT bins), or let the engine supply its own fc, fs and current step. */
GPSACQ_API int gpsacq_handoff_step(const gpsacq_peak* peak, double fc, double fs, double step_hz, double secs_since_sample, gpsacq_handoff_t* out);
GPSACQ_API int gpsacq_handoff_engine(const gpsacq_engine* e, const gpsacq_peak* peak, double secs_since_sample, gpsacq_handoff_t* out);

/*
 * Single-process multi-GPU search of ONE capture's PRN x Doppler grid (BASELINE.json configs[4]; the reference is
 * single-threaded, c/search_offline.cpp has no counterpart).  One engine per listed device; the Doppler grid -K..+K is
 * cut into one contiguous slab per device, every device searches all tasks over its slab, packs each task's best peak
 * into a 64-bit key (snr bits << 32 | (0xFFFF - grid index) << 16 | ca_shift: integer MAX = higher SNR, ties to the
 * LOWER Doppler point like the strict '>' of :196-198) and ONE ncclAllReduce(MAX, uint64) over RCCL (xGMI) merges them.
 * devices == NULL: ordinals 0..n_devices-1.  n_devices == 1 is the degenerate case (same result as gpsacq_search's
 * peaks).  peaks[n_tasks]: snr / lo_shift / ca_shift of the merged best and its max_pwr -- the key has no room for the
 * power, so the winner's value follows in a second all-reduce(MAX, float) (the engine whose key won contributes its value,
 * the others 0).  A device may be listed more than once: engines of one GPU merge their keys on that GPU and RCCL joins the
 * distinct GPUs only.  RCCL is dlopen'ed on first use (librccl.so.1); GPSACQ_ERR_DEVICE if it is missing.  With one distinct
 * GPU no RCCL call is made -- unless GPSACQ_MULTI_FORCE_RCCL=1 is set when the handle is created: then the communicator
 * (ncclCommInitAll over one device) and both all-reduces run as a one-rank group, the same calls a multi-GPU node makes.
 * Each engine's share of a call (staging copy out of the caller's pageable buffer, upload, search, download) is enqueued by
 * its own host thread through pinned buffers, so no device waits for another one's copies.
 */
typedef struct gpsacq_multi gpsacq_multi;
GPSACQ_API int gpsacq_multi_create(const gpsacq_params* params, const int32_t* devices, int n_devices, gpsacq_multi** out);
GPSACQ_API void gpsacq_multi_destroy(gpsacq_multi* m);
GPSACQ_API int gpsacq_multi_set_doppler_step(gpsacq_multi* m, double step_hz);
GPSACQ_API int gpsacq_multi_get_info(const gpsacq_multi* m, gpsacq_info* info, int32_t* n_devices);
GPSACQ_API int gpsacq_multi_search_grid(gpsacq_multi* m, const uint8_t* bits, size_t n_blocks, size_t stride,
                             const gpsacq_task* tasks, size_t n_tasks, gpsacq_peak* peaks);
/*
 * The headline decomposition (BASELINE.json north_star) in one process: a capture of whole runs
 * (32 blocks of `stride` >= 5120 bytes each, block b against PRN b % 32 -- the SearchTask() loop, c/search_offline.cpp:237-262)
 * is cut into one contiguous range of runs per device; every device searches its runs over the full Doppler grid, reduces
 * its peaks to the best per PRN as packed keys, and ONE ncclAllReduce(MAX, uint64) of 32 keys merges them.  Outputs, either
 * may be NULL: peaks[n_runs * 32] -- every (run, PRN) peak in file order, what SearchTask() reports -- and best[32], the
 * merged per-PRN best over the whole capture (max_pwr included: the winner's value, merged next to the keys as above).
 * n_devices == 1 is the degenerate case.  The engines' Doppler windows are left as they were.
 */
GPSACQ_API int gpsacq_multi_search_blocks(gpsacq_multi* m, const uint8_t* bits, size_t n_runs, size_t stride, gpsacq_peak* peaks,
                               gpsacq_peak* best);
/* Host-side times of the last gpsacq_multi_search_* call, milliseconds: enqueue_ms = entry until every device's work and the
 * merge were enqueued (what the calling thread costs the devices; flat in the number of devices), total_ms = the whole call;
 * rccl_allreduces = ncclAllReduce groups issued by this handle so far (0 when no communicator exists).  Any pointer may be NULL. */
GPSACQ_API int gpsacq_multi_last_call_ms(const gpsacq_multi* m, double* enqueue_ms, double* total_ms, int64_t* rccl_allreduces);

/*
 * ---- Tracking channels and NAV data (offline, on a recorded 1-bit real-IF capture) ----------------------------------------
 *
 * THE CHANNEL MODEL.  Integer arithmetic only; the kernels (csrc/track_channel.hpp) and the CPU model of the tests
 * (tests/c/track_model.c) are both written from this text, and agree bit for bit.  "mod 2^N" arithmetic is unsigned
 * wrap-around; the int64 fields below are two's-complement bit patterns of that arithmetic.  spm = samples per millisecond
 * (gpsacq_info.num_lags).  The sample stream is the one gpsacq_search() reads: sample m is bit m % 8 of byte m / 8, 1 = negative.
 * Chip values come from the C/A table of the engine (1 = chip value -1).
 *
 * One EPOCH is one code period.  It covers samples [s, s + n), s = next_sample, n = ceil((1023 * 2^32 - ca_pos) / ca_rate).
 * For sample s + j (0 <= j < n):
 *   carrier phase  ph = lo_phase + j * lo_rate (mod 2^32);  cos bit = bit31(ph) ^ bit30(ph),  sin bit = !bit31(ph)
 *                  (the bits are the signs of cos(2 pi ph) and of -sin(2 pi ph): the mix is x * exp(-i 2 pi ph), so a
 *                  signal ahead of the NCO gives Q > 0)
 *   prompt         P = ca_pos + j * ca_rate  (always < 1023 * 2^32);  early E = P + 2^31, late L = P - 2^31, each wrapped
 *                  into [0, 1023 * 2^32);  the chip at position X is chip[X >> 32]
 *   sums           I_X = sum (1 - 2 (x ^ chip_X ^ cos bit)),  Q_X = sum (1 - 2 (x ^ chip_X ^ sin bit)),  X in E, P, L
 * After the epoch:  lo_phase += n * lo_rate (mod 2^32);  ca_pos += n * ca_rate - 1023 * 2^32;  next_sample += n;  epoch += 1.
 * Then, with k = the epoch count just reached:
 *   AGC (c/channel.cpp:265-288)  if k % agc_period == 0: pwr[pwr_pos] = IP^2 + QP^2, pwr_pos = (pwr_pos + 1) % 8;
 *                  S = sum of the 8 entries (zeros at start);  gain_adj != 0: S < 8 agc_lo -> gain_adj = 0;
 *                  gain_adj == 0: S > 8 agc_hi -> gain_adj = -1.  The carrier shifts are lo_ki + gain_adj, lo_kp + gain_adj.
 *   carrier        while fll_left > 0 (FLL pull-in, then fll_left -= 1):
 *                      dot = IP' IP + QP' QP,  cross = IP' QP - QP' IP  (IP', QP' = the previous epoch's prompt, 0 at start)
 *                      e = sign(dot) * cross;  lo_int += e * 2^fll_k;  lo_rate = lo_int >> 32
 *                  else (Costas):  e = IP * QP;  lo_int += e * 2^(lo_ki + gain_adj);  lo_rate = (lo_int + e * 2^(lo_kp + gain_adj)) >> 32
 *                  then IP' = IP, QP' = QP.
 *   code (DLL)     e = (IE^2 + QE^2) - (IL^2 + QL^2);  ca_int += e * 2^ca_ki;  ca_rate = (ca_int + e * 2^ca_kp) >> 32
 *                  (early stronger = the signal's code is ahead = raise the rate)
 *   aid            if k == aid_epoch (c/channel.cpp:199-206, L1 / 1.023 MHz = 1540):
 *                      lo_int = lo_nom + (ca_int - ca_nom) * 1540;  lo_rate = lo_int >> 32
 *   window         the channel is LOST (status = GPSACQ_TRACK_LOST, it runs no further epoch) when |lo_int - lo_nom| or
 *                  |(lo_rate << 32) - lo_nom| exceeds lo_window, or |ca_int - ca_nom| or |(ca_rate << 32) - ca_nom| exceeds
 *                  ca_window (differences as signed 64-bit), or when the next epoch's n is outside [min_epoch, max_epoch].
 * ">> 32" keeps bits 32..63 of the 64-bit sum as the new 32-bit rate word.
 */
#define GPSACQ_TRACK_OK 0
#define GPSACQ_TRACK_LOST 1
typedef struct {
    int32_t prn;            /* 1..32 */
    int32_t status;         /* GPSACQ_TRACK_OK / GPSACQ_TRACK_LOST */
    uint64_t next_sample;   /* absolute sample index where the next epoch starts */
    uint32_t lo_phase;      /* carrier NCO phase at next_sample, cycles * 2^32 */
    uint32_t lo_rate;       /* carrier NCO word, cycles per sample * 2^32 */
    int64_t lo_int;         /* carrier PI integrator, cycles per sample * 2^64 (mod 2^64) */
    uint64_t ca_pos;        /* prompt code position at next_sample, chips * 2^32, in [0, 1023 * 2^32) */
    uint32_t ca_rate;       /* code NCO word, chips per sample * 2^32 */
    int32_t epoch;          /* epochs run since gpsacq_track_start */
    int64_t ca_int;         /* code PI integrator, chips per sample * 2^64 */
    int64_t lo_nom;         /* nominal carrier word, fc / fs: (uint64)(uint32)(fc / fs * 2^32) << 32 */
    int64_t ca_nom;         /* nominal code word, 1.023 MHz / fs, the same way */
    int32_t gain_adj;       /* AGC: 0 or -1 */
    int32_t pwr_pos;        /* next slot of the power ring */
    int64_t pwr[8];         /* power ring, IP^2 + QP^2 */
    int32_t prev_ip, prev_qp; /* previous epoch's prompt (FLL) */
    int32_t fll_left;       /* FLL epochs still to run */
    int32_t reserved;
} gpsacq_track_chan;        /* 160 bytes */

/* Loop settings; gpsacq_track_default_params() fills them for the engine's fs and every field may then be changed.
 * Defaults: the reference's 10 MHz shifts (c/channel.cpp:104-130: lo ki/kp 20/27, ca ki/kp 11/23) plus
 * round(log2((10000 / spm)^2)) -- both discriminators scale with the square of the correlation amplitude, which scales with spm --
 * and above spm = 10000 round(log2((10000 / spm)^3)), as one step of an NCO word is also worth fs / 2^32 more Hz;
 * fll_k 25 at 10 MHz the same way; fll_epochs 500; aid_epoch -1 (off: the FLL covers the up-to-half-bin error of the hit);
 * agc_period 250 (4 polls per second, :201), agc_lo / agc_hi = floor(1200^2 (spm / 10000)^2), floor(1400^2 (spm / 10000)^2);
 * lo_window = 10 kHz, ca_window = 4 x 10 kHz / 1540 (26 Hz), both in the * 2^64 units of the integrators;
 * min_epoch / max_epoch = spm / 2, min(2 spm, 65535).  Every shift must lie in [0, 62]; 1 <= min_epoch <= max_epoch <= 65535.
 * Above fs = 40 MHz there are no defaults (GPSACQ_ERR_UNSUPPORTED: spm would no longer be samples per millisecond). */
typedef struct {
    int32_t lo_ki, lo_kp, ca_ki, ca_kp, fll_k;
    int32_t fll_epochs;
    int32_t aid_epoch;      /* < 0: no aid */
    int32_t agc_period;
    int64_t agc_lo, agc_hi;
    int64_t lo_window, ca_window;
    int32_t min_epoch, max_epoch;
} gpsacq_track_params;      /* 72 bytes */

/* One record per epoch (optional output of gpsacq_track): where it started, its six sums, and the NCO words it ran at. */
typedef struct {
    uint64_t sample;
    int32_t ie, qe, ip, qp, il, ql;
    uint32_t lo_rate, ca_rate;
} gpsacq_track_record;      /* 40 bytes */

GPSACQ_API int gpsacq_track_default_params(const gpsacq_engine* e, gpsacq_track_params* params);
/*
 * A channel for PRN prn (1..32) from a search hit (host arithmetic; CHANNEL::Start(), c/channel.cpp:134-163).  peak: the hit of a search whose block
 * started at absolute sample block_first_sample, on the engine's current Doppler grid (gpsacq_handoff_engine gives lo_rate and
 * ca_rate).  By the generator's law (gpsacq_sat) the prompt position at block_first_sample is ca_shift * 1.023e6 / fs chips: the
 * channel starts there at ca_pos = ca_shift * ca_rate (mod 1023 * 2^32) and lo_phase = block_first_sample * lo_rate (mod 2^32), then
 * pauses (c/channel.cpp:162-163) to the next code epoch: next_sample advances by n = ceil((1023 * 2^32 - ca_pos) / ca_rate) with the
 * NCOs, so that every epoch it runs is a whole one.  lo_int = lo_rate << 32, ca_int = ca_rate << 32, fll_left = params->fll_epochs.
 * params NULL: the defaults.
 */
GPSACQ_API int gpsacq_track_start(const gpsacq_engine* e, int prn, const gpsacq_peak* peak, uint64_t block_first_sample,
                                  const gpsacq_track_params* params, gpsacq_track_chan* chan);
/*
 * Run channels over a window of the capture: bits[n_bytes] holds samples first_sample .. first_sample + 8 n_bytes - 1
 * (first_sample a multiple of 8).  Every channel needs first_sample <= next_sample (GPSACQ_ERR_ARG otherwise); each runs every
 * epoch that ends inside the window, at most max_epochs, and stops early when LOST.  chans[n_chans] are read and written back,
 * so a later call on a window that starts at or before each next_sample continues them.  Outputs: prompt[n_chans][max_epochs][2]
 * (IP, QP of the epochs of this call; may be NULL), records[n_chans][max_epochs] (may be NULL), n_epochs_out[n_chans] (epochs
 * run by this call).  params NULL: the defaults.  One wave64 per channel on the device; the _device form takes device pointers
 * for bits (4-byte aligned), prompt and records, host pointers for the rest, and returns after completion.
 */
GPSACQ_API int gpsacq_track(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, uint64_t first_sample, gpsacq_track_chan* chans,
                            int n_chans, const gpsacq_track_params* params, int32_t* prompt, gpsacq_track_record* records,
                            int max_epochs, int32_t* n_epochs_out);
GPSACQ_API int gpsacq_track_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, uint64_t first_sample, gpsacq_track_chan* chans,
                                   int n_chans, const gpsacq_track_params* params, void* d_prompt, void* d_records, int max_epochs,
                                   int32_t* n_epochs_out);
/*
 * NAV bits from the prompt I arm (host only).  ip[n_epochs] are consecutive epochs, the first being epoch first_epoch of the channel.
 * Bit sync: over the first sync_epochs epochs (all if <= 0 or more than given), the sign changes between epochs k-1 and k are
 * counted in bin (first_epoch + k) % 20; the fullest bin wins (ties to the lowest), and if it holds fewer than twice the
 * runner-up, or no change was seen, there is no sync: returns GPSACQ_ERR_ARG with *n_bits = 0.  Then one bit per whole 20-epoch
 * window that starts at an epoch of the winning bin: 1 if the summed ip < 0, else 0 (the sign of the I arm; 180 degrees
 * ambiguous, resolved by the preamble).  bits[max_bits]; *bit_epoch0 = the channel epoch where bit 0 starts.
 */
GPSACQ_API int gpsacq_nav_bits(const int32_t* ip, int n_epochs, int first_epoch, int sync_epochs, uint8_t* bits, int max_bits,
                               int* bit_epoch0, int* n_bits);
/* one subframe found by gpsacq_nav_subframes */
typedef struct {
    int32_t bit_offset;     /* index of its first bit in the stream */
    int32_t inverted;       /* 1: found through the inverted preamble */
    uint32_t words[10];     /* the ten 24-bit data words d1..d24 (d1 = bit 23), D30* already removed */
    int32_t id;             /* subframe ID: word 2 bits 20-22 */
    int32_t tow;            /* TOW count: word 2 bits 1-17 */
} gpsacq_subframe;          /* 56 bytes */
/*
 * Subframes of a bit stream (0/1 per byte), scanned like CHANNEL::ParityCheck() (c/channel.cpp:329-353): at position i an upright
 * preamble 10001011 sets D29* = D30* = 0, an inverted one 01110100 sets both to 1, else i += 1.  Then ten 30-bit words are checked
 * with the parity equations of IS-GPS-200 Table 20-XIV (d_k = D_k ^ D30*, D29*, D30* of the previous word carried on); all pass: a
 * subframe, i += 300; word w (0-based) fails: *n_parity_fail += 1, i += 30 (w + 1).  Scanning stops when fewer than 300 bits are
 * left.  out[max_out] (more are counted in *n_out but not written).
 */
GPSACQ_API int gpsacq_nav_subframes(const uint8_t* bits, int n_bits, gpsacq_subframe* out, int max_out, int* n_out, int* n_parity_fail);
/*
 * gpsacq_generate_range with navigation data: satellite s is multiplied by nav[s * n_nav_bits + (floor(q / 20460) mod n_nav_bits)]
 * (+1 / -1), q being the chip count of gpsacq_generate's law (floor((m + code_phase) * 1.023e6 (1 + doppler / L1) / fs)), so a bit
 * lasts 20 code periods and bit 0 starts at q = 0; q < 0 counts backwards from the last bit (THE GENERATOR'S LAW, at gpsacq_sat).
 * nav == NULL: exactly gpsacq_generate_range.
 */
GPSACQ_API int gpsacq_generate_nav_range(gpsacq_engine* e, uint8_t* bits_out, size_t n_bytes, uint64_t first_sample, const gpsacq_sat* sats,
                                         int n_sats, const int8_t* nav, int n_nav_bits, float noise_sigma, uint64_t seed);
GPSACQ_API int gpsacq_generate_nav_range_device(gpsacq_engine* e, void* d_bits_out, size_t n_bytes, uint64_t first_sample,
                                                const gpsacq_sat* sats, int n_sats, const int8_t* nav, int n_nav_bits, float noise_sigma,
                                                uint64_t seed, int sync);

/*
 * ---- Tracking channels on an 8-bit IQ capture ---------------------------------------------------------------------------------
 *
 * gpsacq_iq8_input describes the capture as for gpsacq_search_iq8.  Two modes, chosen by in->multibit:
 *
 * GPSACQ_SAMPLES_SIGN: the reference's flow (README.md:83-115: convert to a 1-bit file, then run on it), bit for bit.  The window
 * is converted on the device into engine scratch -- iq_convert.hpp's arithmetic, once per call -- and the 1-bit channels of
 * gpsacq_track run on it: chans, prompt, records and n_epochs equal gpsacq_iq8_to_bits() of the capture followed by gpsacq_track()
 * on the same window, byte for byte; no 1-bit stream reaches the host.  in->first_sample is the mixer's n of iq[0] (normally equal
 * to the window's first_sample), in->total_samples the capture's length (bits past it read 0), in->mean_i / mean_q the mean of the
 * WHOLE capture.  The window's first_sample must be a multiple of 8 (the byte grid of the 1-bit stream).
 *
 * in->multibit != 0 (GPSACQ_SAMPLES_REAL and GPSACQ_SAMPLES_COMPLEX alike): MULTI-BIT COMPLEX CHANNELS (csrc/track_iq_kernels.hip around csrc/track_channel.hpp;
 * CPU model tests/c/track_model_iq.c).  THE CHANNEL MODEL above with the sample and the sums replaced by:
 *   sample         v_i = I - off - dc_i,  v_q = Q - off - dc_q;  off = 128 for GPSACQ_IQ_U8, 0 for GPSACQ_IQ_S8;  dc_i = nearbyint(mean_i),
 *                  dc_q = nearbyint(mean_q) (ties to even) when remove_dc, else 0.  Integers: |v| <= 256.  There is no floating-point
 *                  mixer: mix_hz is NOT applied to the samples, the channel's carrier NCO does that work (gpsacq_track_start_iq8);
 *                  in->fs, first_sample and total_samples are not read.
 *   sums           with C = 1 - 2 (cos bit), S = 1 - 2 (sin bit) (the two carrier bits exactly as defined above: the signs of cos
 *                  and of -sin) and h_X = 1 - 2 chip_X:
 *                      I_X = sum h_X (v_i C - v_q S),   Q_X = sum h_X (v_i S + v_q C),   X in E, P, L
 *                  -- the complex sample times the two-level exp(-i 2 pi ph).
 * Everything else (epoch length, NCO advance, AGC, FLL, Costas, DLL, aid, windows, LOST) is that text unchanged.  With v_q = 0 and
 * v_i = +-1 (= 1 - 2 x) the sums are the 1-bit model's.  |I_X|, |Q_X| <= 2 * 256 * 65535 < 2^26: gpsacq_track_record and prompt keep
 * their int32 layouts; the discriminator products are formed in 64 bits and shifted mod 2^64 as above.  The window may start at any
 * sample.
 *
 * gpsacq_track_iq8: iq[2 * n_samples] holds samples first_sample .. first_sample + n_samples - 1 as interleaved I, Q bytes; window
 * and resume semantics, outputs and params as gpsacq_track (every epoch that ends inside the window, first_sample <= next_sample,
 * chans read and written back, LOST stops a channel).  params NULL: gpsacq_track_default_params (sign mode) -- in multi-bit mode
 * params are required (gpsacq_track_default_params_iq8 needs the capture's RMS).  The _device form takes device pointers for iq
 * (16-byte aligned), prompt and records.
 */
GPSACQ_API int gpsacq_track_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, uint64_t first_sample,
                                gpsacq_track_chan* chans, int n_chans, const gpsacq_track_params* params, int32_t* prompt,
                                gpsacq_track_record* records, int max_epochs, int32_t* n_epochs_out);
GPSACQ_API int gpsacq_track_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, uint64_t first_sample,
                                       gpsacq_track_chan* chans, int n_chans, const gpsacq_track_params* params, void* d_prompt,
                                       void* d_records, int max_epochs, int32_t* n_epochs_out);
/* device time of the last gpsacq_track_iq8* call on this engine, milliseconds: the 8-bit -> 1-bit conversion (0 in multi-bit
 * mode) and the channel kernel.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_track_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* track_ms);
/*
 * A channel from a hit of gpsacq_search_iq8 (host arithmetic).  Sign mode: exactly gpsacq_track_start.  Multi-bit mode: the code
 * side is gpsacq_track_start's; the carrier NCO runs where the satellite sits IN THE RAW COMPLEX CAPTURE.  The search saw the
 * capture turned by exp(+2 pi i mix_hz n / fs) (iq_convert.hpp) and then, unless in->multibit == GPSACQ_SAMPLES_COMPLEX, through
 * Sample()'s LO exp(-2 pi i fc n / fs) (c/search_offline.cpp:143-153: I by the sign of cos, Q by the sign of -sin), so a hit at
 * lo_dop (gpsacq_handoff_engine) is a raw-capture frequency of
 *     f = lo_dop - mix_hz + fc        (GPSACQ_SAMPLES_COMPLEX: f = lo_dop - mix_hz, fc plays no part)
 * f may be negative or near zero: lo_rate and lo_nom >> 32 are the two's-complement word (uint32)(int64)llround(f / fs * 2^32),
 * lo_int = lo_nom = that word << 32 (the window tests of the model compare signed 64-bit differences, so they hold under the
 * wrap); |f| must stay below fs / 2.  lo_phase = next_sample * lo_rate (mod 2^32).
 */
GPSACQ_API int gpsacq_track_start_iq8(const gpsacq_engine* e, const gpsacq_iq8_input* in, int prn, const gpsacq_peak* peak,
                                      uint64_t block_first_sample, const gpsacq_track_params* params, gpsacq_track_chan* chan);
/*
 * Loop settings for multi-bit channels.  Both discriminators scale with the square of the correlation amplitude, which a 1-bit
 * capture fixes (the quantiser) and a multi-bit one does not: it scales with the sample RMS.  sample_rms = the RMS of v_i, v_q
 * over any stretch of the capture (gpsacq_iq8_accumulate_power / samples, less the squared mean when it is removed).  The result
 * is gpsacq_track_default_params with lo_ki, lo_kp, ca_ki, ca_kp, fll_k lowered by g and agc_lo, agc_hi multiplied by 2^g,
 *     g = round(log2(GPSACQ_TRACK_IQ8_GAIN * sample_rms^2)),   GPSACQ_TRACK_IQ8_GAIN = 4:
 * next to a 1-bit channel (prompt sum ~ n a sqrt(2 / pi) (2 / pi) for a signal of amplitude a in unit noise) a complex one at
 * RMS r collects ~ n a r (4 / pi) -- both arms, no limiter -- 2.5 r times the amplitude, 6.2 r^2 times its square (the CPU model on
 * synthetic captures gives 6.0 r^2).  A plain g = round(log2(sample_rms^2)) would leave every loop gain about six times a 1-bit
 * channel's and trip the AGC on the stronger satellites; the constant is therefore two bits more, 4, the power of two nearest
 * to 6.2, which puts the loops at the 1-bit channels' bandwidths.  g is clamped so that every shift stays in [0, 62] (lo_ki, lo_kp >= 1);
 * GPSACQ_ERR_UNSUPPORTED if it cannot be (sample_rms <= 0, not finite, or so large that a shift would go negative); *params is written only on success.  The smallest
 * shift is ca_ki, so that is g > ca_ki of gpsacq_track_default_params, log2(4 sample_rms^2) >= ca_ki + 1/2: a sample RMS above 152 /
 * 107 / 76 / 53 / 38 / 38 / 26.9 / 13.4 / 9.5 / 3.36 at fs = 2.046 / 2.8 / 4 / 5.456 / 6.5 / 8.184 / 10 / 16.368 / 20 / 40 MHz.
 */
#define GPSACQ_TRACK_IQ8_GAIN 4
GPSACQ_API int gpsacq_track_default_params_iq8(const gpsacq_engine* e, double sample_rms, gpsacq_track_params* params);
/* adds the exact integer sums of (I - off)^2 and (Q - off)^2 over n_samples of a host buffer to power[0..1] (host arithmetic, e may be NULL;
 * off as in gpsacq_iq8_accumulate_sums).  RMS of v over N samples: sqrt((power[0] + power[1]) / (2 N) - (dc_i^2 + dc_q^2) / 2). */
GPSACQ_API int gpsacq_iq8_accumulate_power(const gpsacq_engine* e, const void* iq, size_t n_samples, int format, uint64_t power[2]);
/*
 * Synthetic 8-bit complex capture at a residual IF, generated on the device (no reference counterpart; the source of the tests, of
 * tools/track_bench.py --input iq8 and of rtl-like test files): gpsacq_generate_nav_range's law -- gpsacq_sat, chips and
 * navigation bits as functions of the absolute sample index m -- with a complex carrier and complex noise,
 *     I + jQ = clamp(round(scale * (sigma (n_I + j n_Q) + sum a * nav * chip * exp(2 pi i ((if_hz + doppler) / fs * m + phase)))))
 * n_I, n_Q two independent unit-variance Gaussian streams, round = to nearest (ties to even), clamp to [-127, 127]; written as
 * interleaved bytes, GPSACQ_IQ_S8 as they are, GPSACQ_IQ_U8 plus 128.  iq_out[2 * n_samples] holds samples first_sample ..
 * first_sample + n_samples - 1 (any first_sample); deterministic in (seed, arguments).  The engine's fc plays no part.  A search
 * with mix_hz = fc - if_hz (GPSACQ_SAMPLES_SIGN / _REAL) or mix_hz = -if_hz (GPSACQ_SAMPLES_COMPLEX) reports lo_shift =
 * round(doppler * 40000 / fs) and the code phase of gpsacq_generate.  nav == NULL: no data.  Noise, chip count, carrier, rounding
 * and clamp sample by sample: THE GENERATOR'S LAW, at gpsacq_sat.
 */
GPSACQ_API int gpsacq_generate_iq8_range(gpsacq_engine* e, void* iq_out, size_t n_samples, uint64_t first_sample, int format, double if_hz,
                                         float scale, const gpsacq_sat* sats, int n_sats, const int8_t* nav, int n_nav_bits,
                                         float noise_sigma, uint64_t seed);
GPSACQ_API int gpsacq_generate_iq8_range_device(gpsacq_engine* e, void* d_iq_out, size_t n_samples, uint64_t first_sample, int format,
                                                double if_hz, float scale, const gpsacq_sat* sats, int n_sats, const int8_t* nav,
                                                int n_nav_bits, float noise_sigma, uint64_t seed, int sync);

/*
 * ---- Navigation solver: ephemeris, satellite state, batched position fixes ------------------------------------------------------
 *
 * Everything downstream of "the transmit time of every satellite at one receive instant": the work of the reference's
 * c/ephemeris.cpp (subframe fields, satellite position, clock correction) and of Solve() / LatLonAlt(), c/solve.cpp:137-293.
 * Taking those transmit times out of tracking channels (SNAPSHOT::GetClock(), c/solve.cpp:118-133) is the section after this one.
 *
 * EPHEMERIS (host only).  gpsacq_ephemeris_load folds the subframes 1, 2, 3 among sf[0..n-1] into *eph in the order given (IDs 4,
 * 5 and anything else are ignored; eph->prn and fields of subframes not seen are left as they are: zero the record first).  Field
 * positions, widths, signedness and scale factors are IS-GPS-200 Tables 20-I and 20-III over gpsacq_subframe.words[] (word w of
 * the ICD is words[w - 1], its bit b is bit 24 - b).  Each value is (integer field * its power of two), exact, and the semicircle
 * fields are then multiplied once by the GPS pi, 3.1415926535898.  iodc is the whole 10-bit field.
 * gpsacq_ephemeris_valid: 1 when subframes 1, 2, 3 are all loaded and (iodc & 0xff) == iode2 == iode3 != 0 (IS-GPS-200
 * 20.3.3.4.1; EPHEM::Valid()), else 0 (also for NULL).
 *
 * TIME.  A time of week is a pair (ms, frac): whole milliseconds 0 .. 604 799 999 and seconds in [0, 1e-3) -- a double of
 * seconds of week resolves 1.2e-10 s = 3.5 cm.  Times that feed the orbit (t - t_oe, t - t_oc) are formed from the integer
 * millisecond difference, folded into +-302 400 s, plus frac.  Inside a fix every time is an offset from the fix's earliest
 * transmit millisecond (differences folded the same way, so a fix may straddle the end of the week).
 *
 * SATELLITE STATE.  (tx_ms, tx_frac) is the UNCORRECTED satellite time, what a code replica shows.  With t_k from t_oe and t from
 * t_oc at that time, Kepler's equation E = M + e sin E is iterated from E = M until the step is below 1e-12 (30 passes at most) and
 *     clock_corr = a_f0 + a_f1 t + a_f2 t^2 + F e sqrt_a sin E - t_gd,      F = -4.442807633e-10.
 * The position is IS-GPS-200 Table 20-IV at the corrected time (t_k - clock_corr), ECEF metres at that time, with
 * mu = 3.986005e14, Omega_e-dot = 7.2921151467e-5.  An observation that is not usable (valid == 0, eph index outside
 * [0, n_eph), an ephemeris that is not valid, a negative or non-finite weight) gives an all-zero gpsacq_sat_state.  An ephemeris
 * whose t_oe or t_oc is 604 800 s or more -- the 16-bit fields reach 1 048 560 s -- names no instant of the week and counts as not
 * valid here, whatever gpsacq_ephemeris_valid says of its issue numbers.  An observation whose tx_frac is NaN or infinite is not
 * usable either, in the host forms and in the _device forms alike (it is no argument error: the host forms check the weights only).
 *
 * FIX.  Unknowns x, y, z and the receive time; start at the origin and at the mean corrected transmit time + 75 ms.  Per pass and
 * satellite: turn the satellite by theta = Omega_e-dot (t_tx - t_rx) about z, residual = c (t_rx - t_tx) - range, Jacobian row
 * (unit vector satellite -> receiver, c); weighted normal equations, solved by Cholesky with the time unknown in metres (c dt).
 * Every step is applied and counted in `iterations`; one whose position part is below 1e-4 m is the last (the iteration converges
 * quadratically, so what is left after it is far below the rounding; rms is that of the residuals the last step was made from).
 * 20 steps without that, a pivot that is not positive (below 1e-13 of its diagonal entry) or a non-finite step:
 * GPSACQ_FIX_NO_CONVERGE.  c = 2.99792458e8.
 * lat / lon / alt: LatLonAlt()'s iteration on WGS-84 (a = 6378137, e^2 = 0.00669437999014132), until alt moves less than 1e-9 m,
 * 10 passes at most.  lon = atan2(y, x) in (-pi, pi], taken as 2 atan2(y, x + p) where x >= 0 and as +-2 atan2(p - x, |y|) with the
 * sign of y where x < 0 (p = sqrt(x^2 + y^2); tan(lon / 2) = y / (x + p) = (p - x) / y, each used where its sum does not cancel): a
 * point with y == 0 and x < 0 lies on the antimeridian, lon = pi.  A fix that is not GPSACQ_FIX_OK has every double field 0 and
 * rx_ms = 0.
 *
 * gpsacq_sat_states: one state per observation.  gpsacq_fix_batch: obs[n_fix][sats_per_fix], one fix per row; unusable
 * observations are skipped.  A negative or non-finite weight is GPSACQ_ERR_ARG in the host forms; the _device forms (device
 * pointers for obs and out, eph stays a host pointer; work on the engine's stream, sync != 0 waits) cannot read the weights and
 * skip such an observation instead.  Two kernels (csrc/nav_kernels.hip): one lane per observation, then one lane per fix.
 */
typedef struct {
    int32_t prn;            /* 1..32 */
    int32_t have;           /* bit s-1 set: subframe s (1..3) has been loaded */
    uint32_t week, iodc, iode2, iode3, t_oc, t_oe;   /* t_oc, t_oe in seconds (field * 16) */
    int32_t tow;            /* TOW count of the last subframe loaded */
    int32_t reserved;
    double t_gd, a_f0, a_f1, a_f2;
    double c_rs, dn, m_0, c_uc, e, c_us, sqrt_a;
    double c_ic, omega_0, c_is, i_0, c_rc, omega, omega_dot, idot;
} gpsacq_ephemeris;         /* 192 bytes */
GPSACQ_API int gpsacq_ephemeris_load(gpsacq_ephemeris* eph, const gpsacq_subframe* sf, int n);
GPSACQ_API int gpsacq_ephemeris_valid(const gpsacq_ephemeris* eph);

typedef struct { int32_t eph; int32_t valid; int32_t tx_ms; int32_t reserved; double tx_frac; double weight; } gpsacq_obs;   /* 32 bytes */
typedef struct { double x, y, z; double clock_corr; } gpsacq_sat_state;                                                   /* 32 bytes */
#define GPSACQ_FIX_OK 0
#define GPSACQ_FIX_TOO_FEW 1      /* fewer than 4 usable observations */
#define GPSACQ_FIX_NO_CONVERGE 2  /* 20 iterations, singular normal matrix, or a non-finite step */
typedef struct {
    int32_t status, n_used, iterations, rx_ms;
    double rx_frac;               /* receive time = rx_ms, rx_frac, GPS time of week */
    double x, y, z;               /* ECEF, metres */
    double lat, lon, alt;         /* WGS-84, radians / metres */
    double rms;                   /* weighted rms of the last residuals, metres */
} gpsacq_fix;                     /* 80 bytes */
#define GPSACQ_FIX_MAX_SATS 12
GPSACQ_API int gpsacq_sat_states(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_obs,
                                 gpsacq_sat_state* out);
GPSACQ_API int gpsacq_sat_states_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_obs,
                                        void* d_out, int sync);
GPSACQ_API int gpsacq_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs /* [n_fix][sats_per_fix] */,
                                size_t n_fix, int sats_per_fix, gpsacq_fix* out);
GPSACQ_API int gpsacq_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                       int sats_per_fix, void* d_out, int sync);
/* device time of the two kernels of the last gpsacq_fix_batch* call on this engine, milliseconds (HIP events on its stream; waits
 * for them).  Either pointer may be NULL. */
GPSACQ_API int gpsacq_fix_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* fix_ms);

/*
 * ---- Observables: transmit times from tracking channels -----------------------------------------------------------------------
 *
 * The step between the tracking channels and the solver: SNAPSHOT::GetClock(), c/solve.cpp:118-133, adds TOW x 6 s + buffered bits
 * x 20 ms + ms since the last bit + code chips + code NCO phase.  An offline channel has the same five terms: a TIME TAG gives
 * the first, the epoch count the second and third, the prompt code position P the last two.  THE MODEL; the kernels
 * (csrc/obs_kernels.hip) and the reference of the tests (tests/obs_ref.py) are both written from this text.  Integer arithmetic
 * up to one final division; "mod 2^64" is unsigned wrap-around.
 *
 * TIME TAG (host arithmetic, no device needed).  gpsacq_time_tag_from_subframe: bit_epoch0 is gpsacq_nav_bits's output -- the channel
 * epoch where bit 0 of the stream that sf->bit_offset indexes starts.
 *     epoch = bit_epoch0 + 20 * sf->bit_offset     the channel epoch whose start is the leading edge of the subframe's first bit
 *     ms    = ((tow - 1) mod 100800) * 6000        non-negative modulus: the HOW's TOW count names the start of the NEXT subframe
 *                                                  (IS-GPS-200 20.3.3.2), so tow = 0 gives 604 794 000
 *     eph   = eph_index                            the row of the caller's ephemeris table this channel's observations will name
 *     valid = 1
 * tow outside 0..100799 or a NULL pointer: GPSACQ_ERR_ARG.
 *
 * CODE POSITION PER EPOCH.  gpsacq_track_record holds `sample` and `ca_rate` but not ca_pos.  Inputs: records[c][0..n-1] of ONE
 * tracking call on channel c, chans[c] = the channel state AFTER that call (next_sample, ca_pos, epoch), n = n_epochs[c].  With
 *     end_t = records[c][t+1].sample for t < n-1,  end_{n-1} = chans[c].next_sample,      n_t = end_t - records[c][t].sample
 * the backward recursion, mod 2^64,
 *     pos_n = chans[c].ca_pos
 *     pos_t = pos_{t+1} + (1023 << 32) - n_t * ca_rate_t
 * is the channel loop's own update (THE CHANNEL MODEL: ca_pos += n * ca_rate - 1023 * 2^32) run in reverse, exact in integers:
 * pos_t is the prompt code position at records[c][t].sample.  first_epoch = chans[c].epoch - n is the epoch number of record 0.
 *
 * OBSERVATION of channel c at receive sample R (an absolute sample index).  With t such that records[c][t].sample <= R < end_t:
 *     P       = pos_t + (R - sample_t) * ca_rate_t          ( < 1023 * 2^32 by the channel model's n = ceil(...) )
 *     tx_ms   = (tag.ms + (first_epoch + t - tag.epoch)) mod 604800000      (non-negative; the difference may be negative)
 *     tx_frac = (double)P / 4393751543808000.0
 *     eph = tag.eph, valid = 1, weight = 1.0, reserved = 0
 * The divisor is 1023 * 2^32 * 1000, a double without rounding, and P < 2^42 is one too: tx_frac is ONE IEEE division, in
 * [0, 1e-3).  (No fast-math flag in the build.)  An observation that cannot be made is 32 zero bytes: tag.valid == 0, n == 0, R
 * before record 0's sample, R at or past next_sample.  A LOST channel stays usable up to its last epoch.
 *
 * RECEIVE INSTANTS are an arithmetic sequence R_i = first_rx_sample + i * rx_step, i < n_fix, rx_step >= 1 (the last one must
 * fit 64 bits).  Row i of the output is obs[i][0..n_chans-1], channel c in column c: the [n_fix][sats_per_fix] layout of
 * gpsacq_fix_batch with sats_per_fix = n_chans, 1 <= n_chans <= GPSACQ_FIX_MAX_SATS.
 *
 * gpsacq_observables: records[n_chans][max_epochs] (row stride max_epochs, as gpsacq_track writes them), n_epochs[n_chans],
 * chans[n_chans], tags[n_chans], obs[n_fix][n_chans]; host pointers, returns after completion.  gpsacq_observables_device: records
 * and obs are device pointers (the records straight from gpsacq_track_device / gpsacq_track_iq8_device: 1-bit and multi-bit
 * channels write the same layout); n_epochs, chans and tags stay host pointers; work on the engine's stream, sync != 0 waits.
 * gpsacq_fix_track_device: the same followed by gpsacq_fix_batch_device on the same stream, no host copy in between; d_obs may
 * be NULL (engine scratch), d_fix[n_fix].  Argument errors -- a NULL pointer, n_chans outside 1..GPSACQ_FIX_MAX_SATS, rx_step == 0,
 * n_fix == 0, n_epochs[c] < 0 or > max_epochs, instants past 2^64 -- return GPSACQ_ERR_ARG, launch nothing and write nothing.
 * Two kernels: k_code_pos, one wave64 per channel, the suffix sum as a scan (pos[n_chans][max_epochs] in engine scratch);
 * k_observe, one lane per (instant, channel).
 */
typedef struct { int32_t epoch; int32_t ms; int32_t eph; int32_t valid; } gpsacq_time_tag;   /* 16 bytes */
GPSACQ_API int gpsacq_time_tag_from_subframe(const gpsacq_subframe* sf, int bit_epoch0, int eph_index, gpsacq_time_tag* tag);
GPSACQ_API int gpsacq_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                  const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                  uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, gpsacq_obs* obs);
GPSACQ_API int gpsacq_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                         const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                         uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, void* d_obs, int sync);
GPSACQ_API int gpsacq_fix_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                       const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                       uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, void* d_obs, void* d_fix, int sync);
/* device time of the two kernels of the last gpsacq_observables* / gpsacq_fix_track_device call on this engine, milliseconds (HIP
 * events on its stream; waits for them).  Either pointer may be NULL. */
GPSACQ_API int gpsacq_observables_last_ms(const gpsacq_engine* e, float* code_pos_ms, float* observe_ms);

/*
 * ---- Carrier observables: accumulated Doppler and Doppler per channel ----------------------------------------------------------
 *
 * Every gpsacq_track_record carries lo_rate, the carrier NCO word its epoch ran at.  A phase-locked Costas channel follows the
 * carrier to a fraction of a cycle (19 cm), so the sum of the NCO's advance is the carrier-phase observable.  THE MODEL; the
 * kernels (csrc/obs_kernels.hip: k_carrier_acc, k_observe_rate) and the reference of the tests (tests/rate_ref.py) are both
 * written from this text.  Integers up to the three fp64 operations of doppler_hz; n_t and end_t are those of CODE POSITION PER
 * EPOCH above.
 *
 * NOMINAL WORD.  nom_word[c] (uint32, cycles per sample * 2^32) is the carrier NCO word of zero Doppler.  For 1-bit and
 * sign-mode channels it is (uint32_t)((uint64_t)chan.lo_nom >> 32).  For multi-bit IQ channels chan.lo_nom is NOT it --
 * gpsacq_track_start_iq8 stores the word the channel STARTED at there -- and gpsacq_track_nominal_word_iq8(e, in, &word) gives it
 * (host arithmetic): gpsacq_track_start_iq8's formula at zero Doppler, f = -mix_hz + fc (GPSACQ_SAMPLES_COMPLEX: f = -mix_hz),
 * reduced into [-fs / 2, fs / 2) by whole multiples of fs, word = (uint32)(int64)llround(f / fs * 2^32) (two's complement when
 * negative).  In sign mode it returns (uint32)((fc / fs - floor(fc / fs)) * 2^32), cycles per sample mod 1: for fc < fs that
 * is gpsacq_track_start's lo_nom >> 32 to the bit.
 *
 * ACCUMULATED DOPPLER PER EPOCH.
 *     d_t     = (int64)(int32)(lo_rate_t - nom_word)       the difference wraps in 32 bits and is then sign-extended
 *     A_0     = 0
 *     A_{t+1} = A_t + n_t * d_t                            signed 64-bit (two's complement, mod 2^64)
 * A_t is the accumulated Doppler at records[c][t].sample in cycles * 2^32, counted from record 0 of this call; A_n is the value
 * at next_sample.  Over a run of epochs at constant lo_rate the low 32 bits of A plus n * nom_word advance as lo_phase does.
 *
 * RATE OBSERVATION of channel c at receive sample R, averaged over W = avg_samples >= 1 samples centred on R:
 *     R_a = R - floor(W / 2),   R_b = R_a + W
 *     A(X)       = A_t + (X - sample_t) * d_t               t the epoch that holds X: sample_t <= X < end_t
 *     D          = A(R_b) - A(R_a)
 *     doppler_hz = ((double)D * fs) / ((double)W * 4294967296.0)      product first, then the quotient; fs = the engine's
 *     adr        = A(R)
 *     valid = 1, weight = 1.0, reserved = 0
 * Under the tracking windows |D| < 2^53, so (double)D is exact and W * 2^32 is exact: one rounding in the product, one in the
 * quotient (no fast-math flag in the build).  The window is centred so that the average equals the instantaneous Doppler at R up to
 * the third derivative of the phase (the second cancels).  A rate observation that cannot be made is 32 zero bytes: no epochs; R,
 * R_a or R_b before record 0's sample (R < floor(W / 2) included); R or R_b at or past next_sample.  It needs no time tag.
 * SIGN: doppler_hz > 0 for an approaching satellite, for a capture whose spectrum is not inverted (an inverted one is the caller's
 * to negate).  adr carries no cycle-slip or half-cycle flag.
 *
 * gpsacq_rate_observables: gpsacq_observables's arguments without the tags, plus nom_words[n_chans] and avg_samples; the output
 * rate_obs[n_fix][n_chans] is index-parallel to gpsacq_obs.  The _device form takes device pointers for records and rate_obs.
 * Argument errors as for gpsacq_observables, avg_samples == 0 and nom_words == NULL included: GPSACQ_ERR_ARG, nothing launched,
 * nothing written.  Two kernels: k_carrier_acc, one wave64 per channel, the prefix sum as a scan (acc[n_chans][max_epochs + 1]
 * in engine scratch); k_observe_rate, one lane per (instant, channel).
 */
typedef struct { int32_t valid; int32_t reserved; int64_t adr; double doppler_hz; double weight; } gpsacq_rate_obs;   /* 32 bytes */
GPSACQ_API int gpsacq_track_nominal_word_iq8(const gpsacq_engine* e, const gpsacq_iq8_input* in, uint32_t* word);
GPSACQ_API int gpsacq_rate_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                       const gpsacq_track_chan* chans, const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample,
                                       uint64_t rx_step, size_t n_fix, uint64_t avg_samples, gpsacq_rate_obs* rate_obs);
GPSACQ_API int gpsacq_rate_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                              const gpsacq_track_chan* chans, const uint32_t* nom_words, int n_chans,
                                              uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, uint64_t avg_samples,
                                              void* d_rate_obs, int sync);

/*
 * ---- Velocity and clock drift -------------------------------------------------------------------------------------------------
 *
 * The reference stops at position; this is our own.  THE MODEL; the kernels (csrc/nav_kernels.hip: k_sat_state_rate, k_vel) and
 * tests/rate_ref.py are both written from this text.
 *
 * SATELLITE VELOCITY: the time derivative of IS-GPS-200 Table 20-IV at the corrected time t_k of SATELLITE STATE, with n the
 * corrected mean motion, phi = nu + omega, and E, r, u, i, Omega_k, x' = r cos u, y' = r sin u of that table:
 *     E'      = n / (1 - e cos E)
 *     nu'     = E' sqrt(1 - e^2) / (1 - e cos E)
 *     u'      = nu' (1 + 2 (c_us cos 2phi - c_uc sin 2phi))
 *     r'      = A e sin E E' + 2 nu' (c_rs cos 2phi - c_rc sin 2phi)
 *     i'      = idot + 2 nu' (c_is cos 2phi - c_ic sin 2phi)
 *     Omega_k' = omega_dot - Omega_e-dot
 *     x''     = r' cos u - y' u',      y'' = r' sin u + x' u'
 *     vx = x'' cos Omega_k - y'' cos i sin Omega_k + y' sin i sin Omega_k i' - Omega_k' y
 *     vy = x'' sin Omega_k + y'' cos i cos Omega_k - y' sin i cos Omega_k i' + Omega_k' x
 *     vz = y'' sin i + y' cos i i'
 * ECEF metres per second.  clock_drift = a_f1 + 2 a_f2 t + F e sqrt_a cos E E', with E, E' and t at the UNCORRECTED time, the
 * derivative of clock_corr as it is computed.  An observation that is not usable (SATELLITE STATE's rule) gives an all-zero
 * gpsacq_sat_rate.
 *
 * VELOCITY.  First order, in the ECEF frame frozen at the receive instant.  Per fix: its gpsacq_fix (anything but GPSACQ_FIX_OK:
 * GPSACQ_VEL_NO_FIX, n_used 0), its rows of gpsacq_obs and gpsacq_rate_obs.  A satellite is used where its gpsacq_obs is usable
 * and its rate observation has valid != 0, a finite weight >= 0 and a finite doppler_hz.  For satellite i, with r_s, v_s its state
 * and rate, t_tx its corrected transmit time, (r_r, t_rx) the fix, Omega_e = (0, 0, Omega_e-dot) and R(theta) the turn about z of FIX:
 *     theta_i  = Omega_e-dot (t_tx,i - t_rx)                        the millisecond difference folded, as everywhere
 *     r_i      = R(theta_i) r_s,i
 *     v_i      = R(theta_i) (v_s,i + Omega_e x r_s,i)               inertial velocity expressed in that frame
 *     e_i      = (r_i - r_r) / |r_i - r_r|
 *     rho'_i   = -(c / L1) doppler_hz_i                             L1 = 1575.42e6
 *     rho'_i   = e_i . (v_i - (v_r + Omega_e x r_r)) + c drift_r - c clock_drift_i
 * Unknowns v_r (ECEF, m/s) and c drift_r: linear, so ONE weighted least-squares solve with the rows (-e_i, 1), weights
 * gpsacq_rate_obs.weight, FIX's Cholesky and pivot test (a pivot below 1e-13 of its diagonal entry or a non-finite solution:
 * GPSACQ_VEL_SINGULAR).  Fewer than 4 satellites: GPSACQ_VEL_TOO_FEW.  rms = sqrt(sum w res^2 / sum w) of the residuals AFTER the
 * solve, m/s.  ve, vn, vu: v_r turned by the fix's lat / lon (east, north, up).  drift = drift_r is the fractional frequency
 * error of the SAMPLING clock as seen through the carrier: > 0 when the receiver's clock runs fast.  Terms of order rho'^2 / c
 * (below 3 mm/s) are left out.  Every double is 0 unless GPSACQ_VEL_OK.
 *
 * gpsacq_sat_rates: one rate per observation.  gpsacq_vel_batch: obs[n_fix][sats_per_fix], rate_obs[n_fix][sats_per_fix],
 * fixes[n_fix], out[n_fix]; it runs k_sat_state and k_sat_state_rate into engine scratch, then k_vel.  Host forms refuse a negative
 * or non-finite weight (GPSACQ_ERR_ARG); the _device forms (device pointers for obs, rate_obs, fixes and out) skip such a
 * satellite.  gpsacq_pvt_track_device: gpsacq_fix_track_device extended -- records -> observations and rate observations -> fixes
 * -> velocities on the engine's stream, no host copy in between; d_obs and d_rate_obs may be NULL (engine scratch); d_fix[n_fix]
 * is byte for byte what gpsacq_fix_track_device writes.  Argument errors: GPSACQ_ERR_ARG, nothing launched, nothing written.
 */
typedef struct { double vx, vy, vz; double clock_drift; } gpsacq_sat_rate;                                                   /* 32 bytes */
#define GPSACQ_VEL_OK 0
#define GPSACQ_VEL_TOO_FEW 1      /* fewer than 4 usable satellites */
#define GPSACQ_VEL_NO_FIX 2       /* the fix is not GPSACQ_FIX_OK */
#define GPSACQ_VEL_SINGULAR 3     /* singular normal matrix or a non-finite solution */
typedef struct {
    int32_t status, n_used;
    double vx, vy, vz;            /* ECEF, m/s */
    double ve, vn, vu;            /* east, north, up at the fix, m/s */
    double drift;                 /* fractional frequency error of the sampling clock */
    double rms;                   /* weighted rms of the residuals after the solve, m/s */
} gpsacq_vel;                     /* 72 bytes */
GPSACQ_API int gpsacq_sat_rates(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_obs,
                                gpsacq_sat_rate* out);
GPSACQ_API int gpsacq_sat_rates_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_obs,
                                       void* d_out, int sync);
GPSACQ_API int gpsacq_vel_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs,
                                const gpsacq_rate_obs* rate_obs, const gpsacq_fix* fixes, size_t n_fix, int sats_per_fix, gpsacq_vel* out);
GPSACQ_API int gpsacq_vel_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_rate_obs,
                                       const void* d_fixes, size_t n_fix, int sats_per_fix, void* d_out, int sync);
GPSACQ_API int gpsacq_pvt_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                       const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                       const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                       uint64_t avg_samples, void* d_obs, void* d_rate_obs, void* d_fix, void* d_vel, int sync);
/* device time of the new kernels of the last calls on this engine, milliseconds (HIP events on its stream; waits for them):
 * k_carrier_acc and k_observe_rate of the last gpsacq_rate_observables* / gpsacq_pvt_track_device, k_sat_state_rate and k_vel of the
 * last gpsacq_vel_batch* / gpsacq_pvt_track_device.  A pair whose call has not been made reads 0; neither made: GPSACQ_ERR_ARG.
 * Any pointer may be NULL. */
GPSACQ_API int gpsacq_velocity_last_ms(const gpsacq_engine* e, float* carrier_acc_ms, float* observe_rate_ms, float* sat_rate_ms, float* vel_ms);

/*
 * ---- Carrier-smoothed observables: code-minus-carrier, phase lock and slip resets ---------------------------------------------
 *
 * A fix made from gpsacq_observables carries the code loop's noise of one instant (metres); the carrier observable of the same
 * channel is clean to centimetres but has an unknown constant.  Their difference, code-minus-carrier, is that constant plus the
 * code's noise, so its mean over a window is the code's noise to take out: a box-window Hatch filter.  THE MODEL; the kernels
 * (csrc/smooth_kernels.hip) and the reference of the tests (tests/smooth_ref.py) are both written from this text.  Integer
 * arithmetic up to the one fp64 division of tx_frac; "mod 2^64" is unsigned wrap-around, "(int64)" reads such a value as two's
 * complement, floor(a / b) is the signed division rounded toward minus infinity.
 *
 * INPUTS: those of gpsacq_rate_observables plus the tags -- records[c][0..n-1] of ONE tracking call, n = n_epochs[c], chans[c]
 * after that call, tags[c], nom_words[c], the RECEIVE INSTANTS R_i = first_rx_sample + i * rx_step, i < n_fix -- and a
 * gpsacq_smooth_params.  Per channel, with FULL = 1023 * 2^32:
 *     cw  = (uint32)((uint64)chans[c].ca_nom >> 32)         the nominal code word
 *     S   = records[c][0].sample
 *     t, pos_t, P, first_epoch as in OBSERVATION;   A(R) as in RATE OBSERVATION
 *     sgn = -1 if params.invert != 0, else +1               (SIGN of Carrier observables: an inverted spectrum is the caller's to declare)
 *
 * USABLE INSTANT: tag.valid != 0, n > 0 and records[c][0].sample <= R_i < next_sample -- exactly the instants at which an
 * OBSERVATION can be made.  Any other instant is INVALID: its obs and its info are all-zero bytes.
 *
 * CODE-MINUS-CARRIER of a usable instant, in cycles * 2^32 (1540 carrier cycles per chip):
 *     Z_i = 1540 * ((first_epoch + t) * FULL + P - (R_i - S) * cw) - sgn * A(R_i)          mod 2^64
 * (first_epoch sign-extended to 64 bits).  The bracket is the code's advance over the nominal one, the same quantity A counts
 * for the carrier.  Only differences of Z are ever used, each read as int64.
 *
 * PHASE LOCK of a usable instant, when lock_epochs = L > 0: over the epochs u = t-L+1 .. t of this call's records,
 *     N = sum (ip_u^2 - qp_u^2),   D = sum (ip_u^2 + qp_u^2)        squares and sums in int64 (mod 2^64)
 *     locked iff t >= L-1 and D > 0 and N * lock_den >= D * lock_num       the two products in int64 (mod 2^64)
 * With |ip|, |qp| < 2^21 (1-bit channels: at most 65535) nothing wraps.  L = 0: every usable instant is locked.  A usable instant
 * that is not locked is UNLOCKED: its obs is the raw OBSERVATION, byte for byte what gpsacq_observables writes, its info has
 * flags = GPSACQ_SMOOTH_UNLOCKED and every other field 0.  (During FLL pull-in the ratio N / D swings to -0.8; a Costas loop
 * in lock keeps it above 0.85.)
 *
 * SEGMENTS.  A locked instant i starts a segment (flag GPSACQ_SMOOTH_RESET) iff i = 0, or instant i-1 is INVALID or UNLOCKED, or
 * jump > 0 and |(int64)(Z_i - Z_{i-1})| > jump (the difference INT64_MIN counts as greater).  s_i = the latest segment start
 * <= i, m_i = min(i - s_i + 1, window).
 *
 * SMOOTHING of a locked instant:
 *     D_i  = sum over j = i-m_i+1 .. i of (Z_j - Z_i)          mod 2^64, read as int64
 *          = (S_{i+1} - S_{i+1-m_i}) - m_i * Z_i  mod 2^64,    S_k = sum over j < k of Z_j mod 2^64, Z_j = 0 where j is not locked
 *     q_i  = floor(D_i / m_i)                                  cycles * 2^32: mean code-minus-carrier of the window minus Z_i
 *     c_i  = floor(q_i / 1540)                                 chips * 2^32
 *     P'   = (int64)P + c_i;   k = floor(P' / FULL);   P~ = P' - k * FULL          0 <= P~ < FULL
 *     tx_ms   = (tag.ms + (first_epoch + t + k - tag.epoch)) mod 604800000         non-negative, as in OBSERVATION
 *     tx_frac = (double)P~ / 4393751543808000.0                                    the same single IEEE division
 *     eph = tag.eph, valid = 1, weight = 1.0, reserved = 0
 * Every j of the window is locked and inside i's segment, so the two forms of D_i are the same number mod 2^64 always; the sum of
 * the int64 differences (int64)(Z_j - Z_i) equals it without wrap-around while every |Z_j - Z_i| < 2^63 / m_i, which jump > 0
 * guarantees for jump * window^2 < 2^63 (the defaults: 2^41 * 10^6).  Z constant over the window gives q = c = 0 and the raw bytes.
 *
 * INFO per observation, index-parallel to obs: window = m_i; cmc = (int64)(Z_i - Z_{s_i}), code-minus-carrier since the segment
 * began; corr = q_i; flags = GPSACQ_SMOOTH_RESET (i = s_i) | GPSACQ_SMOOTH_FULL (m_i == window).
 *
 * PARAMETERS.  gpsacq_smooth_default_params: window 1000, lock_epochs 20, lock_num / lock_den 1 / 2, jump (int64)385 << 32 (a
 * quarter chip in cycles, half the early-late spacing), invert 0, reserved 0.  Valid: 1 <= window <= 65536, 0 <= lock_epochs
 * <= 1024, 1 <= lock_num <= lock_den <= 1024, jump >= 0 (0: no jump test); anything else is GPSACQ_ERR_ARG.
 *
 * NOTES.  A nominal word that is off by delta Hz (nom_words[c] and cw are truncated) drifts every channel's Z by delta cycles/s;
 * that is common to all channels and goes into the receiver clock only while the channels' windows are equal -- cmc shows it.
 * Half-cycle slips are invisible to the jump test: 9.5 cm against metres of code noise.  adr still carries no flag.  The standard
 * deviation of corr * (c / L1) / 2^32 over FULL windows is the measured pseudorange sigma of the channel (metres), the number
 * gpsacq_raim_default_params asks for.
 *
 * gpsacq_smooth_observables: host pointers; obs[n_fix][n_chans] in gpsacq_observables's layout, info[n_fix][n_chans] index-parallel
 * (may be NULL), params NULL = the defaults.  gpsacq_smooth_observables_device: records, obs and info are device pointers (d_info
 * may be NULL), the rest host pointers; work on the engine's stream, sync != 0 waits.  gpsacq_fix_smooth_track_device: the same
 * followed by gpsacq_fix_batch_device on the same stream, no host copy in between; d_obs and d_info may be NULL (engine scratch).
 * Argument errors are those of gpsacq_observables and gpsacq_rate_observables plus the parameter ranges: GPSACQ_ERR_ARG, nothing
 * launched, nothing written.  Kernels: k_code_pos and k_carrier_acc as they are, into the scratch they already use (their times stay
 * with gpsacq_observables_last_ms and gpsacq_velocity_last_ms, whose second kernels then read 0), then k_lock_acc (one wave64 per
 * channel: the prefix sums of ip^2 - qp^2 and ip^2 + qp^2; skipped when lock_epochs = 0), k_cmc (one lane per (instant,
 * channel): t, P, Z and the state), k_smooth_scan (one wave64 per channel: S and s_i over the instants, in chunks with a
 * carry) and k_smooth_out (one lane per (instant, channel): the two records).
 */
#define GPSACQ_SMOOTH_RESET 1      /* this instant starts a segment */
#define GPSACQ_SMOOTH_UNLOCKED 2   /* not phase-locked: obs is the raw observation */
#define GPSACQ_SMOOTH_FULL 4       /* the window has its full length */
typedef struct { int32_t window, lock_epochs, lock_num, lock_den; int64_t jump; int32_t invert, reserved; } gpsacq_smooth_params;   /* 32 bytes */
typedef struct { int32_t window; int32_t flags; int64_t cmc; int64_t corr; } gpsacq_smooth_info;                                   /* 24 bytes */
GPSACQ_API int gpsacq_smooth_default_params(gpsacq_smooth_params* p);   /* host only */
GPSACQ_API int gpsacq_smooth_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                         const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, const uint32_t* nom_words, int n_chans,
                                         uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, const gpsacq_smooth_params* params,
                                         gpsacq_obs* obs, gpsacq_smooth_info* info);
GPSACQ_API int gpsacq_smooth_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                                const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, const uint32_t* nom_words,
                                                int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                                const gpsacq_smooth_params* params, void* d_obs, void* d_info, int sync);
GPSACQ_API int gpsacq_fix_smooth_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                              const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                              const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                              const gpsacq_smooth_params* params, void* d_obs, void* d_info, void* d_fix, int sync);
/* device time of the four new kernels of the last gpsacq_smooth_observables* / gpsacq_fix_smooth_track_device call on this engine,
 * milliseconds (HIP events on its stream; waits for them); lock_acc_ms reads 0 when lock_epochs was 0.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_smooth_last_ms(const gpsacq_engine* e, float* lock_acc_ms, float* cmc_ms, float* scan_ms, float* out_ms);

/*
 * ---- Signal quality per observation: C/N0, phase lock and the weight of an observation ----------------------------------------
 *
 * Every solver here is a weighted least-squares solver and every observation maker above writes weight = 1.0.  This section makes
 * the weight: per channel and receive instant a carrier-to-noise density estimate from the prompt correlator sums, the phase-lock
 * ratio over the same window, and from the two a weight in [0, 1].  THE MODEL; the kernels (csrc/quality_kernels.hip) and the
 * reference of the tests (tests/quality_ref.py) are both written from this text.  Integers are uint64, "mod 2^64" is unsigned
 * wrap-around, "(int64)" reads such a value as two's complement; every floating-point step is ONE named IEEE double operation
 * (no fast-math flag and no contraction in the build).
 *
 * INPUTS: those of gpsacq_observables -- records[c][0..n-1] of ONE tracking call (1-bit or multi-bit: the layout is the same),
 * n = n_epochs[c], chans[c] after that call, tags[c], the RECEIVE INSTANTS R_i = first_rx_sample + i * rx_step, i < n_fix -- and
 * a gpsacq_quality_params.
 *
 * USABLE INSTANT: exactly OBSERVATION's: tag.valid != 0, n > 0 and records[c][0].sample <= R_i < next_sample; t is found by the
 * same rule, sample_t <= R_i < end_t.  Any other instant is INVALID: its info is 48 zero bytes (and its weight is 0).
 *
 * WINDOW of a usable instant: the epochs u = t-m+1 .. t, m = min(t + 1, params.epochs).  With ip_u, qp_u sign-extended to 64 bits,
 * products and sums mod 2^64:
 *     A     = sum |ip_u|
 *     D     = sum (ip_u^2 + qp_u^2)
 *     N     = sum (ip_u^2 - qp_u^2)
 *     sig   = A * A
 *     tot   = m * D
 *     noise = tot - sig
 * This is the signal-to-noise-variance estimator (Pauluzzi and Beaulieu, IEEE Trans. Commun. 48 (2000)): the squared mean of
 * |I_P| is the signal power (times m^2), the total prompt power less that is the noise power (times m^2).  The absolute value
 * takes the navigation bit out, so no bit synchronisation and nothing of the tag beyond `valid` is needed.  By Cauchy-Schwarz
 * A^2 <= m * sum ip^2 <= m * D, so noise >= 0 whenever nothing wraps, and nothing wraps while |ip|, |qp| < 2^21 and
 * epochs <= 1024 (the bound the smoothing text states; tot < 2^10 * 2^10 * 2^43 = 2^63) -- for 1-bit channels, |ip| <= 65535,
 * always.  Beyond that bound the arithmetic mod 2^64 still defines ONE answer, and that is the answer.
 *
 * VALUES.
 *     D == 0 or sig == 0:   flag GPSACQ_QUALITY_NO_POWER, lin = cn0_dbhz = weight = 0
 *     else noise == 0:      flag GPSACQ_QUALITY_SATURATED, lin = +infinity, cn0_dbhz = params.cn0_cap_dbhz
 *     else:                 snr      = (double)sig / (double)noise      both conversions uint64 -> double, round to nearest even;
 *                                                                       one division
 *                           lin      = snr * 1000.0                     one epoch is one code period, nominally 1000 per second;
 *                                                                       the Doppler stretch of a few ppm is ignored
 *                           cn0_dbhz = 10.0 * log10(lin)
 * D, sig and noise are compared as uint64 ("D == 0" is all 64 bits zero).  info.sig and info.noise hold sig and noise as computed,
 * in every one of the three cases.
 *
 * LOCK.  locked iff D != 0 and (int64)(N * lock_den) >= (int64)(D * lock_num): the products of the smoothing section's PHASE
 * LOCK, taken over this window (which may be shorter than params.epochs).  Not locked: flag GPSACQ_QUALITY_UNLOCKED.
 *
 * WINDOW LENGTH.  Flag GPSACQ_QUALITY_FULL when m == params.epochs, flag GPSACQ_QUALITY_SHORT when m < params.min_epochs.
 *
 * WEIGHT.  weight = 0 if NO_POWER, or SHORT, or UNLOCKED with params.require_lock != 0, or lin < params.cn0_min_lin.  Otherwise
 *     w      = lin / params.cn0_ref_lin            one division (+infinity stays +infinity)
 *     weight = w < 1.0 ? w : 1.0                   SATURATED gives 1.0
 * The gate and the weight read lin, never cn0_dbhz, so every field but cn0_dbhz is reproducible byte for byte; log10 is the only
 * libm call.  The weight is proportional to C/N0 up to the reference level -- the thermal-noise law of a delay-locked loop's range
 * variance -- and sigma_m of gpsacq_raim_default_params is then the pseudorange sigma at cn0_ref.
 *
 * INFO per (instant, channel), gpsacq_quality_info, 48 bytes: epochs = m, flags, sig, noise, lin, cn0_dbhz, weight.
 *
 * THE OBSERVATION.  When a gpsacq_obs array made for the SAME instants is given (raw or smoothed; valid and usable then coincide),
 * every observation with valid != 0 has its weight replaced by this weight.  No other byte of it is written, and an observation
 * with valid == 0 is not written at all.
 *
 * PARAMETERS.  gpsacq_quality_default_params (host only): epochs 200, min_epochs 20, lock_num / lock_den 1 / 2, require_lock 1,
 * reserved 0, cn0_min_lin 10^(30/10) = 1000.0, cn0_ref_lin 10^(45/10) (pow(10.0, 4.5)), cn0_cap_dbhz 99.0.  Valid:
 * 1 <= min_epochs <= epochs <= 1024, 1 <= lock_num <= lock_den <= 1024, cn0_min_lin finite and >= 0, cn0_ref_lin finite and > 0,
 * cn0_cap_dbhz finite; anything else is GPSACQ_ERR_ARG.  params NULL = the defaults.
 *
 * NOTES.  Noise alone (ip, qp independent, zero mean, equal variance) reads snr = (2/pi) / (2 - 2/pi) = 0.467: 26.7 dB-Hz is
 * the estimator's floor, no channel reads lower for long, and that is why the default gate sits at 30.  During FLL pull-in the
 * power is shared between the two arms, so the estimate reads LOW; that is what require_lock is for.  On 1-bit channels (and
 * sign-mode IQ channels) the samples have been through a hard limiter: this is the C/N0 AFTER the limiter, not the antenna's.
 *
 * gpsacq_quality_observables: host pointers, returns after completion; obs[n_fix][n_chans] in-out and may be NULL,
 * info[n_fix][n_chans] index-parallel.  gpsacq_quality_observables_device: records, obs (may be NULL) and info are device pointers,
 * the rest host pointers; work on the engine's stream, sync != 0 waits.  gpsacq_fix_quality_track_device: observations by
 * gpsacq_observables_device -- or, when smooth_params != NULL, by gpsacq_smooth_observables_device with those parameters; nom_words
 * is then required, otherwise it is not read -- then the weights, then gpsacq_fix_batch_device, all on the engine's stream with no
 * host copy in between; d_obs and d_info may be NULL (engine scratch), d_fix[n_fix].  Argument errors are those of
 * gpsacq_observables plus the parameter ranges (and info == NULL): GPSACQ_ERR_ARG, nothing launched, nothing written.  Two kernels:
 * k_quality_acc, one wave64 per channel, k_lock_acc's idiom: the prefix sums of |ip|, ip^2 + qp^2 and ip^2 - qp^2 over the epochs
 * ([3][n_chans][max_epochs + 1] in engine scratch of its own); k_quality_out, one lane per (instant, channel): the bisection for t,
 * the window sums as differences of prefix sums, the info record and the weight.
 */
#define GPSACQ_QUALITY_NO_POWER 1    /* D == 0 or sig == 0: nothing to estimate from */
#define GPSACQ_QUALITY_SATURATED 2   /* noise == 0: lin = +infinity, cn0_dbhz = cn0_cap_dbhz */
#define GPSACQ_QUALITY_UNLOCKED 4    /* the phase-lock ratio over the window is below lock_num / lock_den */
#define GPSACQ_QUALITY_FULL 8        /* the window has its full length */
#define GPSACQ_QUALITY_SHORT 16      /* the window is shorter than min_epochs */
typedef struct { int32_t epochs, min_epochs, lock_num, lock_den, require_lock, reserved; double cn0_min_lin, cn0_ref_lin, cn0_cap_dbhz; } gpsacq_quality_params;   /* 48 bytes */
typedef struct { int32_t epochs; int32_t flags; uint64_t sig; uint64_t noise; double lin; double cn0_dbhz; double weight; } gpsacq_quality_info;                     /* 48 bytes */
GPSACQ_API int gpsacq_quality_default_params(gpsacq_quality_params* p);   /* host only */
GPSACQ_API int gpsacq_quality_observables(gpsacq_engine* e, const gpsacq_track_record* records, int max_epochs, const int32_t* n_epochs,
                                          const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans, uint64_t first_rx_sample,
                                          uint64_t rx_step, size_t n_fix, const gpsacq_quality_params* params, gpsacq_obs* obs,
                                          gpsacq_quality_info* info);
GPSACQ_API int gpsacq_quality_observables_device(gpsacq_engine* e, const void* d_records, int max_epochs, const int32_t* n_epochs,
                                                 const gpsacq_track_chan* chans, const gpsacq_time_tag* tags, int n_chans,
                                                 uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix, const gpsacq_quality_params* params,
                                                 void* d_obs, void* d_info, int sync);
GPSACQ_API int gpsacq_fix_quality_track_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_records, int max_epochs,
                                               const int32_t* n_epochs, const gpsacq_track_chan* chans, const gpsacq_time_tag* tags,
                                               const uint32_t* nom_words, int n_chans, uint64_t first_rx_sample, uint64_t rx_step, size_t n_fix,
                                               const gpsacq_smooth_params* smooth_params, const gpsacq_quality_params* quality_params,
                                               void* d_obs, void* d_info, void* d_fix, int sync);
/* device time of the two kernels of the last gpsacq_quality_observables* / gpsacq_fix_quality_track_device call on this engine,
 * milliseconds (HIP events on its stream; waits for them).  Either pointer may be NULL. */
GPSACQ_API int gpsacq_quality_last_ms(const gpsacq_engine* e, float* acc_ms, float* out_ms);

/*
 * ---- Atmosphere, elevation mask and DOP ---------------------------------------------------------------------------------------
 *
 * gpsacq_fix_batch is the reference's bare Solve(): signals as if in vacuum, every satellite with an ephemeris used, no figure of
 * the geometry.  This section adds the Klobuchar ionosphere, a Saastamoinen troposphere, an elevation mask and the dilutions of
 * precision.  The reference decodes the ionospheric coefficients (EPHEM::LoadPage18, c/ephemeris.cpp:70-83) and never uses them;
 * the rest is our own.  THE MODEL; the kernels (csrc/fix_kernels.hip: k_sat_view, k_fix_atm) and tests/atm_ref.py are both
 * written from this text.  Nothing of the sections above changes: gpsacq_sat_states*, gpsacq_fix_batch*, gpsacq_vel_batch* compute what they did.
 *
 * PAGE 18 (host only).  gpsacq_iono_load folds, in the order given, every subframe of sf[0..n-1] whose ID (word 2, bits 20-22)
 * is 4 and whose word 3 starts with the eight bits 0x78 (data ID 01, SV/page ID 56: the test EPHEM::Subframe4 makes).  Such a
 * page sets valid = 1, tow = its TOW count (word 2, bits 1-17) and the eight coefficients; everything else is ignored and *io is
 * left as it was (zero the record first).  The fields are eight signed 8-bit integers, IS-GPS-200 Figure 20-1 sheet 8 and Table
 * 20-X, in the convention of EPHEMERIS above (ICD word w is words[w - 1], its bit b is bit 24 - b):
 *     alpha0, alpha1        word 3, bits 9-16 and 17-24       * 2^-30, 2^-27     seconds, seconds / semicircle
 *     alpha2, alpha3, beta0 word 4, bits 1-8, 9-16, 17-24     * 2^-24, 2^-24, 2^11
 *     beta1, beta2, beta3   word 5, bits 1-8, 9-16, 17-24     * 2^14, 2^16, 2^16
 * (LoadPage18's bytes nav[7..14]).  Each value is integer * power of two, exact.  The UTC parameters of the same page are not read.
 *
 * PARAMETERS.  gpsacq_atm_default_params: alpha / beta from *io when it is given and valid, else zeros; elev_mask = 5 degrees
 * (5 pi / 180 radians); flags = GPSACQ_ATM_IONO | GPSACQ_ATM_TROPO; reserved = 0.  Every entry point below checks its parameters:
 * elev_mask finite and in [-pi/2, pi/2) (-pi/2 masks nothing), no flag bit besides the two, finite alpha and beta; else
 * GPSACQ_ERR_ARG.  pi is the true one, 3.141592653589793, everywhere in this section.
 *
 * VIEW of a satellite from a receiver at ECEF r, with (lat, lon, alt) = FIX's LatLonAlt() iteration of r (on the axis, where
 * sqrt(x^2 + y^2) <= 1e-6: lon = 0, lat = +-pi/2, alt = |z| - a sqrt(1 - e^2); off it lon = atan2(y, x) in (-pi, pi] as FIX takes it, so
 * y == 0 with x < 0 is lon = pi, the antimeridian, and not 0).  alt is the height above the WGS-84 ellipsoid, not
 * above the geoid.  s is the satellite's state turned by theta = Omega_e-dot (t_tx - t_rx) about z exactly as FIX and VELOCITY turn
 * it, t_tx the corrected transmit time (tx - clock_corr).  d = s - r, and in the local frame (VELOCITY's rotation for ve, vn, vu)
 *     e = -sin lon dx + cos lon dy
 *     n = -sin lat cos lon dx - sin lat sin lon dy + cos lat dz
 *     u =  cos lat cos lon dx + cos lat sin lon dy + sin lat dz
 *     az = atan2(e, n)  in (-pi, pi],       el = atan2(u, hypot(e, n)).
 *
 * IONOSPHERE: IS-GPS-200 Figure 20-4, angles in semicircles.  With E = el / pi, phi_u = lat / pi, lambda_u = lon / pi and tow the
 * receive time of week in seconds (rx_ms * 1e-3 + rx_frac):
 *     psi      = 0.0137 / (E + 0.11) - 0.022
 *     phi_i    = phi_u + psi cos az,                      clamped to +-0.416
 *     lambda_i = lambda_u + psi sin az / cos(phi_i pi)
 *     phi_m    = phi_i + 0.064 cos((lambda_i - 1.617) pi)
 *     t        = 4.32e4 lambda_i + tow,   t = t - 86400 floor(t / 86400)             in [0, 86400)
 *     F        = 1 + 16 (0.53 - E)^3
 *     AMP      = ((alpha3 phi_m + alpha2) phi_m + alpha1) phi_m + alpha0,            0 where that is negative
 *     PER      = ((beta3 phi_m + beta2) phi_m + beta1) phi_m + beta0,                72000 where that is less
 *     x        = 2 pi (t - 50400) / PER
 *     iono_m   = c F (5e-9 + AMP (1 - x^2 / 2 + x^4 / 24))   where |x| < 1.57,   else c F 5e-9.
 * iono_m = 0 where el <= 0 or GPSACQ_ATM_IONO is off.  (The branch at |x| = 1.57 is the ICD's, and discontinuous.)
 *
 * TROPOSPHERE: Saastamoinen's zenith delay in a standard atmosphere (1013.25 hPa, 288.16 K - 6.5 K / km, 70 % humidity) over
 * sin el.  tropo_m = 0 where el <= 0, alt < -100, alt > 1e4 or GPSACQ_ATM_TROPO is off.  Else, with h = max(alt, 0):
 *     P = 1013.25 (1 - 2.2557e-5 h)^5.2568
 *     T = 288.16 - 6.5e-3 h
 *     e = 6.108 * 0.7 * exp((17.15 T - 4684) / (T - 38.45))
 *     tropo_m = (0.0022768 P / (1 - 0.00266 cos(2 lat) - 0.00028 h / 1000) + 0.002277 (1255 / T + 0.05) e) / sin el.
 *
 * CORRECTED FIX, per row of observations:
 *   0. FIX's iteration unchanged -- same start, same step rule, same failure tests -- over all usable observations.  A failure
 *      ends the fix with FIX's status (fewer than 4 usable: GPSACQ_FIX_TOO_FEW before any step).
 *   1. MASK.  At the position and receive time of stage 0, every used satellite with el < elev_mask is dropped, once and for all
 *      (the position is within tens of metres, 1e-6 rad of elevation: the mask is not evaluated again).  Fewer than 4 left:
 *      GPSACQ_FIX_TOO_FEW with n_used the number left.
 *   2. ROUNDS.  If nothing was dropped and flags == 0 the fix is done.  Else GPSACQ_ATM_ROUNDS = 3 rounds: at the current position
 *      and receive time compute every remaining satellite's D = iono_m + tropo_m, hold it, and run FIX's iteration FROM THE
 *      CURRENT STATE (not from the origin) with the residual  c (t_rx - t_tx) - D - range.  theta keeps the unmodified t_tx: the
 *      signal was under way for t_rx - t_tx.  Each round ends by its own step below 1e-4 m and has FIX's failure tests, 20 steps
 *      included; a failure is GPSACQ_FIX_NO_CONVERGE.  Why three: the altitude error of a round feeds the next round's tropospheric
 *      delay at 3e-4 m per metre, every round shrinks the distance to the model's fixed point about a thousandfold (2e-2, 2e-5,
 *      3e-8 m measured on the tests' constellation), and the solver is tested to 1e-4 m.
 *   3. OUTPUT.  gpsacq_fix as FIX writes it: n_used the satellites in the final solution, `iterations` every step of every stage,
 *      rms that of the residuals the last step was made from; not GPSACQ_FIX_OK: every double 0 and rx_ms = 0 (n_used and
 *      iterations stay).  gpsacq_fix_dop: used_mask has bit s set where observation s of the row is usable and was not dropped
 *      (whatever the status), n_masked is the number the mask dropped.
 * DOP.  At the final position and receive time, H has the rows (ux, uy, uz, 1), u the unit vector satellite -> receiver, over the
 * satellites of used_mask WITH WEIGHT > 0.  Q = (H^T H)^-1, unweighted, by FIX's Cholesky and pivot test.  With the local frame
 * of VIEW at the final position: pdop = sqrt(Qee + Qnn + Quu), hdop = sqrt(Qee + Qnn), vdop = sqrt(Quu), tdop = sqrt(Qtt) (the time
 * unknown in metres), gdop = sqrt(Qee + Qnn + Quu + Qtt) = sqrt(trace Q).  A failed pivot or a fix that is not OK: all five 0.
 *
 * gpsacq_sat_views: obs[n_fix][sats_per_fix] and one gpsacq_fix per row (its x, y, z, rx_ms, rx_frac and status are read; lat /
 * lon / alt are recomputed from x, y, z); out[n_fix][sats_per_fix].  An unusable observation or a fix that is not OK gives 32
 * zero bytes.  gpsacq_fix_atm_batch: k_sat_state, then k_fix_atm, then -- if views are wanted -- k_sat_view on the fixes just
 * written, so its views are exactly gpsacq_sat_views of its own fixes.  dop_out / views_out (d_dop / d_views) may be NULL.
 * Arguments, scratch, stream and events as gpsacq_fix_batch*: the host forms refuse a negative or non-finite weight, the _device
 * forms skip such an observation; params == NULL is GPSACQ_ERR_ARG.  A corrected gpsacq_fix goes into gpsacq_vel_batch* as it is.
 *
 * OUT OF SCOPE.  gps_track and the *_track_device chains stay on the plain fix: the signal generator puts no atmosphere on its
 * captures, where a corrected fix would only be worse, and a real capture needs up to 12.5 minutes for a page 18.  The UTC
 * parameters.  Dropping masked satellites from k_vel (the caller can clear `valid` from used_mask).
 */
typedef struct { int32_t valid; int32_t tow; double alpha[4]; double beta[4]; } gpsacq_iono;   /* 72 bytes */
GPSACQ_API int gpsacq_iono_load(gpsacq_iono* io, const gpsacq_subframe* sf, int n);
#define GPSACQ_ATM_IONO 1
#define GPSACQ_ATM_TROPO 2
#define GPSACQ_ATM_ROUNDS 3
typedef struct { double alpha[4], beta[4]; double elev_mask; int32_t flags; int32_t reserved; } gpsacq_atm_params;   /* 80 bytes */
GPSACQ_API int gpsacq_atm_default_params(const gpsacq_iono* io /* may be NULL or not valid: zeros */, gpsacq_atm_params* p);
typedef struct { double az, el, iono_m, tropo_m; } gpsacq_sat_view;                                                          /* 32 bytes */
typedef struct { uint32_t used_mask; int32_t n_masked; double gdop, pdop, hdop, vdop, tdop; } gpsacq_fix_dop;               /* 48 bytes */
GPSACQ_API int gpsacq_sat_views(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs /* [n_fix][sats_per_fix] */,
                                const gpsacq_fix* fix /* [n_fix] */, size_t n_fix, int sats_per_fix, const gpsacq_atm_params* params,
                                gpsacq_sat_view* out /* [n_fix][sats_per_fix] */);
GPSACQ_API int gpsacq_sat_views_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_fix,
                                       size_t n_fix, int sats_per_fix, const gpsacq_atm_params* params, void* d_out, int sync);
GPSACQ_API int gpsacq_fix_atm_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_fix,
                                    int sats_per_fix, const gpsacq_atm_params* params, gpsacq_fix* fix_out, gpsacq_fix_dop* dop_out,
                                    gpsacq_sat_view* views_out);
GPSACQ_API int gpsacq_fix_atm_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                           int sats_per_fix, const gpsacq_atm_params* params, void* d_fix, void* d_dop, void* d_views,
                                           int sync);
/* device time of the kernels of the last gpsacq_fix_atm_batch* call on this engine, milliseconds (HIP events on its stream; waits
 * for them); sat_view_ms reads 0 when that call asked for no views.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_fix_atm_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* fix_atm_ms, float* sat_view_ms);

/*
 * ---- Fix integrity: residual test and single-satellite exclusion ----------------------------------------------------------------
 *
 * Every solver above trusts every observation it is given: one transmit time that is off (a slipped code chip, a wrong time tag, a
 * cross-correlation lock) moves a fix by tens to hundreds of metres and nothing in the output says so.  The reference's answer is
 * LoadReplicas() (c/solve.cpp), which strips channels whose glitch counters moved; this section is our own: receiver autonomous
 * integrity monitoring (RAIM) on top of CORRECTED FIX -- a chi-square test of the residuals against an expected noise level and,
 * where it fails, the exclusion of the one observation whose removal explains the failure best.  THE MODEL; the kernels
 * (csrc/fix_kernels.hip: k_raim_detect, k_raim_exclude) and tests/raim_ref.py are both written from this text.  Nothing of the
 * sections above changes: their entry points compute what they did.
 *
 * PARAMETERS.  sigma_m is the standard deviation, in metres, of a pseudorange whose observation has weight 1; an observation of
 * weight w has variance sigma_m^2 / w.  threshold[d - 1] is the chi-square quantile with upper tail p_fa at d degrees of freedom.
 * gpsacq_raim_default_params (host only) computes the table from the closed-form tail for integer d; with h = x / 2
 *     even d:  Q_d(x) = e^-h sum_{j < d/2} h^j / j!
 *     odd d:   Q_d(x) = erfc(sqrt h) + e^-h sum_{j < (d-1)/2} h^(j + 1/2) / Gamma(j + 3/2)
 * and Q_d(x) = p_fa bisected on [0, 4000], 200 halvings; it sets exclude = 1 and reserved = 0 and keeps sigma_m and p_fa.  sigma_m
 * must be finite and > 0 and p_fa in [1e-15, 0.5]; anything else, or NULL: GPSACQ_ERR_ARG.  The kernels read only sigma_m,
 * threshold[] and exclude, so a caller may write thresholds of their own.  Every entry point below checks its parameters: sigma_m
 * and all eight thresholds finite and > 0, exclude 0 or 1; else GPSACQ_ERR_ARG and nothing is launched.  For p_fa = 1e-3 the
 * table is 10.827566170662733, 13.815510557964274, 16.26623619623813, 18.46682695290317, 20.515005652432876, 22.457744484825323,
 * 24.321886347856854, 26.12448155837614.
 *
 * STATISTIC, at a converged state (x, y, z, t_rx) over a satellite set S with held delays D_s:
 *     T(S) = sum_{s in S} w_s r_s^2 / sigma_m^2,       r_s = c (t_rx - t_tx,s) - D_s - range_s
 * with the residuals recomputed AT the state after the last step (not gpsacq_fix.rms's "residuals the last step was made from").
 * dof(S) = (number of s in S with w_s > 0) - 4.  Weight-0 observations stay in the solution as they do in FIX: they add nothing
 * to T, do not count, and are never exclusion candidates.
 *
 * PER ROW:
 *   1. FULL.  CORRECTED FIX, stages 0-2 of the section above, unchanged: status, the set S after the mask, the state, and the
 *      delays of the last round (with flags == 0 and nothing masked: zeros).  Not GPSACQ_FIX_OK: gpsacq_fix and gpsacq_fix_dop as
 *      gpsacq_fix_atm_batch writes them, raim status GPSACQ_RAIM_NONE.
 *   2. TEST.  d = dof(S).  d < 1: GPSACQ_RAIM_UNCHECKED, the outputs are the full solution.  T(S) <= threshold[d - 1]:
 *      GPSACQ_RAIM_PASS.
 *   3. EXCLUDE.  If exclude == 0 or d < 2: GPSACQ_RAIM_FAILED, the outputs are the full solution.  Otherwise, for every k in S
 *      with w_k > 0, FIX's Newton iteration over S \ {k}: from the full solution's state, with the full solution's delays held,
 *      with FIX's step rule and failure tests.  A candidate that fails is not a candidate.  T_k is the statistic at its converged
 *      state.  The winner is the smallest T_k, on a tie the lowest k.  No candidate, or T_k > threshold[d - 2]:
 *      GPSACQ_RAIM_FAILED, the outputs are the full solution.
 *   4. FINAL.  From the winner's state GPSACQ_ATM_ROUNDS rounds over S \ {k}, stage 2 of CORRECTED FIX: delays at the current
 *      state, then Newton from the current state.  A failure here: fix status GPSACQ_FIX_NO_CONVERGE (every double 0, n_used and
 *      iterations stay), raim status GPSACQ_RAIM_NONE with excluded = k.  If flags == 0 and the elevation mask dropped nothing,
 *      the winner's state is final and no round runs.  The mask is not evaluated again.  Status GPSACQ_RAIM_EXCLUDED;
 *      gpsacq_fix holds the final state with n_used one less; `iterations` counts the steps of FULL, of the winning candidate and
 *      of FINAL (not the losing candidates'); gpsacq_fix_dop has bit k cleared in used_mask and its DOP over the final set.
 *
 * gpsacq_fix_raim: dof, stat and threshold describe the solution that was output -- PASS and FAILED: d, T(S), threshold[d - 1];
 * UNCHECKED: d (0 or less), T(S), 0; EXCLUDED: d - 1, T_k recomputed at the FINAL state with FINAL's delays, threshold[d - 2].
 * stat_full is T(S) of step 2.  excluded is the observation's column in the row, or -1.  n_candidates is the number of subset
 * solves that converged, 0 if step 3 did not run.  GPSACQ_RAIM_NONE: every other field 0, excluded -1 unless FINAL failed.
 *
 * gpsacq_fix_raim_batch: k_sat_state as it is; k_raim_detect, one lane per fix (k_fix_atm's algorithm plus the statistic and the
 * test; it writes fix, dop and raim of every row, and for the rows that go on to step 3 a record in engine scratch: state, t0,
 * set and the twelve delays); k_raim_exclude, sixteen lanes per fix, lane k < 12 solving the subset without observation k, the
 * minimum found by a reduction across the sixteen lanes, the winning lane running FINAL and overwriting the row's three records.
 * k_raim_exclude is always launched (whether a row was flagged is known on the device only); a group whose row needs no exclusion
 * returns at once, so exclude_ms is small but never 0.  Arguments, scratch, stream, events and weights as gpsacq_fix_atm_batch*:
 * the host form refuses a negative or non-finite weight, the _device form skips such an observation; dop_out (d_dop) may be NULL,
 * fix and raim may not; either params pointer NULL is GPSACQ_ERR_ARG.  Argument errors launch nothing and write nothing.
 *
 * OUT OF SCOPE.  More than one exclusion per fix.  Protection levels.  k_vel: the caller clears `valid` from used_mask, as before.
 * gps_track and the *_track_device chains: nobody has measured the pseudorange sigma of our tracked channels, and a threshold
 * without it is a guess.
 */
#define GPSACQ_RAIM_MAX_DOF 8     /* GPSACQ_FIX_MAX_SATS - 4 */
typedef struct { double sigma_m; double p_fa; double threshold[GPSACQ_RAIM_MAX_DOF]; int32_t exclude; int32_t reserved; } gpsacq_raim_params; /* 88 bytes */
GPSACQ_API int gpsacq_raim_default_params(double sigma_m, double p_fa, gpsacq_raim_params* p);   /* host only */
#define GPSACQ_RAIM_NONE 0        /* no fix to judge */
#define GPSACQ_RAIM_UNCHECKED 1   /* no redundancy: dof < 1 */
#define GPSACQ_RAIM_PASS 2
#define GPSACQ_RAIM_EXCLUDED 3    /* the test failed, one observation was dropped and the rest pass */
#define GPSACQ_RAIM_FAILED 4      /* the test failed and no single exclusion mends it (or none was tried) */
typedef struct { int32_t status, dof, excluded, n_candidates; double stat_full, stat, threshold; } gpsacq_fix_raim;   /* 40 bytes */
GPSACQ_API int gpsacq_fix_raim_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs, size_t n_fix,
                                     int sats_per_fix, const gpsacq_atm_params* atm_params, const gpsacq_raim_params* raim_params,
                                     gpsacq_fix* fix_out, gpsacq_fix_dop* dop_out, gpsacq_fix_raim* raim_out);
GPSACQ_API int gpsacq_fix_raim_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, size_t n_fix,
                                            int sats_per_fix, const gpsacq_atm_params* atm_params, const gpsacq_raim_params* raim_params,
                                            void* d_fix, void* d_dop, void* d_raim, int sync);
/* device time of the kernels of the last gpsacq_fix_raim_batch* call on this engine, milliseconds (HIP events on its stream; waits
 * for them): k_sat_state, k_raim_detect, k_raim_exclude.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_fix_raim_last_ms(const gpsacq_engine* e, float* sat_state_ms, float* detect_ms, float* exclude_ms);

/*
 * ---- Coarse-time fixes: positions from code phases alone -----------------------------------------------------------------------
 *
 * Everything above starts from tracking records: a channel runs for 19 s and decodes subframes 1-3 before the first transmit
 * time exists.  A search peak gives only the code phase, the transmit time modulo one millisecond.  With ephemerides from
 * elsewhere and a rough idea of place and time (the PRIOR) that is enough: the whole milliseconds follow from the prior, and the
 * unknown error of the prior's time becomes a fifth unknown of the solve.  Every block of a capture is its own fix.  THE MODEL;
 * the kernels (csrc/coarse_kernels.hip) and the reference of the tests (tests/coarse_ref.py) are both written from this text.
 *
 * INPUTS.  eph[n_eph] as for gpsacq_fix_batch.  obs[n_fix][sats_per_fix] of gpsacq_obs, of which only eph, valid, tx_frac and
 * weight are read: tx_frac in [0, 1e-3) is the sub-millisecond part of the uncorrected satellite time that the replica shows at
 * the receive instant; tx_ms is ignored.  USABLE here: usable as in "Navigation solver" and also 0 <= tx_frac < 1e-3.
 * prior[n_fix] of gpsacq_coarse_prior: a place (ECEF metres) and a receive time t0 = (rx_ms, 0), rx_ms in 0 .. 604 799 999.  A
 * prior whose rx_ms is outside the week or whose place is not finite is GPSACQ_ERR_ARG in the host form; the _device form cannot
 * read it and treats every observation of that row as not usable.  gpsacq_coarse_params: rms_max_m, finite and > 0;
 * gpsacq_coarse_default_params (host only) sets it to c / 1.023e6 = 293.05 m, one C/A chip.  Times below are seconds from t0; an
 * absolute time is (rx_ms + whole milliseconds, fraction), split by FIX's rule (k = floor(1e3 t), frac = t - 1e-3 k, moved by one
 * millisecond where rounding left frac outside [0, 1e-3)), and the orbit folds it against t_oe and t_oc as everywhere else.
 * R(a) turns a vector about z by the angle a: (x cos a - y sin a, x sin a + y cos a, z).
 *
 * A. WHOLE MILLISECONDS.  Per fix, over the usable observations in column order, f_k = tx_frac:
 *      pass 1: the satellite position at the uncorrected time -75e-3, turned by R(-Omega_e 75e-3); tau = its distance to the
 *              prior's place / c.
 *      pass 2: position and clock correction cc at the uncorrected time -tau, turned by R(-Omega_e tau); tau' = distance / c.
 *      P_k = cc - tau'                                    the uncorrected satellite time the prior predicts, from t0
 *    The reference r is the first usable column:
 *      N_r = nearbyint((P_r - f_r) 1e3),   delta = N_r 1e-3 + f_r - P_r
 *    every other column
 *      N_k = nearbyint((delta + P_k - f_k) 1e3)
 *    and T_k = N_k 1e-3 + f_k for all of them.  (nearbyint: to nearest, ties to even.)  delta absorbs what is common to all
 *    satellites -- the receiver's clock and the mean of the prior's errors -- so only the DIFFERENCES between satellites have to
 *    stay below half a millisecond.  An error dp of the prior's place moves P_k - P_r by at most 2 |dp| / c, an error dt of its
 *    time by at most 1600 m/s |dt| / c (twice the largest range rate): every N_k is right up to one common integer while
 *        2 |dp| + 1600 m/s |dt| < 150 km       (c x 0.5 ms).
 *    Beyond that it depends on the geometry.  A common integer is one millisecond of receive time and is found by the solve.
 *
 * B. FIVE UNKNOWNS: x, y, z, b (metres) and s (seconds, the correction of the prior's time).  Start at the prior's place with
 *    b = s = 0.  Per pass and satellite: position p, clock correction cc, ECEF velocity v and clock drift d at the uncorrected
 *    time T_k + s (v and d as in "Velocity and clock drift", SATELLITE RATE), then
 *      rho   = c (cc - T_k) - b
 *      theta = -Omega_e rho / c
 *      range = |x - R(theta) p|,   u = (x - R(theta) p) / range
 *      res   = rho - range
 *      h     = (u, 1, -(c d + u . R(theta) v))            so that res ~ h . (dx, db, ds)
 *    Weighted normal equations A = sum w h h^T, g = sum w h res, solved by a 5x5 Cholesky with FIX's pivot rule (a pivot below
 *    1e-13 of its diagonal entry: singular).  Every step is applied and counted in `iterations`; one with |dx| < 1e-4 m and
 *    |ds| < 1e-7 s is the last.  20 steps without such a one, a bad pivot, a non-finite step or |s| reaching half a week
 *    (302 400 s: no correction of a prior): GPSACQ_FIX_NO_CONVERGE.  Fewer than 5 usable observations: GPSACQ_FIX_TOO_FEW before
 *    any step.  (In A, an N_k that is not finite or beyond 1e6 -- an ephemeris that describes no orbit -- is taken as 0.)
 *    The receive time is t0 + s - b / c as (rx_ms, rx_frac); lat / lon / alt as in FIX; rms = sqrt(sum w res^2 / sum w) over the
 *    residuals the last step was made from.
 *
 * C. RECORDS.  Three per fix.
 *    gpsacq_fix as everywhere: not GPSACQ_FIX_OK means every double 0 and rx_ms = 0 (n_used and iterations stay).
 *    gpsacq_coarse_info: ref the reference column (-1: no usable observation); coarse_s = s; bias_m = b; pdop = sqrt of the trace
 *    of the position block of (H^T H)^-1 and cdop = sqrt of its s-s entry (seconds per metre), H the five-column rows h at the
 *    final state, unweighted, over the usable observations with weight > 0; both 0 where the Cholesky factor of H^T H fails or
 *    either is not finite.  flags: GPSACQ_COARSE_INCONSISTENT when n_used >= 6 and rms > rms_max_m -- with one satellite to spare
 *    a wrong millisecond or a false peak shows as kilometres of residual.  Not GPSACQ_FIX_OK: ref stays, everything else 0.
 *    Five satellites have no residual to judge, and the five-state normal matrix of even the best five of a constellation has a
 *    condition of 1e9 - 1e10: read pdop and cdop before trusting such a fix.
 *    obs_out[n_fix][sats_per_fix], optional: the usable observations of a GPSACQ_FIX_OK fix as ordinary observations -- eph and
 *    weight kept, valid = 1, (tx_ms, tx_frac) the split of t0 + T_k + s folded into the week -- everything else 32 zero bytes.
 *    They drop into gpsacq_fix_batch, gpsacq_fix_atm_batch, gpsacq_fix_raim_batch and gpsacq_sat_views unchanged.  At the optimum
 *    of the five-state problem the four-state normal equations hold, so gpsacq_fix_batch on obs_out returns the same place and
 *    receive time.  obs_out must not overlap obs.
 *
 * FROM PEAKS.  gpsacq_coarse_obs: peaks[n_fix][n_chans] of gpsacq_peak, task order with the block outer and the channel inner
 * (task b * n_chans + c = block b against the PRN of eph[c]), 1 <= n_chans <= GPSACQ_FIX_MAX_SATS.  ca_shift is the code position,
 * in samples, at the block's first sample, and THAT SAMPLE is the receive instant of the row.  Per (fix, channel)
 *      valid = snr >= snr_min and 0 <= ca_shift < fs / 1000,   eph = channel,   tx_frac = (double)ca_shift / fs,   weight = 1.0,
 *      tx_ms = reserved = 0;
 * an observation that is not valid is 32 zero bytes.  fs is the engine's.  A whole-sample code phase is off by up to one sample,
 * c / fs = 55 m of range at 5.456 MHz, so such fixes are good to 100-200 m with eight satellites; the code phase below a sample
 * is the business of "Fine code phases" further down, whose observations (gpsacq_coarse_obs_fine) enter here unchanged.
 *
 * gpsacq_coarse_fix_batch: host pointers, returns after completion; a negative or non-finite weight is GPSACQ_ERR_ARG; params
 * NULL means the defaults; obs_out may be NULL, fix_out and info_out may not.  gpsacq_coarse_fix_batch_device: obs, prior and the
 * three outputs are device pointers (d_obs_out may be NULL: the whole milliseconds then live in engine scratch, and the fixes are
 * the same byte for byte), eph stays a host pointer; work on the engine's stream, sync != 0 waits; a bad weight skips the
 * observation.  gpsacq_coarse_obs / _device likewise.  gpsacq_coarse_fix_peaks_device: k_coarse_obs then k_coarse_fix on the same
 * stream, no host copy in between; d_obs may be NULL (engine scratch).  Argument errors -- a NULL pointer, n_fix == 0,
 * sats_per_fix or n_chans outside 1..GPSACQ_FIX_MAX_SATS, a non-finite snr_min, rms_max_m not finite or <= 0 -- return
 * GPSACQ_ERR_ARG, launch nothing and write nothing.
 * Kernels (csrc/coarse_kernels.hip): k_coarse_obs, one lane per (fix, channel).  k_coarse_fix, one lane per fix: nothing of the
 * row is held in registers -- the satellite loop of every pass reads the observation back from memory, evaluates the orbit
 * (csrc/orbit_device.hpp, the one copy k_sat_state and k_sat_state_rate use) and adds into the 15 + 5 sums.
 *
 * OUT OF SCOPE.  Doppler-aided time.  gps_test and gps_track.  (Sub-sample code phases: "Fine code phases" below; a prior of place
 * from the capture's own Dopplers: "Cold snapshot fixes" further down; the correlator and gpsacq_peak stay as they are.)
 */
typedef struct { double x, y, z; int32_t rx_ms; int32_t reserved; } gpsacq_coarse_prior;                                    /* 32 bytes */
typedef struct { double rms_max_m; double reserved; } gpsacq_coarse_params;                                                  /* 16 bytes */
#define GPSACQ_COARSE_INCONSISTENT 1   /* n_used >= 6 and rms > rms_max_m */
typedef struct { int32_t ref; int32_t flags; double coarse_s, bias_m, pdop, cdop; } gpsacq_coarse_info;                     /* 40 bytes */
GPSACQ_API int gpsacq_coarse_default_params(gpsacq_coarse_params* p);   /* host only */
GPSACQ_API int gpsacq_coarse_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs /* [n_fix][sats_per_fix] */,
                                       const gpsacq_coarse_prior* prior, size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params,
                                       gpsacq_fix* fix_out, gpsacq_coarse_info* info_out, gpsacq_obs* obs_out);
GPSACQ_API int gpsacq_coarse_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_prior,
                                              size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* params, void* d_fix, void* d_info,
                                              void* d_obs_out, int sync);
GPSACQ_API int gpsacq_coarse_obs(gpsacq_engine* e, const gpsacq_peak* peaks /* [n_fix][n_chans] */, size_t n_fix, int n_chans, double snr_min,
                                 gpsacq_obs* obs);
GPSACQ_API int gpsacq_coarse_obs_device(gpsacq_engine* e, const void* d_peaks, size_t n_fix, int n_chans, double snr_min, void* d_obs, int sync);
GPSACQ_API int gpsacq_coarse_fix_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_peaks, size_t n_fix,
                                              int n_chans, double snr_min, const void* d_prior, const gpsacq_coarse_params* params, void* d_obs,
                                              void* d_fix, void* d_info, void* d_obs_out, int sync);
/* device time of k_coarse_obs and k_coarse_fix as last run on this engine, milliseconds (HIP events on its stream; waits for
 * them); a kernel that has not run reads 0.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_coarse_last_ms(const gpsacq_engine* e, float* obs_ms, float* fix_ms);

/*
 * ---- Coarse-time fix integrity: residual test and one-satellite exclusion ------------------------------------------------------
 *
 * gpsacq_coarse_fix_batch trusts every code phase it is given, and a code phase that is wrong -- a sidelobe at snr_min, a
 * cross-correlation peak of the aided searches -- is not the 150 m of a slipped chip that "Fix integrity" guards against: it is
 * up to half a millisecond, 150 km.  All the solver says of it is GPSACQ_COARSE_INCONSISTENT, and the row is lost.
 * gpsacq_fix_raim_batch on obs_out cannot mend the row either: the false observation has bent the fifth unknown s, every transmit
 * time of obs_out carries that s, and the other satellites are evaluated seconds from where they were.  This section is the
 * test and the exclusion on the coarse-time solve itself.  THE MODEL; the kernel (csrc/coarse_kernels.hip: k_coarse_exclude,
 * behind k_coarse_fix) and tests/coarse_raim_ref.py are both written from this text.  Nothing of the sections above changes:
 * gpsacq_coarse_fix_batch* computes what it did.
 *
 * INPUTS as for gpsacq_coarse_fix_batch, and a gpsacq_raim_params of "Fix integrity" (the same 88 bytes), of which sigma_m,
 * threshold[] and exclude are read.  sigma_m is the standard deviation, in metres, of the range a code phase of weight 1 stands
 * for (c times its error in seconds); a weight w means sigma_m^2 / w.  Five unknowns leave at most GPSACQ_FIX_MAX_SATS - 5 = 7
 * degrees of freedom, so only threshold[0..6] can be reached.  USABLE as in "Coarse-time fixes".  W is the sum of the weights of
 * the usable observations of the row, n_w the number of them with weight > 0.
 *
 * PER ROW:
 *   1. FULL.  The coarse-time fix of the row, steps A, B and C of "Coarse-time fixes" unchanged: the three records are those
 *      gpsacq_coarse_fix_batch writes.  Not GPSACQ_FIX_OK: raim status GPSACQ_RAIM_NONE.
 *   2. TEST.  d = n_w - 5 and
 *          T = rms^2 W / sigma_m^2,
 *      rms the value in FULL's gpsacq_fix record: sqrt(sum w res^2 / sum w) over the residuals the last step was made from.  No
 *      further pass over the orbits is made for it.  This is NOT the statistic of "Fix integrity", whose residuals are
 *      recomputed at the state after the last step: the two differ by what the last step moved the residuals, and that step is
 *      below 1e-4 m.  d < 1: GPSACQ_RAIM_UNCHECKED.  T <= threshold[d - 1]: GPSACQ_RAIM_PASS.  In both the outputs are FULL's.
 *   3. EXCLUDE.  exclude == 0 or d < 2: GPSACQ_RAIM_FAILED, the outputs are FULL's.  Otherwise there is one candidate for every
 *      usable column k with w_k > 0: the complete coarse-time fix of the row with column k taken as not usable -- from the
 *      prior, not from FULL's state, AND WITH STEP A DONE AGAIN, so that a candidate which drops the reference column takes the
 *      next usable one as its reference and rounds every whole millisecond against it.  (A false reference bends delta, and
 *      with it every N_k of FULL; nothing of FULL's whole milliseconds can be kept.)  A candidate that is not GPSACQ_FIX_OK is no
 *      candidate.  T_k = rms_k^2 (W - w_k) / sigma_m^2, rms_k the candidate's rms.  The winner is the smallest T_k, on a tie the
 *      lowest k.  No candidate, or T_k > threshold[d - 2]: GPSACQ_RAIM_FAILED, the outputs are FULL's.
 *   4. EXCLUDED.  gpsacq_fix, gpsacq_coarse_info and obs_out are the winner's: what gpsacq_coarse_fix_batch gives for the row with
 *      `valid` of column k cleared -- n_used one less, column k of obs_out 32 zero bytes, ref, pdop / cdop and
 *      GPSACQ_COARSE_INCONSISTENT the candidate's own.  `iterations` alone differs: it counts FULL's steps and the winner's (not
 *      the losing candidates'), as gpsacq_fix_raim_batch does.  Status GPSACQ_RAIM_EXCLUDED.
 *
 * gpsacq_fix_raim as in "Fix integrity": dof, stat and threshold describe the solution that was output -- PASS and FAILED: d, T,
 * threshold[d - 1]; UNCHECKED: d (0 or less), T, 0; EXCLUDED: d - 1, T_k, threshold[d - 2], excluded = k.  stat_full = T.
 * excluded is the column in the row, or -1.  n_candidates is the number of candidates that were GPSACQ_FIX_OK, 0 if step 3 did
 * not run.  GPSACQ_RAIM_NONE: every other field 0, excluded -1.
 * Weight-0 observations stay in the solves as they do in "Coarse-time fixes": they add nothing to rms or T, do not count in
 * n_w, and are never candidates.
 * What the test can do follows from d.  Eight and nine satellites (d = 3, 4): a false code phase is the one column whose
 * candidate passes.  Seven (d = 2): a candidate has ONE degree of freedom left, so the smallest T_k need not be the false
 * column's, as with six satellites in "Fix integrity".  Six (d = 1): every candidate would have zero residual; FAILED, none is
 * tried.  Five: UNCHECKED.
 *
 * gpsacq_coarse_raim_batch: host pointers, returns after completion.  gpsacq_coarse_raim_batch_device: obs, prior and the four
 * outputs are device pointers, eph and both params host pointers; work on the engine's stream, sync != 0 waits.  Arguments as
 * gpsacq_coarse_fix_batch* (coarse_params NULL means the defaults; obs_out / d_obs_out may be NULL and must not be obs; the host
 * form refuses a bad weight or prior, the _device form skips the observation or the row) and as gpsacq_fix_raim_batch* for the
 * raim parameters: raim_params NULL is GPSACQ_ERR_ARG, sigma_m and all eight thresholds finite and > 0, exclude 0 or 1.  raim_out
 * / d_raim may not be NULL.  Argument errors launch nothing and write nothing.  The two forms agree byte for byte.
 * Kernels (csrc/coarse_kernels.hip), two launches on the engine's stream.  k_coarse_fix as it is: FULL.  k_coarse_exclude, sixteen
 * lanes per fix and four fixes per wave64, always launched (whether a row was flagged is known on the device only): every lane
 * of a group reads FULL's record and makes the test; a group whose row needs no exclusion writes its raim record and returns,
 * so exclude_ms is small but never 0; otherwise lane k < sats_per_fix solves the row without column k -- the one solve of
 * k_coarse_fix with a column to skip, reading the caller's obs and working in a row of its own in engine scratch
 * ([n_fix][sats_per_fix][sats_per_fix] observations), because the candidates of a fix run side by side and their whole
 * milliseconds differ -- the smallest (T_k, k) and the count meet in a butterfly across the sixteen lanes, and the winning lane
 * alone writes the three records and copies its row to obs_out.  No LDS, no atomics, no barrier; every loop is bounded.
 *
 * OUT OF SCOPE.  More than one exclusion per fix.  Protection levels.  Exclusion where FULL itself is not GPSACQ_FIX_OK.  A sigma
 * of our own code phases: the caller passes one (README: 19.93 m whole-sample and 3.41 m fine were measured on the generated
 * scene at amplitude 0.2).  gps_test and gps_track.
 */
GPSACQ_API int gpsacq_coarse_raim_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs /* [n_fix][sats_per_fix] */,
                                        const gpsacq_coarse_prior* prior, size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* coarse_params,
                                        const gpsacq_raim_params* raim_params, gpsacq_fix* fix_out, gpsacq_coarse_info* info_out,
                                        gpsacq_obs* obs_out, gpsacq_fix_raim* raim_out);
GPSACQ_API int gpsacq_coarse_raim_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_prior,
                                               size_t n_fix, int sats_per_fix, const gpsacq_coarse_params* coarse_params,
                                               const gpsacq_raim_params* raim_params, void* d_fix, void* d_info, void* d_obs_out, void* d_raim,
                                               int sync);
/* device time of the two kernels of the last gpsacq_coarse_raim_batch* call on this engine, milliseconds (HIP events on its stream;
 * waits for them): k_coarse_fix, k_coarse_exclude.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_coarse_raim_last_ms(const gpsacq_engine* e, float* fix_ms, float* exclude_ms);

/*
 * ---- Fine code phases: search peaks refined below a sample --------------------------------------------------------------------
 *
 * A search peak carries its code phase in whole samples: tx_frac = ca_shift / fs is off by up to half a sample, 27 m of range at
 * 5.456 MHz (15.8 m rms).  gpsacq_refine goes back to the 1-bit capture for every hit: in the time domain it correlates a window
 * of consecutive blocks against early, prompt and late replicas at the hit's Doppler and reads the code phase below a sample off
 * the early and late amplitudes, as the DLL of THE CHANNEL MODEL does.  One 7.3 ms block does not beat the sample grid: thermal
 * noise and the 16-samples-per-3-chips staircase of fs = 5.456 MHz leave about 12 m.  Over ~100 ms the code Doppler slides the
 * replica across the staircase and averages it out: sixteen blocks leave about a fifth of the whole-sample error (simulated with
 * eight satellites at amplitude 0.2, noise sigma 1: 2.9 m rms against 15.8 m).  THE MODEL; the kernels (csrc/refine_kernels.hip)
 * and the reference of the tests (tests/refine_ref.py) are both written from this text.  Integer arithmetic "mod 2^N" is unsigned
 * wrap-around as in THE CHANNEL MODEL, whose carrier bits, chip table and sums are used.
 *
 * INPUTS.  bits[n_bytes]: the capture as gpsacq_search reads it, sample m is bit m % 8 of byte m / 8, 1 = negative.  stride: bytes
 * between blocks, 5000 <= stride <= 2^31, any value, odd ones included.  tasks[n_tasks] and peaks[n_tasks]: the task list given
 * to the search and the peaks it returned; tasks == NULL is the reference schedule, task t = (block t, PRN t % 32).
 * gpsacq_refine_params: blocks, 1 .. 64, the length of the window; min_segments >= 1; half_spacing_chips in [1/64, 0.5], the
 * distance d of the early and of the late replica from the prompt one; snr_min, finite.  gpsacq_refine_default_params (host only)
 * sets 16, 1, 0.25 and 25.0, the threshold of the search.
 *
 * PER TASK.  spm = gpsacq_info.num_lags, o = 8 block stride (the first sample of the block), FULL = 1023 * 2^32.
 * 1. NCO WORDS.  lo_rate and ca_rate are those of gpsacq_handoff_engine(e, peak, 0, .), the step of the engine's current Doppler
 *    grid included: lo_dop = lo_shift * step (on the reference grid lo_shift * fs / 40000), ca_dop = lo_dop / L1 * 1.023e6,
 *    lo_rate = (uint32)((fc + lo_dop) / fs * 2^32), ca_rate = (uint32)((1.023e6 + ca_dop) / fs * 2^32), every operation rounded
 *    by itself (no fused multiply-add).
 * 2. NOT A HIT (GPSACQ_FINE_NO_HIT): not snr >= snr_min; ca_shift outside [0, spm); block < 0 or prn outside 0 .. 31; o at or
 *    beyond sample 8 n_bytes; fc + lo_dop or 1.023e6 + ca_dop outside [0, fs); ca_rate == 0.  The record is then that flag and
 *    zeros.
 * 3. WINDOW AND SEGMENTS.  The window is the blocks * 40000 samples that start at o: contiguous in the stream, whatever the stride.
 *    It is cut into segments of spm samples, one nominal code period each:
 *      segments = min(floor(blocks * 40000 / spm), floor((8 n_bytes - o) / spm));
 *    the tail of the window is not used.  Fewer segments than the first term: GPSACQ_FINE_SHORT.  Fewer than min_segments:
 *    GPSACQ_FINE_FEW.  Nothing is read at or beyond byte n_bytes.
 * 4. SUMS.  D = (uint32)(half_spacing_chips * 2^32), P0 = (ca_shift * ca_rate) mod FULL.  For sample j of the window (the first is
 *    j = 0), which is sample o + j of the capture:
 *      carrier phase  ph = j * lo_rate (mod 2^32); cos bit and sin bit as in THE CHANNEL MODEL
 *      prompt         P = (P0 + j * ca_rate) mod FULL;  early E = (P + D) mod FULL;  late L = (P - D) mod FULL
 *      the chip at position X is chip[X >> 32]
 *    and per segment s (samples j = s spm .. (s + 1) spm - 1) the six sums I_X, Q_X, X in E, P, L, as in THE CHANNEL MODEL.
 *      early = sum over the segments of I_E^2 + Q_E^2,   prompt and late likewise,
 *    as uint64: a segment adds at most 2 spm^2, so nothing overflows.
 * 5. ESTIMATE, in fp64.  d = D / 2^32, a_E = sqrt((double)early), a_L = sqrt((double)late).  early + late == 0:
 *    GPSACQ_FINE_NO_POWER, offset_chips = tx_frac = 0.  Otherwise
 *      offset_chips = ((1 - d) * (a_E - a_L)) / (a_E + a_L)
 *    (early stronger = the signal's code is ahead, as in the DLL; the triangle's early and late arms are 1 - d -+ x at an offset
 *    x, so the ratio is x / (1 - d)),
 *      pos = P0 / 2^32 + offset_chips, moved once by +-1023 into [0, 1023),     tx_frac = pos / 1.023e6,
 *    and a tx_frac that is not < 1e-3 is 0.0.
 * 6. USABLE: the record carries none of GPSACQ_FINE_NO_HIT, GPSACQ_FINE_NO_POWER and GPSACQ_FINE_FEW.
 * The record is gpsacq_fine; a hit's record keeps lo_rate, ca_rate, the segment count and the three sums whatever its flags.
 *
 * OBSERVATIONS.  gpsacq_coarse_obs_fine: gpsacq_coarse_obs (FROM PEAKS, above) with fine[n_fix][n_chans] beside the peaks; valid
 * additionally needs a usable record whose tx_frac lies in [0, 1e-3), and tx_frac is the record's.  The observations drop into
 * gpsacq_coarse_fix_batch*, and its obs_out into gpsacq_fix_batch, gpsacq_fix_atm_batch and gpsacq_fix_raim_batch, all unchanged.
 *
 * gpsacq_refine: host pointers, returns after completion.  gpsacq_refine_device: bits, tasks, peaks and fine are device pointers
 * (bits at any byte address), params stays a host pointer (NULL: the defaults); work on the engine's stream, sync != 0 waits.
 * Neither form reads the task list on the host, so both report a task out of range as GPSACQ_FINE_NO_HIT, and they agree byte
 * for byte.  gpsacq_coarse_obs_fine / _device likewise.  gpsacq_coarse_fix_fine_device: k_refine, k_coarse_obs_fine and
 * k_coarse_fix on the same stream, capture, tasks and peaks to records, observations and fixes with no host copy in between;
 * tasks are block outer and channel inner (task b * n_chans + c, eph = c) as FROM PEAKS has them, n_tasks = n_fix * n_chans, the
 * observations' snr_min is refine_params' and d_fine and d_obs may be NULL (engine scratch).  Argument errors -- a NULL pointer,
 * n_tasks or n_fix == 0, n_bytes == 0, a parameter or the stride outside the bounds above, n_chans outside
 * 1..GPSACQ_FIX_MAX_SATS -- return GPSACQ_ERR_ARG, launch nothing and write nothing; an engine whose num_lags exceeds 65535, or
 * whose fs is below 1.138 MHz (1.023e6 / fs + 1 / 1540 > 0.9 chips per sample), is GPSACQ_ERR_UNSUPPORTED.
 * Kernel (csrc/refine_kernels.hip): k_refine, one workgroup of four wave64 per task; wave w takes segments w, w + 4, ..., lane l
 * the 32-sample words l, l + 64, ... of a segment, five masks and six popcounts per word as the tracking channels'; the 96 chips
 * of a word are bits of one 32-chip window cut out of the chip sequence in LDS; the squares are added as integers, so the record
 * does not depend on the order of anything.
 *
 * LIMITS OF THE MODEL.  The estimate is the mean offset over the window, carried to its first sample at the replica's rate: a
 * Doppler half a bin off (68 Hz at 5.456 MHz) moves it by at most 0.044 chips/s * T / 2, which is 0.75 m at 16 blocks.  The
 * triangle is linear only for |offset| <= d, and a 1-bit front end rounds its corners.  The segments are added non-coherently, so
 * data-bit flips and the half-bin carrier error cost little.  Subtracting the analytic noise floor from the three powers did not
 * help consistently in simulation and is left out.  For the peaks of plain 1-bit searches; those of gpsacq_search_iq8 go through
 * "Snapshot chain on an 8-bit IQ capture" below.
 *
 * OUT OF SCOPE.  Accumulated or re-aligned searches (gpsacq_set_noncoherent, creep compensation, block alignment), fs above
 * 10 MHz where ca_shift refers to block 0 of several passes, multi-GPU, gps_test and gps_track.  The correlator and gpsacq_peak
 * do not change.  (8-bit IQ captures: "Snapshot chain on an 8-bit IQ capture" below.)
 */
#define GPSACQ_FINE_NO_HIT 1     /* the peak is no hit, or its task or NCO words are out of range: the record is this flag and zeros */
#define GPSACQ_FINE_SHORT 2      /* the capture ends before the window does */
#define GPSACQ_FINE_NO_POWER 4   /* early + late == 0 */
#define GPSACQ_FINE_FEW 8        /* segments < min_segments */
typedef struct { int32_t blocks; int32_t min_segments; double half_spacing_chips; double snr_min; } gpsacq_refine_params;          /* 24 bytes */
typedef struct { int32_t flags, segments; uint32_t lo_rate, ca_rate; uint64_t early, prompt, late; double offset_chips, tx_frac; } gpsacq_fine; /* 56 bytes */
GPSACQ_API int gpsacq_refine_default_params(gpsacq_refine_params* p);   /* host only */
GPSACQ_API int gpsacq_refine(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks, const gpsacq_peak* peaks,
                             size_t n_tasks, const gpsacq_refine_params* params, gpsacq_fine* fine_out);
GPSACQ_API int gpsacq_refine_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks,
                                    size_t n_tasks, const gpsacq_refine_params* params, void* d_fine, int sync);
GPSACQ_API int gpsacq_coarse_obs_fine(gpsacq_engine* e, const gpsacq_peak* peaks /* [n_fix][n_chans] */, const gpsacq_fine* fine, size_t n_fix,
                                      int n_chans, double snr_min, gpsacq_obs* obs);
GPSACQ_API int gpsacq_coarse_obs_fine_device(gpsacq_engine* e, const void* d_peaks, const void* d_fine, size_t n_fix, int n_chans, double snr_min,
                                             void* d_obs, int sync);
GPSACQ_API int gpsacq_coarse_fix_fine_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes, size_t stride,
                                             const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                             const gpsacq_refine_params* refine_params, const void* d_prior, const gpsacq_coarse_params* params,
                                             void* d_fine, void* d_obs, void* d_fix, void* d_info, void* d_obs_out, int sync);
/* device time of k_refine and k_coarse_obs_fine as last run on this engine, milliseconds (HIP events on its stream; waits for
 * them); a kernel that has not run reads 0.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_refine_last_ms(const gpsacq_engine* e, float* refine_ms, float* obs_ms);

/*
 * ---- Snapshot signal quality: C/N0 and the weight of a code-phase observation ---------------------------------------------------
 *
 * gpsacq_coarse_obs and gpsacq_coarse_obs_fine write weight = 1.0, and a satellite that aided acquisition dug out 10 dB below the
 * search threshold then pulls on a fix as hard as one at 44 dB-Hz, though its fine code phase is three to four times as noisy.
 * This section is the snapshot chain's counterpart of "Signal quality per observation": a carrier-to-noise density estimate per
 * fine record and from it a weight in [0, 1].  Nothing goes back to the capture: gpsacq_refine kept the prompt power and the
 * segment count, and the noise floor of a +-1 stream is analytic.  THE MODEL; the kernel (csrc/snapq_kernels.hip) and the reference
 * of the tests (tests/snapq_ref.py) are both written from this text.  Integers are uint64; every floating-point step is ONE named
 * IEEE double operation (no fast-math flag and no contraction in the build).
 *
 * INPUTS.  fine[n_fix][n_chans]: the gpsacq_fine records, index-parallel with the peaks and the observations of
 * gpsacq_coarse_obs_fine.  spm = gpsacq_info.num_lags and fs are the engine's.  A gpsacq_snap_quality_params.
 *
 * PER (fix, channel).
 * 1. NO RECORD.  flags carries any of GPSACQ_FINE_NO_HIT, GPSACQ_FINE_NO_POWER, GPSACQ_FINE_FEW, or segments <= 0: the info is the
 *    flag GPSACQ_QUALITY_NO_RECORD and zeros (epochs included), and the weight is 0.
 * 2. FLOOR.  A segment of spm samples of a +-1 stream that is uncorrelated with the replica adds spm to E[I_P^2] and spm to
 *    E[Q_P^2] (the two-level carrier replicas are +-1 too), so
 *      floor = 2 * spm * segments          (uint64; spm and segments are below 2^31, nothing overflows)
 *      sig   = prompt > floor ? prompt - floor : 0
 *      noise = floor
 *    -- the floor = 2 * spm * segments of "Aided acquisition".
 * 3. sig == 0: flag GPSACQ_QUALITY_NO_POWER, lin = cn0_dbhz = weight = 0.
 * 4. Otherwise
 *      snr      = (double)sig / (double)floor       both conversions uint64 -> double, round to nearest even; one division
 *      lin      = snr * (fs / (double)spm)          one division, one product: a segment is spm / fs seconds
 *      cn0_dbhz = 10.0 * log10(lin)
 * 5. Flag GPSACQ_QUALITY_SHORT when segments < params.min_segments.
 * 6. WEIGHT.  weight = 0 if NO_RECORD, NO_POWER, SHORT or lin < params.cn0_min_lin.  Otherwise
 *      w      = lin / params.cn0_ref_lin            one division
 *      weight = w < 1.0 ? w : 1.0
 * 7. The gate and the weight read lin, never cn0_dbhz, so every field but cn0_dbhz is reproducible byte for byte; log10 is the
 *    only libm call.
 *
 * INFO per (fix, channel): the gpsacq_quality_info of "Signal quality per observation", 48 bytes, with epochs = segments (a segment
 * is one code period, as an epoch is), flags, sig, noise, lin, cn0_dbhz, weight.  GPSACQ_QUALITY_SATURATED, _UNLOCKED and _FULL
 * are never set here.
 *
 * THE OBSERVATION.  When a gpsacq_obs array obs[n_fix][n_chans] is given, every observation with valid != 0 has its weight replaced
 * by this weight.  No other byte of it is written, and an observation with valid == 0 is not written at all.
 *
 * PARAMETERS.  gpsacq_snap_quality_default_params (host only): min_segments 1, reserved 0, cn0_min_lin 500.0, cn0_ref_lin
 * 10^(43.5/10) (pow(10.0, 4.35)).  Valid: min_segments >= 1, cn0_min_lin finite and >= 0, cn0_ref_lin finite and > 0; anything else
 * is GPSACQ_ERR_ARG.  params NULL = the defaults.
 *   THE GATE.  For a stream uncorrelated with the replica prompt / floor has mean 1 and standard deviation 1 / sqrt(segments) (a
 *   chi-square with two degrees of freedom per segment), so lin of noise alone has standard deviation (fs / spm) / sqrt(segments):
 *   92 Hz at the default 117 segments, and the default gate of 500 Hz stands 5.4 of those above zero.  A caller with a shorter
 *   window sets the gate from this law themselves.
 *   THE REFERENCE LEVEL is what the amplitude-0.2 satellites of the bench scene read (43.6 dB-Hz simulated with tools/
 *   snap_quality_law.py); sigma_m of gpsacq_raim_params is then the fine code-phase sigma at that level.
 *
 * LIMITS OF THE MODEL.  This is the C/N0 AFTER the 1-bit limiter, not the antenna's.  The prompt replica sits at the peak's whole
 * sample: at 5.456 MHz that is up to 0.094 chips off, and the figure reads up to 0.9 dB low; half a Doppler bin costs another
 * 0.07 dB.  An aided peak is the largest of its hypotheses, so it reads slightly high.  The weights follow the measured range
 * variance of the fine code phase within a factor of about two, on the conservative side (amplitudes 0.2 .. 0.03 at 16 blocks:
 * variance ratio 1 .. 0.05, weight 1 .. 0.024), and make no claim below cn0_min_lin.
 *
 * OUT OF SCOPE.  Whole-sample observations without a fine record, per-observation sigmas in gpsacq_raim_params, gps_test and
 * gps_track.  The records of a multi-bit gpsacq_refine_iq8 ("Snapshot chain on an 8-bit IQ capture" below) do not belong here: the
 * analytic floor of step 2 is that of a +-1 stream, and their prompt power scales with the capture's amplitude.  Their floor is
 * measured: "Snapshot signal quality on an 8-bit IQ capture", gpsacq_snap_quality_iq8.
 *
 * gpsacq_snap_quality: host pointers, returns after completion; obs in-out and may be NULL.  gpsacq_snap_quality_device: fine, obs
 * (may be NULL) and info are device pointers, params stays a host pointer; work on the engine's stream, sync != 0 waits.  The two
 * agree byte for byte.  gpsacq_coarse_fix_quality_device: gpsacq_coarse_fix_fine_device with the weights between the observations
 * and the fix -- k_refine, k_coarse_obs_fine, k_snap_quality and k_coarse_fix on the engine's stream with no host copy in between;
 * d_qinfo[n_fix][n_chans] may be NULL (engine scratch), as d_fine and d_obs.  Argument errors -- a NULL fine or info, n_fix == 0,
 * n_chans outside 1..GPSACQ_FIX_MAX_SATS, a parameter out of range, and for the chain those of gpsacq_coarse_fix_fine_device --
 * return GPSACQ_ERR_ARG, launch nothing and write nothing.  Kernel (csrc/snapq_kernels.hip): k_snap_quality, one lane per
 * (fix, channel); no LDS, no atomics, no loop.
 */
#define GPSACQ_QUALITY_NO_RECORD 32  /* snapshot quality only: the fine record is not usable; the info is this flag and zeros */
typedef struct { int32_t min_segments, reserved; double cn0_min_lin, cn0_ref_lin; } gpsacq_snap_quality_params;   /* 24 bytes */
GPSACQ_API int gpsacq_snap_quality_default_params(gpsacq_snap_quality_params* p);   /* host only */
GPSACQ_API int gpsacq_snap_quality(gpsacq_engine* e, const gpsacq_fine* fine /* [n_fix][n_chans] */, size_t n_fix, int n_chans,
                                   const gpsacq_snap_quality_params* params, gpsacq_obs* obs /* in-out, or NULL */, gpsacq_quality_info* info);
GPSACQ_API int gpsacq_snap_quality_device(gpsacq_engine* e, const void* d_fine, size_t n_fix, int n_chans, const gpsacq_snap_quality_params* params,
                                          void* d_obs, void* d_info, int sync);
GPSACQ_API int gpsacq_coarse_fix_quality_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes,
                                                size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                const gpsacq_refine_params* refine_params, const gpsacq_snap_quality_params* quality_params,
                                                const void* d_prior, const gpsacq_coarse_params* params, void* d_fine, void* d_obs, void* d_qinfo,
                                                void* d_fix, void* d_info, void* d_obs_out, int sync);
/* device time of k_snap_quality as last run on this engine, milliseconds (HIP events on its stream; waits for them).  ms may be
 * NULL. */
GPSACQ_API int gpsacq_snap_quality_last_ms(const gpsacq_engine* e, float* ms);

/*
 * ---- Cold snapshot fixes: fine Doppler and a Doppler-only position solver ------------------------------------------------------
 *
 * The coarse-time solver wants a PRIOR: a place good to tens of kilometres (2 |dp| + 1600 m/s |dt| < 150 km, above).  A capture of
 * unknown origin has none, but its hits carry one: the Doppler of a satellite is the projection of a known velocity on the line
 * of sight, and a handful of them fix the receiver to a few kilometres once each is known to about 1 Hz.  A search peak knows its
 * Doppler to half a bin only (lo_shift in steps of fs / 40000, +-68 Hz at 5.456 MHz, some +-70 km of place per satellite), so
 * gpsacq_fine_doppler goes back to the capture as gpsacq_refine does and reads the carrier's turn from one code period to the next
 * off the prompt sums; gpsacq_doppler_fix_batch then solves place and clock drift from the Dopplers alone, from no place at all,
 * and hands gpsacq_coarse_fix_batch its prior.  Only the TIME has to be known, to about +-30 s.  THE MODEL; the kernels
 * (csrc/doppler_kernels.hip) and the reference of the tests (tests/dop_ref.py) are both written from this text.  Integer arithmetic
 * is exact (int64 / uint64, the bound is under OVERFLOW); every fp64 expression is evaluated as written, left to right, every
 * operation rounded by itself (no fused multiply-add).
 *
 * 1. FINE DOPPLER.  INPUTS are those of gpsacq_refine: bits, n_bytes, stride, tasks or NULL, peaks, n_tasks.  gpsacq_dopfine_params:
 * blocks, 1 .. 64, the length of the window; min_segments >= 2; snr_min, finite; coherence_min, finite and >= 0.
 * gpsacq_dopfine_default_params (host only) sets 16, 2, 25.0 and 0.0 (the coherence gate is off).
 * PER TASK.  spm, o and FULL as in "Fine code phases", PER TASK, whose steps 1 (NCO WORDS), 2 (NOT A HIT, here
 * GPSACQ_DOPFINE_NO_HIT) and 3 (WINDOW AND SEGMENTS, here GPSACQ_DOPFINE_SHORT and GPSACQ_DOPFINE_FEW) apply word for word, with
 * this section's blocks, min_segments and snr_min.  Then
 *   PROMPT SUMS.  P0 = (ca_shift * ca_rate) mod FULL.  For sample j of the window: carrier phase ph = j * lo_rate (mod 2^32), cos
 *     bit and sin bit as in THE CHANNEL MODEL; prompt position P = (P0 + j * ca_rate) mod FULL, chip[P >> 32].  Per segment s
 *     (samples j = s spm .. (s + 1) spm - 1) the two sums I_s, Q_s as in THE CHANNEL MODEL: exactly step 4's I_P and Q_P.  Q is
 *     the -sin arm, so with z = I + iQ a signal whose carrier lies df above the replica's turns z by +2 pi df T per segment.
 *   SQUARES, blind to the data bits (a bit flip negates z and leaves z^2):  A_s = I_s^2 - Q_s^2,  B_s = 2 I_s Q_s,  int64.
 *   LAG-1 SUMS over s = 1 .. segments - 1 (z_s^2 times the conjugate of z_(s-1)^2, and what bounds it):
 *       re    = sum (A_s A_(s-1) + B_s B_(s-1))                        int64
 *       im    = sum (B_s A_(s-1) - A_s B_(s-1))                        int64
 *       mag   = sum (I_s^2 + Q_s^2) (I_(s-1)^2 + Q_(s-1)^2)            uint64
 *     and over s = 0 .. segments - 1
 *       power = sum (I_s^2 + Q_s^2)                                    uint64
 *     With fewer than 2 segments re = im = mag = 0.
 *   OVERFLOW.  |I|, |Q| <= spm, so a term of re, im or mag is at most 4 spm^4 and there are fewer than blocks * 40000 / spm of
 *     them: an engine and parameters with blocks * 160000 * spm^3 >= 2^63 are GPSACQ_ERR_UNSUPPORTED (at spm = 10000: more than 57
 *     blocks).  So are the engines gpsacq_refine refuses (num_lags > 65535, fs below 1.138 MHz).
 *   ESTIMATE, in fp64.  mag == 0, or re == 0 and im == 0: GPSACQ_DOPFINE_NO_POWER and coherence = df_hz = doppler_hz = 0.  Otherwise
 *       T          = (double)spm / fs
 *       df_hz      = atan2((double)im, (double)re) / ((4 pi) T)        4 pi = 4.0 * 3.141592653589793
 *       coherence  = hypot((double)re, (double)im) / (double)mag       in (0, 1]: 1 for a noise-free steady turn
 *       doppler_hz = (((double)lo_rate * fs) / 2^32 - fc) + df_hz      the Doppler the replica really had, plus the rest
 *     unambiguous while |df| < 1 / (4 T) = 250 Hz; a bin is +-68 Hz.  Then GPSACQ_DOPFINE_WEAK where coherence < coherence_min
 *     (a NO_POWER record has coherence 0, so any coherence_min > 0 marks it).
 *   USABLE: the record carries none of GPSACQ_DOPFINE_NO_HIT, _NO_POWER, _FEW and _WEAK.
 * The record is gpsacq_dopfine; a NO_HIT record is that flag and zeros, every other keeps segments, lo_rate, ca_rate and the four
 * sums whatever its flags.
 * LIMITS.  Squaring a 1 ms sum costs 6 dB and more below about 12 dB of SNR per millisecond: for hits of the plain 1-bit search
 * (38 dB-Hz and up).  The estimate is the mean over the window; the Doppler's own rate (below 1 Hz/s) is not modelled.  Measured
 * with 116 lag-1 products at amplitude 0.2, noise sigma 1, over 16 384 hits: 1.26 Hz rms, 6.6 Hz worst, coherence 0.78 .. 0.95
 * (1.5 Hz had been expected).  WITHOUT noise |df| reads some 7 % low (4 Hz at 60 Hz): the hard-limited signal keeps its third
 * harmonic, which meets the third harmonic of the two-bit replica in a term that turns the other way; noise at the usual level
 * linearises the limiter and takes the term away (tests/test_doppler.py measures both).
 *
 * RATE OBSERVATIONS.  gpsacq_rate_obs_fine: peaks[n_fix][n_chans] and dopfine[n_fix][n_chans], block outer and channel inner as
 * FROM PEAKS of "Coarse-time fixes" has them.  Per (fix, channel): valid where snr >= snr_min and the record is usable and its
 * doppler_hz is finite; then valid = 1, reserved = 0, adr = 0, doppler_hz the record's, weight = 1.0.  Anything else is 32 zero
 * bytes.  The output is gpsacq_rate_obs, what gpsacq_vel_batch reads.
 *
 * 2. DOPPLER FIX.  INPUTS.  eph[n_eph] as for gpsacq_fix_batch.  obs[n_fix][sats_per_fix] of gpsacq_obs, of which ONLY eph and
 * valid are read (gpsacq_coarse_obs's output serves).  rate_obs[n_fix][sats_per_fix].  rx_ms[n_fix], int32 in 0 .. 604 799 999:
 * the prior of TIME only, the receive instant t0 = (rx_ms, 0).  gpsacq_doppler_fix_params: rms_max_mps, finite and > 0.
 * A column is USABLE where its eph is in 0 .. n_eph - 1, that ephemeris passes SATELLITE STATE's rule (gpsacq_ephemeris_valid),
 * valid != 0 in both records, doppler_hz is finite and the rate observation's weight is finite and >= 0.  A row whose rx_ms is
 * outside the week has no usable column.  n_used counts the usable columns; fewer than 4: GPSACQ_FIX_TOO_FEW, no step.
 * UNKNOWNS x, y, z (ECEF metres) and g = c drift_r (m/s).  Every usable column k carries a light time tau_k, 75e-3 s at first.
 * Omega = Omega_e-dot, c, L1 and R(a) as in "Coarse-time fixes" and VELOCITY.  SATELLITE of column k at light time tau: position p,
 * clock drift d and ECEF velocity v (SATELLITE STATE, SATELLITE RATE) at the uncorrected time -tau from t0, split by FIX's rule
 * into (rx_ms + whole milliseconds folded into the week, fraction); a = -Omega tau;
 *       r  = R(a) p,     vi = R(a) (v + (-Omega p_y, Omega p_x, 0))          the inertial velocity in the frame of t0
 *   START.  u = sum over the usable columns of r / |r|, each at tau = 75e-3.  |u| not >= 1e-6: GPSACQ_FIX_NO_CONVERGE.  Otherwise
 *     (x, y, z) = (6371000 u_x / |u|, 6371000 u_y / |u|, 6371000 u_z / |u|) and g = 0: the foot of the mean satellite direction.
 *   PASS.  Per usable column, in column order, with its satellite at tau_k:
 *       D     = r - (x, y, z),   range = |D|,   e = D / range  (every division by range is a product with 1 / range)
 *       w     = vi - (-Omega y, Omega x, 0)
 *       ew    = e . w
 *       pred  = (ew + g) - c d
 *       res   = -(c / L1) doppler_hz - pred
 *       h     = ( -(w - ew e) / range + (-Omega e_y, Omega e_x, 0),  1 )     so that res ~ h . (dx, dy, dz, dg)
 *       tau_k = range / c                                                    for the next pass
 *     (VELOCITY's equation with v_r = 0, differentiated by the place.)  Weighted normal equations A = sum w h h^T, b = sum w h res
 *     with w the rate observation's weight, FIX's 4x4 Cholesky and pivot rule.  rms = sqrt(sum w res^2 / sum w) of this pass.
 *     The step is applied and counted in `iterations`; one with |(dx, dy, dz)| < 1e-3 m is the last.  A bad pivot, a step that is
 *     not finite, |(x, y, z)| not <= 1e8 m after a step, or 20 steps without a last one: GPSACQ_FIX_NO_CONVERGE.
 *   RECORD gpsacq_doppler_fix.  GPSACQ_FIX_OK: x, y, z; lat, lon, alt as in FIX; drift = g / c; rms that of the last pass, m/s;
 *     pdop = sqrt of the trace of the position block of (H^T H)^-1, H the rows h of the last pass, unweighted, over the usable
 *     columns with weight > 0 -- metres of place per m/s of range rate -- and 0 where its Cholesky factor fails or it is not
 *     finite; flags = GPSACQ_DOPPLER_INCONSISTENT when n_used >= 5 and rms > rms_max_mps.  Any other status: every double and
 *     flags 0; n_used and iterations stay.
 *   PRIOR.  prior_out[n_fix] of gpsacq_coarse_prior: rx_ms the row's as given, reserved 0, and the place of a GPSACQ_FIX_OK row that
 *     is not INCONSISTENT; for every other row x = y = z = NaN, which gpsacq_coarse_fix_batch_device treats as a row with no
 *     usable observation.
 * gpsacq_doppler_fix_default_params (host only) sets rms_max_mps = 3.0 m/s, about 16 Hz.  Measured (tools/snapshot_bench.py --cold,
 * 2048 blocks x 8 satellites at amplitude 0.2, the time 20 s off): rms 0.08 .. 0.72 m/s, median 0.40; three times the largest is
 * 2.15 m/s, rounded up to one digit.  (2.0 m/s, the value first proposed from an expected 1.5 Hz per Doppler, is below that.)  One
 * Doppler 200 Hz off among eight leaves 3.3 m/s and more.
 * WHAT TO EXPECT (simulated, three geometries, drift 2e-6): 5-6 steps; exact Dopplers land 4-35 m from the truth; 1.5 Hz of noise
 * on eight satellites 2.4-3.0 km median and 6.3 km worst, on five 7 km median and 21 km worst; a time 30 s off moves the place by
 * up to 26 km with eight satellites and 64 km with five.  Eight satellites and +-30 s stay inside the coarse-time condition, five
 * do not always.  The receiver is taken to be at rest: 1 m/s of its own speed is some 5 Hz, kilometres of place.
 *
 * 3. THE CHAIN.  gpsacq_cold_fix_device: on the engine's stream, no host copy in between,
 *       k_fine_dop -> k_coarse_obs and k_rate_obs_fine -> k_doppler_fix -> k_refine -> k_coarse_obs_fine -> k_coarse_fix
 * from the capture, tasks, peaks (task b * n_chans + c = block b against the PRN of eph[c], n_tasks = n_fix * n_chans) and
 * d_rx_ms[n_fix] to d_fix, d_info (gpsacq_coarse_fix_batch's records) and d_doppler_fix.  Both snr_min of the observations are
 * their kernel's params' (dopfine_params for k_coarse_obs and k_rate_obs_fine, refine_params for k_coarse_obs_fine).  d_dopfine,
 * d_rate_obs, d_prior, d_fine, d_obs and d_obs_out may be NULL (engine scratch); d_obs holds k_coarse_obs's observations first and
 * k_coarse_obs_fine's in the end.  d_obs_out, d_rate_obs and d_fix go into gpsacq_vel_batch_device unchanged: a snapshot velocity
 * (and a second reading of the clock drift) comes for free.
 *
 * gpsacq_fine_doppler, gpsacq_rate_obs_fine, gpsacq_doppler_fix_batch: host pointers, return after completion; a negative or
 * non-finite weight or an rx_ms outside the week is GPSACQ_ERR_ARG in gpsacq_doppler_fix_batch.  The _device forms: device pointers
 * for everything but eph and the params (NULL: the defaults), bits at any byte address; work on the engine's stream, sync != 0
 * waits; a bad weight skips the column, a bad rx_ms the row; host and device form agree byte for byte.  Argument errors -- a NULL
 * pointer (prior_out and d_prior may be NULL), n_tasks or n_fix == 0, n_bytes == 0, a parameter or the stride outside its bounds,
 * n_chans or sats_per_fix outside 1..GPSACQ_FIX_MAX_SATS, d_obs_out == d_obs -- return GPSACQ_ERR_ARG, launch nothing and write
 * nothing.
 * Kernels (csrc/doppler_kernels.hip).  k_fine_dop: one workgroup of four wave64 per task with k_refine's word loop
 * (csrc/capture_words.hpp holds the one copy): three masks and two popcounts per word; every segment's (I, Q) goes into LDS as two
 * int32 (at most 64 * 40000 / 1137 = 2251 segments, 18 KB); after one barrier thread i takes s = i, i + 256, ...; the four sums
 * meet through integer shuffles and one LDS step.  No atomics, no float before the estimate: the record depends on the order of
 * nothing.  k_rate_obs_fine: one lane per (fix, channel).  k_doppler_fix: one lane per fix, nothing of the row in registers (the
 * light times live in engine scratch), the orbit from csrc/orbit_device.hpp.  Every loop is bounded by kernel arguments.
 *
 * OUT OF SCOPE.  Coherent sums longer than one code period and signals below about 38 dB-Hz (for satellites found from a first fix:
 * "Coherent aided acquisition" further down).  Doppler rate over the window.  A
 * height constraint for five-satellite rows.  Solving the time error from the Dopplers.  Fusing k_fine_dop into k_refine.
 * Accumulated or re-aligned searches, multi-GPU, gps_test and gps_track.  (8-bit IQ captures: "Snapshot chain on an 8-bit IQ
 * capture" below.)
 */
#define GPSACQ_DOPFINE_NO_HIT 1     /* the peak is no hit, or its task or NCO words are out of range: the record is this flag and zeros */
#define GPSACQ_DOPFINE_SHORT 2      /* the capture ends before the window does */
#define GPSACQ_DOPFINE_NO_POWER 4   /* mag == 0, or re == 0 and im == 0 */
#define GPSACQ_DOPFINE_FEW 8        /* segments < min_segments */
#define GPSACQ_DOPFINE_WEAK 16      /* coherence < coherence_min */
typedef struct { int32_t blocks; int32_t min_segments; double snr_min; double coherence_min; } gpsacq_dopfine_params;             /* 24 bytes */
typedef struct { int32_t flags, segments; uint32_t lo_rate, ca_rate; int64_t re, im; uint64_t mag, power;
                 double coherence, df_hz, doppler_hz; } gpsacq_dopfine;                                                          /* 72 bytes */
typedef struct { double rms_max_mps; double reserved; } gpsacq_doppler_fix_params;                                               /* 16 bytes */
#define GPSACQ_DOPPLER_INCONSISTENT 1   /* n_used >= 5 and rms > rms_max_mps */
typedef struct { int32_t status, n_used, iterations, flags; double x, y, z, lat, lon, alt, drift, rms, pdop; } gpsacq_doppler_fix; /* 88 bytes */
GPSACQ_API int gpsacq_dopfine_default_params(gpsacq_dopfine_params* p);            /* host only */
GPSACQ_API int gpsacq_doppler_fix_default_params(gpsacq_doppler_fix_params* p);    /* host only */
GPSACQ_API int gpsacq_fine_doppler(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks,
                                   const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_dopfine_params* params, gpsacq_dopfine* dopfine_out);
GPSACQ_API int gpsacq_fine_doppler_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks,
                                          const void* d_peaks, size_t n_tasks, const gpsacq_dopfine_params* params, void* d_dopfine, int sync);
GPSACQ_API int gpsacq_rate_obs_fine(gpsacq_engine* e, const gpsacq_peak* peaks /* [n_fix][n_chans] */, const gpsacq_dopfine* dopfine, size_t n_fix,
                                    int n_chans, double snr_min, gpsacq_rate_obs* rate_obs);
GPSACQ_API int gpsacq_rate_obs_fine_device(gpsacq_engine* e, const void* d_peaks, const void* d_dopfine, size_t n_fix, int n_chans, double snr_min,
                                           void* d_rate_obs, int sync);
GPSACQ_API int gpsacq_doppler_fix_batch(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_obs* obs /* [n_fix][sats_per_fix] */,
                                        const gpsacq_rate_obs* rate_obs, const int32_t* rx_ms, size_t n_fix, int sats_per_fix,
                                        const gpsacq_doppler_fix_params* params, gpsacq_doppler_fix* fix_out, gpsacq_coarse_prior* prior_out);
GPSACQ_API int gpsacq_doppler_fix_batch_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_obs, const void* d_rate_obs,
                                               const void* d_rx_ms, size_t n_fix, int sats_per_fix, const gpsacq_doppler_fix_params* params,
                                               void* d_doppler_fix, void* d_prior, int sync);
GPSACQ_API int gpsacq_cold_fix_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_bits, size_t n_bytes, size_t stride,
                                      const void* d_tasks, const void* d_peaks, const void* d_rx_ms, size_t n_fix, int n_chans,
                                      const gpsacq_dopfine_params* dopfine_params, const gpsacq_doppler_fix_params* doppler_params,
                                      const gpsacq_refine_params* refine_params, const gpsacq_coarse_params* coarse_params, void* d_dopfine,
                                      void* d_rate_obs, void* d_doppler_fix, void* d_prior, void* d_fine, void* d_obs, void* d_fix, void* d_info,
                                      void* d_obs_out, int sync);
/* device time of k_fine_dop, k_rate_obs_fine and k_doppler_fix as last run on this engine, milliseconds (HIP events on its
 * stream; waits for them); a kernel that has not run reads 0.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_doppler_last_ms(const gpsacq_engine* e, float* fine_dop_ms, float* rate_obs_ms, float* doppler_fix_ms);

/*
 * ---- Snapshot chain on an 8-bit IQ capture: multi-bit fine code phase and fine Doppler -------------------------------------------
 *
 * gpsacq_search_iq8 searches an rtl-sdr / HackRF file as it is and gpsacq_track_iq8 tracks it, but gpsacq_refine and
 * gpsacq_fine_doppler read a 1-bit real-IF stream: a snapshot fix from an 8-bit IQ file had to go through gpsacq_iq8_to_bits first,
 * which throws one arm away (3 dB) and puts the other through a limiter (about 2 dB), in the one chain whose point is to work with
 * little signal.  gpsacq_refine_iq8 and gpsacq_fine_doppler_iq8 go back to the IQ bytes themselves.  The records are gpsacq_fine and
 * gpsacq_dopfine as they are, and everything downstream takes them unchanged: gpsacq_coarse_obs_fine*, gpsacq_rate_obs_fine*,
 * gpsacq_doppler_fix_batch*, gpsacq_coarse_fix_batch*, gpsacq_coarse_raim_batch*, gpsacq_vel_batch*.  THE MODEL; the kernels
 * (csrc/snapshot_iq_kernels.hip) and the references of the tests (tests/refine_iq_ref.py, tests/dop_iq_ref.py) are both written
 * from this text.  "Step n" is step n of "Fine code phases", PER TASK.
 *
 * INPUTS.  A gpsacq_iq8_input `in`, as for gpsacq_search_iq8.  iq[2 * n_samples]: interleaved I, Q bytes, sample m in bytes 2 m and
 * 2 m + 1; the device form takes a 16-byte-aligned device pointer.  stride: BYTES between blocks with gpsacq_search_iq8's bounds, a
 * multiple of 16, 80000 <= stride <= 2^31.  tasks[n_tasks], or NULL for the reference schedule, and peaks[n_tasks] as returned by
 * gpsacq_search_iq8 with the same `in`.  gpsacq_refine_params / gpsacq_dopfine_params as they are.
 *
 * in->multibit != 0 (GPSACQ_SAMPLES_REAL and GPSACQ_SAMPLES_COMPLEX alike): THE MULTI-BIT PATH.
 *   SAMPLE.  v_i, v_q are exactly the sample of "Tracking channels on an 8-bit IQ capture": v_i = I - off - dc_i, v_q = Q - off - dc_q,
 *     off = 128 for GPSACQ_IQ_U8 and 0 for GPSACQ_IQ_S8, dc = nearbyint(mean) (ties to even) when remove_dc, else 0; |v| <= 256.  No
 *     floating-point mixer: mix_hz goes into the carrier word.  in->fs, first_sample and total_samples are not read.
 *   NCO WORDS.  lo_dop, ca_dop and ca_rate are step 1's.  The carrier word is gpsacq_track_start_iq8's, where the satellite sits in
 *     the raw capture:
 *         f = lo_dop - mix_hz + fc      (GPSACQ_SAMPLES_COMPLEX: f = lo_dop - mix_hz), left to right,
 *         lo_rate = (uint32)(int64)llround(f / fs * 2^32)                 (round half away from zero; two's complement for f < 0)
 *   NOT A HIT is step 2 with `|f| >= fs / 2` (or f not a number) in place of the test of fc + lo_dop in [0, fs), and with o and the
 *     capture's length as below.
 *   WINDOW.  o = block * (stride / 2), the first sample of the block, against n_samples: a block at or beyond sample n_samples is no
 *     hit.  Segments, GPSACQ_FINE_SHORT and GPSACQ_FINE_FEW are step 3 word for word with n_samples for 8 n_bytes.  Nothing at or
 *     beyond byte 2 * n_samples is read.
 *   SUMS.  Chips at (P0 + j ca_rate -+ D) mod FULL and the carrier phase j lo_rate (mod 2^32) as in step 4; with C = 1 - 2 (cos bit),
 *     S = 1 - 2 (sin bit) and h_X = 1 - 2 chip_X, per segment the six sums of the multi-bit channel model,
 *         I_X = sum h_X (v_i C - v_q S),   Q_X = sum h_X (v_i S + v_q C),   X in E, P, L,
 *     and early = sum over the segments of I_E^2 + Q_E^2, prompt and late likewise, as uint64.  |I_X|, |Q_X| <= 512 spm < 2^25 (spm
 *     <= 65535), a segment adds less than 2^51 and there are fewer than 2^12 segments (64 * 40000 / 1137 = 2251): nothing overflows.
 *   ESTIMATE, FLAGS, USABLE.  Steps 5 and 6 unchanged.
 *   FINE DOPPLER (gpsacq_fine_doppler_iq8).  The prompt sums I_s = I_P, Q_s = Q_P of the segments go into the lag-1 law of "Cold
 *     snapshot fixes" with gpsacq_dopfine_params' blocks, min_segments and snr_min.  Its OVERFLOW bound (a term at most 4 spm^4) does
 *     not hold for 25-bit sums, so they are normalised first, exactly and in integers:
 *         M   = the largest |I_s| or |Q_s| over the segments
 *         k   = max(0, bitlength(M) - 12)                    bitlength(0) = 0, bitlength(4095) = 12, bitlength(4096) = 13
 *         I'_s = (I_s + 2^(k-1)) >> k                        arithmetic shift (floor); I_s itself when k = 0.  Q'_s likewise
 *     A, B, re, im and mag are formed from I', Q': |I'| <= 2^12, so |A|, |B| <= 2^25, a term is at most 2^50 and the sum of fewer than
 *     2^12 of them below 2^62.  There is no new GPSACQ_ERR_UNSUPPORTED case.  power stays the sum of the UNSHIFTED squares.  df_hz
 *     and coherence are ratios and do not see k (the shifted estimate differed from the unshifted one by at most 0.018 Hz in
 *     simulation, against an error of 0.6 to 4 Hz).  The Doppler is the search's own sense, the replica's frequency less what
 *     was not Doppler in it:
 *         doppler_hz = (((double)(int32)lo_rate * fs) / 2^32 - (f - lo_dop)) + df_hz
 *     (int32)lo_rate is the word read as two's complement; f - lo_dop is the fp64 difference of the two values above.
 *
 * in->multibit == GPSACQ_SAMPLES_SIGN: the capture is converted once per call into engine scratch, by the path
 * gpsacq_track_iq8_device uses (iq_convert.hpp's arithmetic, in->mean_i / mean_q, mix_hz, fs and first_sample as there), and the
 * 1-bit kernels of "Fine code phases" and "Cold snapshot fixes" run on it with n_bytes = ceil(n_samples / 8) and stride / 16: the
 * result is byte for byte gpsacq_iq8_to_bits_device followed by gpsacq_refine_device / gpsacq_fine_doppler_device.
 *
 * gpsacq_refine_iq8, gpsacq_fine_doppler_iq8: host pointers, return after completion.  The _device forms: iq, tasks, peaks and the
 * records are device pointers, `in` and the params stay host pointers (params NULL: the defaults); work on the engine's stream, sync
 * != 0 waits; host and device form agree byte for byte.  gpsacq_coarse_fix_fine_iq8_device is gpsacq_coarse_fix_fine_device and
 * gpsacq_cold_fix_iq8_device is gpsacq_cold_fix_device with (in, d_iq, n_samples) for (d_bits, n_bytes): the same kernels downstream
 * of the two that read the capture, one stream, no host copy in between, the same optional scratch buffers; in sign mode the capture
 * is converted once for both kernels.  Argument errors are those of the 1-bit forms plus in == NULL, a format or multibit value that
 * gpsacq_search_iq8 refuses, a mean beyond +-128 where it is removed, a stride outside the bounds above and a misaligned device
 * pointer: GPSACQ_ERR_ARG, nothing launched and nothing written.  Engines the 1-bit forms refuse are GPSACQ_ERR_UNSUPPORTED here too.
 * Kernels (csrc/snapshot_iq_kernels.hip).  k_refine_iq and k_fine_dop_iq: one workgroup of four wave64 per task; wave w takes
 * segments w, w + 4, ..., lane l the 16-byte groups (8 samples) l, l + 64, ... of a segment; bytes XORed with 0x80 for
 * GPSACQ_IQ_U8, weight dwords of +1 / -1 / 0 bytes and 4 x int8 dot products, 24 per group (8 for the prompt alone), the mean as a
 * correction applied only when it is not zero; the 24 chips of a group are bits of one 32-chip window cut out of the chip sequence in
 * LDS; int32 sums per lane, xor shuffles over the wave, 64-bit integer squares; no atomics and no float before the estimate, so
 * the record does not depend on the order of anything.  Every loop is bounded by kernel arguments.
 *
 * gpsacq_snap_quality* stays for 1-bit records (sign mode's included): its analytic floor is that of a +-1 stream.  The multi-bit
 * records' floor is measured on the capture: "Snapshot signal quality on an 8-bit IQ capture" below, gpsacq_snap_quality_iq8.
 *
 * OUT OF SCOPE.  (The aided searches on the IQ bytes are "Aided acquisition on an 8-bit IQ capture" and "Coherent aided acquisition
 * on an 8-bit IQ capture" below.)  Accumulated or re-aligned searches, multi-GPU, gps_test and gps_track.
 */
GPSACQ_API int gpsacq_refine_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride, const gpsacq_task* tasks,
                                 const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_refine_params* params, gpsacq_fine* fine_out);
GPSACQ_API int gpsacq_refine_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                        const void* d_tasks, const void* d_peaks, size_t n_tasks, const gpsacq_refine_params* params, void* d_fine,
                                        int sync);
GPSACQ_API int gpsacq_fine_doppler_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_peak* peaks, size_t n_tasks, const gpsacq_dopfine_params* params,
                                       gpsacq_dopfine* dopfine_out);
GPSACQ_API int gpsacq_fine_doppler_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_peaks, size_t n_tasks, const gpsacq_dopfine_params* params,
                                              void* d_dopfine, int sync);
GPSACQ_API int gpsacq_coarse_fix_fine_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                                 size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                 const gpsacq_refine_params* refine_params, const void* d_prior, const gpsacq_coarse_params* params,
                                                 void* d_fine, void* d_obs, void* d_fix, void* d_info, void* d_obs_out, int sync);
GPSACQ_API int gpsacq_cold_fix_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                          size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, const void* d_rx_ms, size_t n_fix,
                                          int n_chans, const gpsacq_dopfine_params* dopfine_params, const gpsacq_doppler_fix_params* doppler_params,
                                          const gpsacq_refine_params* refine_params, const gpsacq_coarse_params* coarse_params, void* d_dopfine,
                                          void* d_rate_obs, void* d_doppler_fix, void* d_prior, void* d_fine, void* d_obs, void* d_fix, void* d_info,
                                          void* d_obs_out, int sync);
/* device time of the last call of this section on this engine, milliseconds (HIP events on its stream; waits for them): the 8-bit ->
 * 1-bit conversion (sign mode), the kernel that wrote the fine records (k_refine_iq, in sign mode k_refine) and the one that wrote
 * the fine Dopplers (k_fine_dop_iq, in sign mode k_fine_dop).  A kernel that the last call did not run reads 0.  Any pointer may be
 * NULL. */
GPSACQ_API int gpsacq_snapshot_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* refine_ms, float* fine_dop_ms);

/*
 * ---- Aided acquisition: predicted code phase and Doppler, windowed search -------------------------------------------------------
 *
 * The snapshot chain above uses the satellites the FFT search finds in ONE 7.3 ms block at its threshold of 25.  A satellite 8 to
 * 10 dB below that never enters a fix, though the capture holds it over its 117 ms -- and after the first fix the receiver knows
 * where to look to within a sample and a Doppler grid point.  gpsacq_aid_predict turns a fix (and a velocity, where there is one)
 * into a predicted code phase and Doppler per satellite; gpsacq_aided_search goes back to the 1-bit capture as gpsacq_refine does
 * and sums the 1 ms prompt powers of a window of blocks over the few hypotheses around the prediction; its peaks drop into
 * gpsacq_refine, gpsacq_fine_doppler, gpsacq_coarse_obs[_fine], gpsacq_coarse_fix_fine_device and gpsacq_track_start unchanged.
 * (Estimated from the generator's figure, amplitude 0.151 = 45 dB-Hz, not measured: amplitude 0.03 is about 32 dB-Hz, a search snr
 * of about 12; the sum of 117 prompt powers at the right hypothesis then stands about 8 sigma over its floor.)  THE MODEL; the
 * kernels (csrc/aided_kernels.hip) and the reference of the tests (tests/aided_ref.py) are both written from this text.  Integer
 * arithmetic "mod 2^N" is unsigned wrap-around as in THE CHANNEL MODEL; every fp64 expression is evaluated as written, every
 * operation rounded by itself (no fused multiply-add).
 *
 * A. PREDICTION.  gpsacq_aid_predict.  INPUTS.  eph[n_eph] as for gpsacq_fix_batch.  fix[n_fix] of gpsacq_fix: its place and its
 * (rx_ms, rx_frac) are taken as the RECEIVE INSTANT of the first sample of the row's block (FROM PEAKS of "Coarse-time fixes"
 * makes that sample the receive instant of a row).  vel[n_fix] of gpsacq_vel, optional: NULL, or a status other than
 * GPSACQ_VEL_OK, means v_r = 0 and drift_r = 0.  n_chans in 1 .. GPSACQ_FIX_MAX_SATS: channel c is eph[c], as in FROM PEAKS, and
 * the records are aid[n_fix][n_chans], block outer and channel inner.  gpsacq_aid_params: elev_min_deg, finite and in [-90, 90];
 * gpsacq_aid_default_params (host only) sets 5.0.
 * PER (fix, channel).  Times are seconds from the receive instant; the time t is the pair (rx_ms + k folded into the week, frac)
 * with (k, frac) FIX's split of rx_frac + t (k = floor(1e3 u), frac = u - 1e-3 k, moved by one millisecond where rounding left
 * frac outside [0, 1e-3)).  Omega_e, c, L1 and R(a) as in "Coarse-time fixes" and VELOCITY.
 *   LIGHT TIME: the two passes of "Coarse-time fixes" A from the fix's place r_r.
 *       pass 1: the satellite position at the uncorrected time -75e-3, turned by R(-Omega_e 75e-3); tau = its distance to r_r / c.
 *       pass 2: position and clock correction cc at the uncorrected time -tau, turned by R(-Omega_e tau); tau' = distance / c.
 *   CODE.  T = cc - tau' is the uncorrected satellite time the replica shows at the receive instant; (tx_ms, tx_frac) is the pair
 *     of T, and
 *       ca_center = (int)nearbyint(tx_frac * fs) mod spm,      spm = gpsacq_info.num_lags
 *     -- FROM PEAKS read backwards (tx_frac = ca_shift / fs).
 *   DOPPLER: VELOCITY's row read backwards.  Position p, clock correction cc3, velocity v and clock_drift of the satellite at the
 *     uncorrected time (tx_ms, tx_frac) (SATELLITE STATE, SATELLITE VELOCITY); then, exactly as VELOCITY has them,
 *       theta = Omega_e ((double)fold(tx_ms - rx_ms) 1e-3 + ((tx_frac - cc3) - rx_frac))
 *       r_i = R(theta) p,     v_i = R(theta) (v + Omega_e x p),     e_i = (r_i - r_r) / |r_i - r_r|
 *       rho' = e_i . (v_i - (v_r + Omega_e x r_r)) + c drift_r - c clock_drift
 *       doppler_hz = -(L1 / c) rho'
 *       lo_center  = (int)nearbyint(doppler_hz / gpsacq_info.doppler_step_hz)
 *   ELEVATION by k_sat_view's rule: (lat, lon) = FIX's LatLonAlt() of r_r, d = r_i - r_r in VIEW's local frame,
 *     elev_deg = atan2(u, hypot(e, n)) * 180 / pi.
 *   (nearbyint: to nearest, ties to even.)
 * RECORD gpsacq_aid.  flags: GPSACQ_AID_NO_FIX, the fix is not GPSACQ_FIX_OK; GPSACQ_AID_NO_EPH, c >= n_eph, or the ephemeris does
 * not pass SATELLITE STATE's rule, or r_i, tx_frac, doppler_hz or elev_deg is not finite; for these two everything else in the
 * record is 0.  GPSACQ_AID_LOW: elev_deg < elev_min_deg.  GPSACQ_AID_OFF_GRID: |lo_center| > (gpsacq_info.num_doppler_total - 1)
 * / 2, beyond the engine's grid (a Doppler beyond +-2^31 steps counts so too, with lo_center 0).  A record with any flag is NOT
 * USABLE; LOW and OFF_GRID keep the rest of the record.
 * NOT MODELLED.  The atmosphere: ionosphere and troposphere delay the code by 2 to 30 m, at most about half a sample at 5.456 MHz
 * (55 m per sample), well inside any window.  The Doppler's own rate over the window (below 1 Hz/s).  The fix's own error enters
 * as it is: 150 m of place or 0.5 us of receive time is one chip.
 * THE RECEIVE INSTANT OF A COARSE-TIME FIX.  gpsacq_coarse_fix_batch reports t0 + s - b / c, and its s is good to cdop times the
 * range noise only -- milliseconds -- which lands in rx_frac and moves EVERY prediction by the same code offset.  The fix's place
 * and b are good: take the receive instant as t0 + nearbyint(1e3 s) 1e-3 - bias_m / c from its gpsacq_coarse_info (any whole
 * millisecond serves: a few milliseconds of satellite motion are metres) and put that into rx_ms and rx_frac before predicting.
 * tools/snapshot_bench.py --aided does; with the fix's own time it found 8 of 2048 weak satellites, with this one 2022 of 2024.
 *
 * B. WINDOWED SEARCH.  gpsacq_aided_search.  INPUTS as gpsacq_refine's: bits[n_bytes], stride, tasks[n_tasks] (NULL: the reference
 * schedule, task t = (block t, PRN t % 32)).  aid[n_tasks]: a prediction per task (of which flags, ca_center and lo_center are
 * read).  peaks_in[n_tasks], optional: what the plain search returned for these tasks.  gpsacq_aided_params: blocks, 1 .. 64, the
 * length of the window; min_segments >= 1; code_half = W, 0 .. 127, and dop_half = K, 0 .. 8: the search covers 2W + 1 code
 * phases and 2K + 1 Doppler grid points around the prediction; keep_snr and ratio_min, finite.  gpsacq_aided_default_params (host
 * only) sets 16, 1, 16, 1, 25.0 (the threshold of the search) and ratio_min = 1.922 (DEFAULT RATIO_MIN below).
 * PER TASK.  spm, o, FULL, the window, its segments and the flags GPSACQ_AIDED_SHORT and GPSACQ_AIDED_FEW are exactly steps 2 and 3
 * of "Fine code phases" with this section's blocks and min_segments.
 * 1. KEPT.  peaks_in is given and peaks_in[t].snr >= keep_snr: the output peak is peaks_in[t] byte for byte, the record is the flag
 *    GPSACQ_AIDED_KEPT and zeros, and nothing is read from the capture.  This comes before everything below.
 * 2. NO_AID (the record is GPSACQ_AIDED_NO_AID and zeros, the output peak is 16 zero bytes): the aid record is not usable, or its
 *    ca_center is outside [0, spm); or the task is out of range by refine's rule (block < 0, prn outside 0 .. 31, o at or beyond
 *    sample 8 n_bytes); or no Doppler hypothesis of step 3 is valid.
 * 3. HYPOTHESES.  Doppler index d = 0 .. 2K with lo_shift_d = lo_center - K + d.  d is VALID when |lo_shift_d| lies on the
 *    engine's grid (at most (num_doppler_total - 1) / 2) and refine's NCO range test passes: fc + lo_dop and 1.023e6 + ca_dop in
 *    [0, fs) and ca_rate != 0, with lo_rate_d and ca_rate_d from step 1 of "Fine code phases".  Code index h = 0 .. 2W, with
 *      base = (ca_center - W) mod spm        in [0, spm)
 *      P0(h, d) = ((base + h) * ca_rate_d) mod FULL              base + h is NOT reduced mod spm
 *      ca_shift_h = (base + h) mod spm                           what is reported
 *    and at window sample j (the first is j = 0, sample o + j of the capture) the replica of (h, d) shows
 *      P = (P0(h, d) + j * ca_rate_d) mod FULL = ((base + h + j) * ca_rate_d) mod FULL,     chip[P >> 32]:
 *    the replica of h at sample j is the replica of h = 0 at sample j + h, exactly -- ONE chip stream per (segment, d).  The
 *    carrier is refine's, ph = j * lo_rate_d (mod 2^32), counted from the window's first sample and the same for every h.  The
 *    segments are the window's, fixed, whatever h is.
 * 4. SUMS.  I_P, Q_P: the prompt sums of THE CHANNEL MODEL over the spm samples of a segment, as step 4 of "Fine code phases" has
 *    them.  power(h, d) = sum over the segments of I_P^2 + Q_P^2, uint64 (a segment adds at most 2 spm^2; 64 blocks stay below
 *    2^39).  For base + h < spm this is bit for bit the `prompt` field gpsacq_refine returns for a peak (ca_shift_h, lo_shift_d).
 *    Across the wrap (base + h >= spm) refine starts from ((base + h - spm) * ca_rate) mod FULL: the two differ by
 *    (spm * ca_rate) mod FULL of code position, the code Doppler's creep over one millisecond: ca_dop * 1 ms, 3.2e-3 chip at 5 kHz
 *    (far below the sample grid, but enough to move a sample across a chip boundary: the sums differ in a few units).
 * 5. RECORD gpsacq_aided: flags, segments, n_code = 2W + 1, n_dop = 2K + 1, and
 *      best   = the largest power over the valid d and all h; its place (best_d, best_h) is the hypothesis with the largest KEY
 *               (power, -d, -h) in lexicographic order -- among equal powers the smaller d, then the smaller h -- so the result
 *               does not depend on the order of any reduction
 *      lo_shift = lo_center - K + best_d,     ca_shift = ca_shift_(best_h)
 *      total  = the sum of power(h, d) over the valid d and all h
 *      floor  = 2 * spm * segments           what a +-1 stream uncorrelated with the replica leaves: E[I^2 + Q^2] = 2 spm
 *      ratio  = (double)best / (double)floor,   0.0 where floor == 0
 *    GPSACQ_AIDED_NO_POWER: best == 0.  GPSACQ_AIDED_BELOW: ratio < ratio_min.  DETECTED: none of NO_AID, FEW, NO_POWER, BELOW.
 *    Every record but KEPT and NO_AID keeps all its fields whatever its flags.
 * 6. OUTPUT PEAK (gpsacq_peak).  Detected: { (float)ratio, lo_shift, ca_shift, (float)best }.  Otherwise 16 zero bytes.  AN AIDED
 *    PEAK'S snr IS ON THE RATIO SCALE (1 = the floor), not on the search's: give the calls downstream snr_min <= ratio_min, which
 *    passes every aided peak and, while ratio_min <= keep_snr, every KEPT peak too.
 * 7. powers_out[n_tasks][2K + 1][2W + 1], optional, uint64: power(h, d) at [t][d][h]; the rows of invalid d are 0, KEPT and NO_AID
 *    tasks are all 0.
 * LIMITS.  A segment is one millisecond of coherent sum, 1 kHz wide: neighbouring Doppler grid points (136 Hz at 5.456 MHz) differ
 * by a few per cent of power, so best_d picks among near equals and lo_shift is good to +-K grid points, no better;
 * gpsacq_fine_doppler takes it from there.  ca_shift is a whole sample, as a search peak's; gpsacq_refine takes it from there.
 * DEFAULT RATIO_MIN.  No closed form covers the floor: the C/A cross-correlation of the strong satellites is part of it.  Measured
 * (tools/aided_floor.py, on the CPU with tests/aided_ref.py): the scene of tools/snapshot_bench.py (eight satellites at amplitude
 * 0.2, noise sigma 1, fs = 5.456 MHz) made with tests/gen_ref.py and searched for its 24 ABSENT PRNs with the defaults, 2304 draws of
 * (window start, lo_center, PRN, ca_center), 99 hypotheses each: the largest ratio was 1.7376 (median 1.348, 99.9 % below 1.688).  The default is that
 * plus a quarter of its excess over 1: 1.7376 + 0.7376 / 4 = 1.922.  It belongs to 16 blocks, W = 16, K = 1: more hypotheses or fewer segments raise the
 * floor's maximum, and a caller who changes them measures again.
 * WHAT TO EXPECT.  Measured on the CPU (tests/test_aided.py, 16 blocks, five satellites at 0.2 beside the weak one): amplitude 0.03
 * reads ratio 1.63, 0.04 reads 1.98, 0.045 reads 2.20, 0.05 reads 2.45, where the plain search gives all of them an snr of 15 to 16,
 * a noise peak.  So the default detects from about amplitude 0.04 (some 33.5 dB-Hz on the generator's scale, estimated), not from the
 * 0.03 first hoped for.  Measured on an MI355X (tools/snapshot_bench.py --aided, 1024 blocks, two satellites at 0.05 and two absent
 * PRNs per block, shader clock not read): 2022 of 2024 weak tasks detected, all at the true code phase (17.3 m rms, whole samples),
 * median ratio 2.49; no detection in 2048 absent tasks, largest ratio 1.696.
 *
 * C. THE CHAIN.  gpsacq_aided_peaks_device: k_aid_predict then k_aided on the engine's stream, no host copy in between, from eph,
 * d_fix[n_fix], d_vel[n_fix] (may be NULL), the capture, d_tasks[n_fix * n_chans] (block outer, channel inner: task b * n_chans
 * + c = block b against the PRN of eph[c]; NULL is the reference schedule) and d_peaks_in (may be NULL) to d_aid (may be NULL:
 * engine scratch), d_aided and d_peaks_out, exactly what the two calls give.
 *
 * gpsacq_aid_predict, gpsacq_aided_search: host pointers, return after completion.  The _device forms: device pointers for
 * everything but eph and the params (NULL: the defaults), bits at any byte address; work on the engine's stream, sync != 0
 * waits; host and device form agree byte for byte.  peaks_out must not be peaks_in.  Argument errors -- a NULL pointer (vel,
 * peaks_in, powers_out and d_aid of the chain may be NULL), n_fix or n_tasks == 0, n_bytes == 0, a parameter or the stride outside
 * its bounds, n_chans outside 1..GPSACQ_FIX_MAX_SATS, n_eph <= 0 -- return GPSACQ_ERR_ARG, launch nothing and write nothing.
 * GPSACQ_ERR_UNSUPPORTED: the engines gpsacq_refine refuses (num_lags > 65535, fs below 1.138 MHz) and an engine in non-coherent
 * mode (gpsacq_set_noncoherent with more than one block); a finer Doppler grid (gpsacq_set_doppler_step) is supported, lo_center
 * and lo_shift then count its points.
 * Kernels (csrc/aided_kernels.hip).  k_aid_predict: one lane per (fix, channel), the orbit from csrc/orbit_device.hpp, the frame
 * from csrc/nav_device.hpp.  k_aided: one workgroup of four wave64 per task; a wave owns whole segments.  Per (segment, d) its
 * lanes build, once per 32-sample word and with k_refine's word loop (csrc/capture_words.hpp), the samples xor-ed with the two
 * carrier masks and the ONE chip-mask stream of spm + 2W samples into LDS; then lane h (h + 64, ... in further passes over the
 * same masks) walks the segment's words, cuts its own chip mask out of two neighbouring stream words with a funnel shift by
 * h & 31 at word offset h >> 5, takes two xor-popcounts per word, squares its own I and Q and adds into its own uint64.  No
 * cross-lane reduction inside a segment, no atomics; the four waves' sums meet in LDS once per d, and the best hypothesis is the
 * maximum of a packed key.  Every loop is bounded by kernel arguments, every LDS index by the host-checked limits
 * (spm <= 65535, W <= 127, K <= 8).
 *
 * OUT OF SCOPE.  Accumulated or re-aligned searches, fs above 10 MHz, multi-GPU, gps_test and gps_track.  (8-bit IQ input:
 * "Aided acquisition on an 8-bit IQ capture" below.)  The correlator, the search and every existing record stay as they are.
 */
#define GPSACQ_AID_NO_FIX 1      /* the fix is not GPSACQ_FIX_OK: the record is this flag and zeros */
#define GPSACQ_AID_NO_EPH 2      /* no valid ephemeris, or a state that is not finite: the record is this flag and zeros */
#define GPSACQ_AID_LOW 4         /* elev_deg < elev_min_deg */
#define GPSACQ_AID_OFF_GRID 8    /* |lo_center| beyond the engine's Doppler grid */
typedef struct { double elev_min_deg; double reserved; } gpsacq_aid_params;                                                       /* 16 bytes */
typedef struct { int32_t flags, ca_center, lo_center, reserved; double tx_frac, doppler_hz, elev_deg; } gpsacq_aid;                /* 40 bytes */
#define GPSACQ_AIDED_KEPT 1      /* peaks_in[t].snr >= keep_snr: the output peak is the input peak, the record this flag and zeros */
#define GPSACQ_AIDED_NO_AID 2    /* no usable prediction, a task out of range or no valid Doppler hypothesis: this flag and zeros */
#define GPSACQ_AIDED_SHORT 4     /* the capture ends before the window does */
#define GPSACQ_AIDED_FEW 8       /* segments < min_segments */
#define GPSACQ_AIDED_NO_POWER 16 /* best == 0 */
#define GPSACQ_AIDED_BELOW 32    /* ratio < ratio_min */
typedef struct { int32_t blocks, min_segments, code_half, dop_half; double keep_snr, ratio_min; } gpsacq_aided_params;             /* 32 bytes */
typedef struct { int32_t flags, segments, n_code, n_dop, best_h, best_d, lo_shift, ca_shift; uint64_t best, total, floor;
                 double ratio; } gpsacq_aided;                                                                                   /* 64 bytes */
GPSACQ_API int gpsacq_aid_default_params(gpsacq_aid_params* p);       /* host only */
GPSACQ_API int gpsacq_aided_default_params(gpsacq_aided_params* p);   /* host only */
GPSACQ_API int gpsacq_aid_predict(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_fix* fix /* [n_fix] */,
                                  const gpsacq_vel* vel /* [n_fix] or NULL */, size_t n_fix, int n_chans, const gpsacq_aid_params* params,
                                  gpsacq_aid* aid_out /* [n_fix][n_chans] */);
GPSACQ_API int gpsacq_aid_predict_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel, size_t n_fix,
                                         int n_chans, const gpsacq_aid_params* params, void* d_aid, int sync);
GPSACQ_API int gpsacq_aided_search(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks, const gpsacq_aid* aid,
                                   const gpsacq_peak* peaks_in /* or NULL */, size_t n_tasks, const gpsacq_aided_params* params,
                                   gpsacq_aided* aided_out, gpsacq_peak* peaks_out, uint64_t* powers_out /* [n_tasks][2K + 1][2W + 1] or NULL */);
GPSACQ_API int gpsacq_aided_search_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_aid,
                                          const void* d_peaks_in, size_t n_tasks, const gpsacq_aided_params* params, void* d_aided,
                                          void* d_peaks_out, void* d_powers_out, int sync);
GPSACQ_API int gpsacq_aided_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel,
                                         const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks, const void* d_peaks_in, size_t n_fix,
                                         int n_chans, const gpsacq_aid_params* aid_params, const gpsacq_aided_params* aided_params, void* d_aid,
                                         void* d_aided, void* d_peaks_out, int sync);
/* device time of k_aid_predict and k_aided as last run on this engine, milliseconds (HIP events on its stream; waits for them); a
 * kernel that has not run reads 0.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_aided_last_ms(const gpsacq_engine* e, float* predict_ms, float* search_ms);

/*
 * ---- Coherent aided acquisition: 20 ms sums, bit edge and fine Doppler ------------------------------------------------------------
 *
 * gpsacq_aided_search squares every 1 ms prompt sum on the spot and throws its sign and phase away; its default detects from about
 * amplitude 0.04.  gpsacq_aided_coh_search keeps the signed sums (I, Q) of a window's segments, turns them back by a Doppler finer
 * than the grid, and adds them coherently over a data bit's M = 20 ms with a hypothesis for the bit edge -- the classic
 * high-sensitivity step.  Its peaks drop into the same calls downstream.  THE MODEL; the kernel (k_aided_coh of
 * csrc/aided_kernels.hip) and the reference of the tests (tests/aided_coh_ref.py) are both written from this text, with the
 * conventions of the section above (integers mod 2^N, every fp64 operation rounded by itself).
 *
 * A. SEARCH.  gpsacq_aided_coh_search.  INPUTS are gpsacq_aided_search's: bits[n_bytes], stride, tasks[n_tasks] (NULL: the
 * reference schedule), aid[n_tasks], peaks_in[n_tasks] (optional).  gpsacq_aided_coh_params:
 *     blocks        1 .. 64          the window
 *     min_segments  >= 1
 *     code_half     W, 0 .. 31       2 W + 1 code phases, one pass of 64 lanes
 *     dop_half      K, 0 .. 8        2 K + 1 Doppler grid points
 *     coh_ms        M, one of 1, 2, 4, 5, 10, 20: the segments of a coherent sum (the divisors of a data bit worth having)
 *     fine_half     F, 0 .. 7        2 F + 1 fine Doppler hypotheses per grid point
 *     fine_step     u, 1 .. 512      their spacing in 1/1024 cycle per segment: u (fs / spm) / 1024 Hz
 *     reserved      not read
 *     keep_snr, ratio_min            finite
 * gpsacq_aided_coh_default_params (host only) sets 16, 20, 16, 1, 20, 3, 25 (24.4 Hz at 5.456 MHz), 0, 25.0 and ratio_min =
 * 10.73 (DEFAULT RATIO_MIN below).
 * PER TASK.
 * 1. KEPT, 2. NO_AID, 3. HYPOTHESES (d, h): steps 1 to 3 of B. WINDOWED SEARCH above, word for word, with this section's blocks,
 *    min_segments, W and K: base, P0(h, d), one chip stream per (segment, d), the carrier counted from the window's first sample,
 *    the window's fixed segments s = 0 .. S - 1 (S = `segments`), the flags SHORT and FEW.
 * 4. SEGMENT SUMS.  z_s = (I_s, Q_s) of hypothesis (h, d): THE CHANNEL MODEL's prompt sums over the spm samples of segment s --
 *    what step 4 above squares.  |I_s|, |Q_s| <= spm.
 * 5. COHERENT SUMS.  The ROTATION TABLE is data of the model: C[k] = nearbyint(2^14 cos(2 pi k / 1024)) and S[k] =
 *    nearbyint(2^14 sin(2 pi k / 1024)), int16, k = 0 .. 1023, built by the host in fp64; gpsacq_aided_coh_table writes C then S.
 *    (No entry lies within 3.9e-4 of a rounding tie: any sane cos gives the same table.)  For the fine index g = 0 .. 2F let
 *    f = g - F and k_s = (f u s) mod 1024, a true modulo (0 .. 1023 also for negative f).  In int64
 *        A_s = I_s C[k_s] + Q_s S[k_s]
 *        B_s = Q_s C[k_s] - I_s S[k_s]
 *    -- z_s turned BACK by f u s / 1024 cycles: a positive f is the hypothesis of a Doppler ABOVE lo_shift_d's, by
 *    f u (fs / spm) / 1024 Hz.  For the edge e = 0 .. M - 1 the period boundaries are {0, S} and every s with 0 < s < S and
 *    s = e (mod M).  Two consecutive boundaries a < b make one period; the partial periods at both ends count (an e at or beyond S
 *    leaves the one period [0, S)).  Per period
 *        A' = floor((sum of A_s over a <= s < b) / 2^14),     B' likewise
 *    -- an arithmetic shift AFTER the sum, not before -- and
 *        power(h, d, g, e) = sum over the periods of A'^2 + B'^2,  uint64.
 *    BOUNDS.  |A_s|, |B_s| <= sqrt(2) spm (2^14 + 1) < 2^31 for spm <= 65535; a period of at most 20 segments stays below 2^36,
 *    A' below 2^22; a period of n segments adds at most about 2 n^2 spm^2, so power <= M S 2 spm^2 (1 + 2^-13) <= 20 * 2 * 65535 *
 *    (64 * 40000) (1 + 2^-13) < 2^43: the key of step 6 gives it 44 bits.  (The library still refuses, GPSACQ_ERR_UNSUPPORTED, an
 *    engine and parameters with M * 2 * spm * (blocks * 40000) >= 2^43; the limits above leave none.)
 *    With M = 1 and F = 0 every period is one segment and C[0] = 2^14, S[0] = 0: power(h, d, 0, 0) is gpsacq_aided_search's
 *    power(h, d) bit for bit.
 * 6. RECORD gpsacq_aided_coh: flags, segments, n_code = 2W + 1, n_dop = 2K + 1, n_fine = 2F + 1, n_edge = M, and
 *      best    = the largest power over the valid d and all g, e, h; its place (best_d, best_f = g, best_e, best_h) is the
 *                hypothesis with the largest KEY (power, -d, -g, -e, -h) in lexicographic order -- among equal powers the smallest
 *                d, then g, then e, then h -- whatever the order of any reduction
 *      lo_shift = lo_center - K + best_d,     ca_shift = (base + best_h) mod spm
 *      noncoh  = the sum over the segments of I_s^2 + Q_s^2 at (best_h, best_d): gpsacq_aided_search's power there
 *      floor   = 2 * spm * segments      the scale of the section above: for a +-1 stream uncorrelated with the replica a period of
 *                n segments leaves n * 2 spm, whatever the partition
 *      ratio   = (double)best / (double)floor,   0.0 where floor == 0
 *      doppler_hz = lo_dop + ((double)((best_f - F) * u) / 1024.0) * (fs / (double)spm), the operations in that order, lo_dop being
 *                step 1's of "Fine code phases" for lo_shift (lo_shift * doppler_step_hz on a finer grid, else lo_shift * fs / 40000)
 *      best_e  = the segment index mod M at which a data bit starts: the bit phase of the window's first sample, which a
 *                coarse-time fix knows to about +-3 ms only
 *      reserved = 0.0
 *    The flags are GPSACQ_AIDED_* with the meanings of the section above (NO_POWER: best == 0; BELOW: ratio < ratio_min); KEPT and
 *    NO_AID records are the flag and zeros.  OUTPUT PEAK as step 6 above: detected, { (float)ratio, lo_shift, ca_shift,
 *    (float)best }, its snr on THIS section's ratio scale; otherwise 16 zero bytes (KEPT: the input peak).
 * 7. powers_out[n_tasks][2K + 1][2F + 1][M][2W + 1], optional, uint64: power(h, d, g, e) at [t][d][g][e][h]; rows of invalid d
 *    are 0, KEPT and NO_AID tasks are all 0.
 * LIMITS.  The segments are the window's, not the code periods of hypothesis h: the true bit edge falls INSIDE one segment per
 * bit, and that segment partly cancels -- at worst one of twenty, about 0.2 dB on average.  (Aligning the segments per hypothesis
 * would give up the one shared chip stream.)  The Doppler's rate over the window and 8-bit IQ input stay out of scope as above.
 * A coherent sum of M ms is 1 / M kHz wide: u and F must cover half a grid step in steps well below 1000 / (2 M) Hz.
 * DEFAULT RATIO_MIN.  Measured as the section above did (tools/aided_floor.py --coherent, on the CPU with tests/aided_coh_ref.py):
 * the scene of tools/snapshot_bench.py with random navigation bits on its eight satellites, searched for its 24 absent PRNs with
 * the defaults, 2304 draws of 3 * 7 * 20 * 33 = 13 860 hypotheses each: the largest ratio was 8.7837 (median 3.9374, 99.9 % below
 * 7.8919).  The default is that plus a quarter of its excess over 1: 8.7837 + 7.7837 / 4 = 10.73.  The floor's maximum over so
 * many hypotheses and only six or seven bit periods is far above the non-coherent 1.74, and its tail is not noise: white noise alone
 * would put the maximum of 13 860 sums of seven periods near 3 (estimated); the median of 3.9 and the draws above 6 are the C/A
 * cross-correlation of the eight satellites at amplitude 0.2, 16 dB above the signal sought, which a 20 ms sum adds up coherently
 * wherever a Doppler difference is close to a multiple of 1 kHz.  The signal still clears this default from a lower amplitude than
 * the non-coherent one does, but by less than the noise alone would promise.  It belongs to the defaults and to that scene; a
 * caller who changes either measures again (the scene of tests/test_aided_coh.py, five strong satellites, read at most 3.5).
 * WHAT TO EXPECT.  Measured on the CPU (tests/test_aided_coh.py and its scene: 16 blocks, five satellites at 0.2 with navigation
 * bits beside the weak one, the two absent PRNs read 3.23 and 3.49): amplitude 0.03 reads ratio 11.17 (detected, just above the
 * default; gpsacq_aided_search reads 1.79 there, BELOW), 0.0337 reads 13.67 where the non-coherent search reads 1.911, still BELOW,
 * 0.034 reads 13.84 against 1.922 and 0.035 reads 14.63 against 1.959.  So the default detects from about amplitude 0.03, where
 * the section above needs 0.04: some 2.5 dB, not the 8 dB the ratios alone suggest, because the threshold rose with them.
 * Measured on an MI355X (tools/snapshot_bench.py --aided-coh, 1024 blocks, two satellites at amplitude 0.03 and two absent PRNs per
 * block, navigation bits on, shader clock not read): 875 of 2048 weak tasks detected (870 at the true code phase, 5 elsewhere),
 * median ratio 10.36 -- just under the default: 0.03 is where it begins to detect -- where gpsacq_aided_search detects 50; no detection
 * in 2048 absent tasks, largest ratio 6.08; doppler_hz 6.0 Hz rms from the generator's, best_e equal to its edge in 62 %, within one
 * segment in 87 %; k_aided_coh 6.64 ms beside k_aided 6.15 ms on the same 4096 tasks.  DESIGN.md 8.5 has the rest.  The dB-Hz scale
 * is the generator's, estimated, as above.
 *
 * B. THE RECEIVE INSTANT ON THE DEVICE.  gpsacq_aid_instant: "THE RECEIVE INSTANT OF A COARSE-TIME FIX" above as a kernel, one
 * lane per fix.  fix[n_fix] (gpsacq_fix), coarse_info[n_fix] and prior[n_fix] as gpsacq_coarse_fix_batch took and gave them;
 * fix_out[n_fix] is a copy of the fix with (rx_ms, rx_frac) replaced, c = 2.99792458e8, every operation rounded by itself,
 * nearbyint to nearest, ties to even:
 *     t       = nearbyint(1e3 * coarse_s) * 1e-3 - bias_m / c
 *     k       = floor(1e3 * t)
 *     rx_ms   = (prior.rx_ms + k) folded into the week (0 .. 604 799 999)
 *     rx_frac = t - 1e-3 * k
 * A fix that is not GPSACQ_FIX_OK is copied byte for byte.  A GPSACQ_FIX_OK fix whose coarse_s or bias_m is not finite, or whose
 * k is outside -2^31 .. 2^31 - 1, is copied with status GPSACQ_FIX_NO_CONVERGE, so that gpsacq_aid_predict refuses it.  fix_out
 * may be fix.
 *
 * C. THE CHAIN.  gpsacq_aided_coh_peaks_device: k_aid_instant, then k_aid_predict (unchanged), then k_aided_coh on the engine's
 * stream, no host copy in between: gpsacq_aided_peaks_device's arguments plus d_info and d_prior.  d_info == NULL skips the
 * instant step (the fixes are taken as they are; d_prior is then not read).  d_fix_instant (the fixes predicted from) and d_aid
 * may be NULL: engine scratch.  The results are exactly what the three calls give.
 *
 * The host forms take host pointers and return after completion; the _device forms take device pointers for everything but eph
 * and the params (NULL: the defaults), bits at any byte address, work on the engine's stream, sync != 0 waits; host and device
 * form agree byte for byte.  Argument errors as in the section above (and coh_ms outside its set, F, u, W, K outside their
 * ranges): GPSACQ_ERR_ARG, nothing launched, nothing written.  GPSACQ_ERR_UNSUPPORTED: everything gpsacq_aided_search refuses,
 * and fit * (2W + 1) > 5120 with fit = blocks * 40000 / spm, the z matrix of the kernel (the defaults need 117 * 33 = 3861).
 * Kernels (csrc/aided_kernels.hip).  k_aided_coh<M>: one workgroup of four wave64 per task.  Per d: the CORRELATION STAGE is
 * k_aided's segment walk at one pass (wave w takes segments w, w + 4, ...; lane h stores its (I, Q) as an int32 pair into z[s][h]
 * in LDS, 40 KB); after a barrier the COHERENT STAGE takes (h, g) as its work item on the z column of h: one walk over the
 * segments turns z_s by the table (in LDS, 4 KB), keeps the prefix sums of the turned series and, for e = s mod M alone, closes
 * that edge's period as the difference to the prefix kept at its last boundary -- every e in O(S), M accumulators, the walk
 * unrolled by M so that no register array is indexed at run time.  The best hypothesis is the maximum of a packed key, reduced
 * once per d.  No atomics, no scratch; every loop is bounded by kernel arguments, every LDS index by the host-checked limits.
 * k_aid_instant: one lane per fix.
 */
typedef struct { int32_t blocks, min_segments, code_half, dop_half, coh_ms, fine_half, fine_step, reserved;
                 double keep_snr, ratio_min; } gpsacq_aided_coh_params;                                                         /* 48 bytes */
typedef struct { int32_t flags, segments, n_code, n_dop, n_fine, n_edge, best_h, best_d, best_f, best_e, lo_shift, ca_shift;
                 uint64_t best, noncoh, floor; double ratio, doppler_hz, reserved; } gpsacq_aided_coh;                          /* 96 bytes */
GPSACQ_API int gpsacq_aided_coh_default_params(gpsacq_aided_coh_params* p);   /* host only */
GPSACQ_API int gpsacq_aided_coh_table(int16_t* out /* [2048]: C[0 .. 1023], then S[0 .. 1023] */);   /* host only */
GPSACQ_API int gpsacq_aided_coh_search(gpsacq_engine* e, const uint8_t* bits, size_t n_bytes, size_t stride, const gpsacq_task* tasks,
                                       const gpsacq_aid* aid, const gpsacq_peak* peaks_in /* or NULL */, size_t n_tasks,
                                       const gpsacq_aided_coh_params* params, gpsacq_aided_coh* aided_out, gpsacq_peak* peaks_out,
                                       uint64_t* powers_out /* [n_tasks][2 K + 1][2 F + 1][M][2 W + 1] or NULL */);
GPSACQ_API int gpsacq_aided_coh_search_device(gpsacq_engine* e, const void* d_bits, size_t n_bytes, size_t stride, const void* d_tasks,
                                              const void* d_aid, const void* d_peaks_in, size_t n_tasks, const gpsacq_aided_coh_params* params,
                                              void* d_aided, void* d_peaks_out, void* d_powers_out, int sync);
GPSACQ_API int gpsacq_aid_instant(gpsacq_engine* e, const gpsacq_fix* fix, const gpsacq_coarse_info* coarse_info, const gpsacq_coarse_prior* prior,
                                  size_t n_fix, gpsacq_fix* fix_out);
GPSACQ_API int gpsacq_aid_instant_device(gpsacq_engine* e, const void* d_fix, const void* d_info, const void* d_prior, size_t n_fix, void* d_fix_out,
                                         int sync);
GPSACQ_API int gpsacq_aided_coh_peaks_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_info /* or NULL */,
                                             const void* d_prior, const void* d_vel, const void* d_bits, size_t n_bytes, size_t stride,
                                             const void* d_tasks, const void* d_peaks_in, size_t n_fix, int n_chans, const gpsacq_aid_params* aid_params,
                                             const gpsacq_aided_coh_params* coh_params, void* d_fix_instant, void* d_aid, void* d_aided,
                                             void* d_peaks_out, int sync);
/* device time of k_aid_instant, k_aid_predict and k_aided_coh in the last call of this section on this engine, milliseconds (HIP
 * events on its stream; waits for them); a kernel that call did not run reads 0.  Any pointer may be NULL.  The chain's prediction
 * is timed here alone: gpsacq_aided_last_ms keeps the times of the section above's own calls. */
GPSACQ_API int gpsacq_aided_coh_last_ms(const gpsacq_engine* e, float* instant_ms, float* predict_ms, float* search_ms);

/*
 * ---- Aided acquisition on an 8-bit IQ capture: multi-bit windowed search ----------------------------------------------------------
 *
 * gpsacq_search_iq8 finds the strong satellites of an rtl-sdr / HackRF file, gpsacq_coarse_fix_fine_iq8_device fixes from them and
 * gpsacq_aid_predict says where the others must be -- but gpsacq_aided_search, the one step whose purpose is to find satellites
 * BELOW the search threshold, read a 1-bit real-IF stream: gpsacq_iq8_to_bits first, which drops one arm (3 dB) and puts the other
 * through a limiter (about 2 dB, more beside strong satellites), exactly where every dB decides.  gpsacq_aided_search_iq8 goes back
 * to the IQ bytes themselves.  The record is gpsacq_aided as it is, and its peaks drop into gpsacq_refine_iq8,
 * gpsacq_fine_doppler_iq8 and everything behind them unchanged.  THE MODEL; the kernel (csrc/aided_iq_kernels.hip) and the
 * reference of the tests (tests/aided_iq_ref.py) are both written from this text.  "Step n" is step n of "Aided acquisition" B,
 * WINDOWED SEARCH, which holds word for word except where this text changes it.
 *
 * INPUTS.  `in`, iq[2 * n_samples], n_samples and stride exactly as for gpsacq_refine_iq8: stride in BYTES, a multiple of 16,
 * 80000 <= stride <= 2^31; the device form takes a 16-byte-aligned device pointer.  tasks[n_tasks] (NULL: the reference schedule),
 * aid[n_tasks], peaks_in[n_tasks] (optional), gpsacq_aided_params and powers_out as for gpsacq_aided_search; peaks_in are the peaks of
 * gpsacq_search_iq8 with the same `in`.
 *
 * in->multibit != 0 (GPSACQ_SAMPLES_REAL and GPSACQ_SAMPLES_COMPLEX alike): THE MULTI-BIT PATH.
 *   SAMPLE.  v_i, v_q are the SAMPLE of "Snapshot chain on an 8-bit IQ capture": v = byte - off - dc, off = 128 for GPSACQ_IQ_U8 and 0
 *     for GPSACQ_IQ_S8, dc = nearbyint(mean) (ties to even) when remove_dc, else 0; |v| <= 256.  No floating-point mixer.
 *   WINDOW.  o = block * (stride / 2) against n_samples; segments, GPSACQ_AIDED_SHORT and GPSACQ_AIDED_FEW as that section's WINDOW
 *     has them, with this call's blocks and min_segments.  Nothing at or beyond byte 2 * n_samples is read.
 *   Step 1 (KEPT) is unchanged.  Step 2 (NO_AID) is unchanged, with "o at or beyond sample n_samples" as the range test.
 *   Step 3 (HYPOTHESES) is unchanged except for the carrier.  For Doppler index d, with lo_dop_d, ca_dop_d and ca_rate_d from step
 *     1 of "Fine code phases" for lo_shift_d:
 *         f_d = lo_dop_d - mix_hz + fc      (GPSACQ_SAMPLES_COMPLEX: f_d = lo_dop_d - mix_hz), left to right,
 *         lo_rate_d = (uint32)(int64)llround(f_d / fs * 2^32)             (round half away from zero; two's complement for f < 0)
 *     d is VALID when |lo_shift_d| lies on the engine's grid, |f_d| < fs / 2, 1.023e6 + ca_dop_d lies in [0, fs) and ca_rate_d != 0.
 *     base, P0(h, d), ca_shift_h, the ONE chip stream per (segment, d) and the carrier phase j * lo_rate_d (mod 2^32) counted from
 *     the window's first sample stay word for word.
 *   Step 4 (SUMS).  With C = 1 - 2 (cos bit), S = 1 - 2 (sin bit) and h_P = 1 - 2 chip as in that section's SUMS, per segment
 *         I_P = sum h_P (v_i C - v_q S),   Q_P = sum h_P (v_i S + v_q C)
 *     and power(h, d) = sum over the segments of I_P^2 + Q_P^2, uint64.  |I_P|, |Q_P| <= 512 spm < 2^25, a segment adds less than
 *     2^51 and there are fewer than 2^12 segments: nothing overflows.  For base + h < spm, power(h, d) is bit for bit the `prompt`
 *     field gpsacq_refine_iq8 returns for a peak (ca_shift_h, lo_shift_d) with the same `in` and blocks (a test uses it); across
 *     the wrap the two differ by the code Doppler's creep over one millisecond, as step 4 says of gpsacq_refine.
 *   Step 5 (RECORD), THE MEASURED FLOOR.  A +-1 replica uncorrelated with the samples leaves
 *         E[I_P^2 + Q_P^2] = 2 * sum (v_i^2 + v_q^2)     over the segment's samples
 *     -- exactly: C^2 = S^2 = 1, and the cross terms v_i v_q C S cancel between I and Q.  So
 *         floor = 2 * (sum over the samples of the window's segments of v_i^2 + v_q^2),
 *     an exact integer below 2^46 (2 * 2^17 per sample, fewer than 2^12 segments of at most 65535 samples).  For a +-1 real stream it
 *     is the 2 * spm * segments of gpsacq_aided_search: ratio stays on the same scale, 1 = the floor.  best <= spm * floor (Cauchy-
 *     Schwarz), below 2^62.  total is the sum mod 2^64; only a capture on the rails, correlated with every replica alike, could
 *     bring it near 2^64 (255 hypotheses * 9 grid points * 2^62 would need every one of them at the bound).
 *     ratio = (double)best / (double)floor, 0.0 where floor == 0.  The flags, the key (power, -d, -h), the output peak (step 6) and
 *     powers_out (step 7) are unchanged.
 *
 * in->multibit == GPSACQ_SAMPLES_SIGN: the capture is converted once per call into engine scratch by the path gpsacq_refine_iq8
 * uses, and k_aided runs on it with n_bytes = ceil(n_samples / 8) and stride / 16: the result is byte for byte
 * gpsacq_iq8_to_bits_device followed by gpsacq_aided_search_device.
 *
 * DEFAULT RATIO_MIN.  gpsacq_aided_default_params_iq8 (host only) sets gpsacq_aided_default_params' values with ratio_min measured
 * for the multi-bit path; a NULL params of this section's calls means these in multi-bit mode and gpsacq_aided_default_params' in
 * sign mode.  Without the limiter the strong satellites'
 * cross-correlation sits differently against the floor, and 1.922 does not transfer.  Measured (tools/aided_floor.py --iq8, on
 * the CPU with tests/aided_iq_ref.py): the scene of tools/snapshot_bench.py --iq8 (eight satellites at amplitude 0.2, noise sigma 1,
 * fs = 5.456 MHz, IF 0.4 MHz, scale 16, int8, the mean not removed) made with tests/gen_ref.py's 8-bit IQ generator and searched for
 * its 24 ABSENT PRNs with the defaults, 2304 draws of (window start, lo_center, PRN, ca_center), 99 hypotheses each: the largest
 * ratio was 2.9517 (median 1.7357, 99.9 % below 2.6363).  The default is that plus a quarter of its excess over 1: 2.9517 + 1.9517 / 4 =
 * 3.44.  That is far above the sign path's 1.7376, and it is not noise (the same capture without satellites read a median of 1.22 and at
 * most 1.35 over 48 draws): it is the C/A cross-correlation of the eight satellites at amplitude 0.2, which keeps both arms and passes
 * no limiter here exactly as the signal sought does -- some 5 dB more of either against the same floor.  It
 * belongs to 16 blocks, W = 16, K = 1 and to sign mode not at all: sign mode's callers take gpsacq_aided_default_params' 1.922.
 * WHAT TO EXPECT.  Measured on the CPU (tests/test_aided_iq.py: 16 blocks, five satellites at 0.2 with Dopplers spread evenly over
 * the range beside the weak one, the same capture searched both ways, three captures per amplitude): amplitude 0.03 reads ratio 2.67
 * to 3.07 where the sign path reads 1.58 to 1.70, 0.04 reads 3.83 to 4.40 against 1.96 to 2.03, 0.05 reads 5.45 to 6.09 against 2.44 to
 * 2.49.  At 0.04 the excess over 1 is 2.95, 3.09 and 3.42 times the sign path's: the median gain is 3.09, 4.9 dB -- the arm and the
 * limiter.  The two absent PRNs read 1.39 to 2.02 where the sign path reads 1.23 to 1.43, and the threshold rose with them: this
 * default detects from about amplitude 0.035, the sign path's 1.922 from about 0.039 (interpolated on ratio - 1 ~ amplitude^2).  So in
 * this scene most of the 4.9 dB go into a threshold that eight strong satellites set; a caller with fewer or weaker ones beside the
 * signal measures a lower one (tools/aided_floor.py --iq8) and keeps more of it.  Measured on an MI355X (tools/snapshot_bench.py --iq8
 * --aided, 1024 blocks, eight satellites at 0.2, two weak ones and two absent PRNs per block, both searches on the same tasks in the
 * same run, HIP events, shader clock not read): at amplitude 0.05 the multi-bit search detects 1815 of the 1815 weak tasks the
 * plain search had missed and the sign path 1811, median ratios 5.60 and 2.51; at 0.04 it detects 1986 of 2023 where the sign path
 * detects 1486, median ratios 4.05 and 2.02; every detection at the true code phase, none in 2047 absent tasks either way (largest
 * ratios 2.71 and 1.74).  k_aided_iq 40.98 ms for 3862 tasks of 99 hypotheses beside 6.54 ms for the conversion and k_aided (6.3
 * times), and beside the 150 ms that one k_refine_iq group walk per hypothesis would take (9.93 ms for 8426 hits of three replicas
 * in the same run).
 *
 * THE CHAIN.  gpsacq_aided_peaks_iq8_device is gpsacq_aided_peaks_device with (in, d_iq, n_samples) for (d_bits, n_bytes):
 * k_aid_predict, then the search, one stream, no host copy in between; d_aid may be NULL (engine scratch).
 *
 * gpsacq_aided_search_iq8: host pointers, returns after completion.  The _device forms: iq, tasks, aid, peaks and the records are
 * device pointers, `in`, eph and the params stay host pointers; work on the engine's stream, sync != 0 waits; host and device form
 * agree byte for byte.  peaks_out must not be peaks_in.  Argument errors are those of gpsacq_aided_search plus those
 * gpsacq_refine_iq8 adds -- in == NULL, a format or multibit value that gpsacq_search_iq8 refuses, a mean beyond +-128 where it is
 * removed, a stride outside the bounds above, a misaligned device pointer: GPSACQ_ERR_ARG, nothing launched and nothing written.
 * GPSACQ_ERR_UNSUPPORTED as gpsacq_aided_search.
 * Kernel (csrc/aided_iq_kernels.hip).  k_aided_iq: one workgroup of four wave64 per task; a wave owns whole segments.  The
 * hypotheses of one (segment, d) share one carrier-wiped series a_j = (v_i C - v_q S, v_i S + v_q C) and one chip stream s', and
 * summation by parts turns sum_j s'[j + h] a_j over a chunk of n samples into
 *     R(h) = s'[M] A[n] - sum over the chip transitions m of the stream of (s'[m] - s'[m - 1]) A[m - h],      M = n + 2 W - 1,
 * with A the prefix sums of a -- exactly, in integers, so the model above does not see it.  Per chunk of 1024 samples the wave
 * writes A into LDS (16-byte groups, the mean taken off per sample, a wave scan) and compacts the stream's transitions into a list
 * (ballot and popcount); lane h then reads one int2 of A per transition, neighbouring lanes neighbouring entries: about 1040 reads
 * per segment at 5.456 MHz where the direct sum has 5456 multiply-adds per hypothesis.  The lane squares its own I and Q into its
 * own uint64; the four waves' sums meet in LDS once per d; the best hypothesis is the maximum of the pair (power, 31 - d, 255 - h).
 * The floor is summed once per segment from the same bytes.  No atomics, no float before the ratio.  Every loop is bounded by
 * kernel arguments, every LDS index by the host-checked limits (spm <= 65535, W <= 127, K <= 8).  DESIGN.md 8.9 has the rest.
 *
 * OUT OF SCOPE.  Accumulated or re-aligned searches, multi-GPU, gps_test and gps_track.  (The multi-bit coherent search is the next
 * section; the weights of gpsacq_refine_iq8 records from the floor law above are "Snapshot signal quality on an 8-bit IQ capture".)
 */
GPSACQ_API int gpsacq_aided_default_params_iq8(gpsacq_aided_params* p);   /* host only */
GPSACQ_API int gpsacq_aided_search_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_aid* aid, const gpsacq_peak* peaks_in /* or NULL */, size_t n_tasks,
                                       const gpsacq_aided_params* params, gpsacq_aided* aided_out, gpsacq_peak* peaks_out,
                                       uint64_t* powers_out /* [n_tasks][2K + 1][2W + 1] or NULL */);
GPSACQ_API int gpsacq_aided_search_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_aid, const void* d_peaks_in, size_t n_tasks,
                                              const gpsacq_aided_params* params, void* d_aided, void* d_peaks_out, void* d_powers_out, int sync);
GPSACQ_API int gpsacq_aided_peaks_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_vel,
                                             const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride, const void* d_tasks,
                                             const void* d_peaks_in, size_t n_fix, int n_chans, const gpsacq_aid_params* aid_params,
                                             const gpsacq_aided_params* aided_params, void* d_aid, void* d_aided, void* d_peaks_out, int sync);
/* device time of the last call of this section on this engine, milliseconds (HIP events on its stream; waits for them): the 8-bit ->
 * 1-bit conversion (sign mode), k_aid_predict (the chain) and the search (k_aided_iq, in sign mode k_aided).  A kernel that the last
 * call did not run reads 0.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_aided_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* predict_ms, float* search_ms);

/*
 * ---- Coherent aided acquisition on an 8-bit IQ capture: multi-bit 20 ms sums ------------------------------------------------------
 *
 * gpsacq_aided_coh_search, the most sensitive step of the library, read a 1-bit stream: a caller with an rtl-sdr or HackRF file went
 * through gpsacq_iq8_to_bits first and paid one arm (3 dB) and the limiter (about 2 dB) exactly where the coherent sums had won their
 * 2.5 dB.  gpsacq_aided_coh_search_iq8 runs the 20 ms sums on the IQ bytes themselves.  THE MODEL; the kernel
 * (csrc/aided_coh_iq_kernels.hip) and the reference of the tests (tests/aided_coh_iq_ref.py) are both written from this text.  It adds
 * no arithmetic of its own: it COMPOSES two sections above, "IQ" = "Aided acquisition on an 8-bit IQ capture" and "COH" = "Coherent
 * aided acquisition", A. SEARCH, each holding word for word except where this text says otherwise.
 *
 * INPUTS.  `in`, iq[2 * n_samples], n_samples, stride (BYTES, a multiple of 16, 80000 <= stride <= 2^31), tasks[n_tasks] (NULL: the
 * reference schedule), aid[n_tasks] and peaks_in[n_tasks] (optional) are IQ's.  The parameters are COH's gpsacq_aided_coh_params with
 * COH's limits: blocks 1 .. 64, min_segments >= 1, W 0 .. 31, K 0 .. 8, M one of 1, 2, 4, 5, 10, 20, F 0 .. 7, u 1 .. 512, keep_snr and
 * ratio_min finite, and fit * (2 W + 1) <= 5120 with fit = blocks * 40000 / spm.
 *
 * in->multibit != 0 (GPSACQ_SAMPLES_REAL and GPSACQ_SAMPLES_COMPLEX alike): THE MULTI-BIT PATH.  PER TASK:
 *   SAMPLE, WINDOW, step 1 (KEPT), step 2 (NO_AID) and step 3 (HYPOTHESES: f_d, lo_rate_d, the valid d, base, P0(h, d), the ONE chip
 *     stream per (segment, d), the carrier phase counted from the window's first sample) are IQ's.
 *   Step 4 (SEGMENT SUMS).  z_s = (I_s, Q_s) of hypothesis (h, d) are IQ's per-segment sums of step 4,
 *         I_s = sum h_P (v_i C - v_q S),   Q_s = sum h_P (v_i S + v_q C)     over the spm samples of segment s,
 *     kept with their signs and NOT squared.
 *   Step 5 (COHERENT SUMS) is COH's step 5 on these z_s: the same ROTATION TABLE, k_s = (f u s) mod 1024, A_s = I_s C[k_s] + Q_s S[k_s],
 *     B_s = Q_s C[k_s] - I_s S[k_s] in int64, the period boundaries {0, S} and every 0 < s < S with s = e (mod M), the partial
 *     periods at both ends counted, A' = floor((sum of A_s over the period) / 2^14) -- the shift AFTER the sum -- and
 *         power(h, d, g, e) = sum over the periods of A'^2 + B'^2,  uint64.
 *     BOUNDS.  They differ from COH's and decide the kernel's integer types.  |v_i|, |v_q| <= 256, so a sample adds at most 512 to
 *     either sum: |I_s|, |Q_s| <= 512 spm < 2^25.  By Cauchy-Schwarz I_s^2 <= spm * sum (v_i C - v_q S)^2 and likewise Q_s^2, and the
 *     two sums of squares add up to 2 sum (v_i^2 + v_q^2) <= spm * 2^18: I_s^2 + Q_s^2 <= 2^18 spm^2.  |A_s|, |B_s| <=
 *     sqrt(I_s^2 + Q_s^2) sqrt(C^2 + S^2) <= 2^9 spm (2^14 + 1) < 2^40: every product with the int16 table is a 64-bit product.  A
 *     prefix over fewer than 2^12 segments stays below 2^52, a period of at most 20 segments below 2^45, A' below 2^30 (so A'^2 +
 *     B'^2 < 2^61).  A period of n segments adds at most n^2 2^18 spm^2 (1 + 2^-13), and the n of a partition add up to S with n <=
 *     M: power <= M S 2^18 spm^2 (1 + 2^-13) <= 20 * 2^18 * 65535 * (64 * 40000) * (1 + 2^-13) = 2^59.6 < 2^60 -- it fits uint64,
 *     and it does NOT fit the 44 bits COH's packed key gives a power.  (The library still refuses, GPSACQ_ERR_UNSUPPORTED, an engine
 *     and parameters with M * (2^18 + 2^5) * spm * (blocks * 40000) >= 2^63; the limits above leave none.)
 *     With M = 1 and F = 0 every period is one segment and C[0] = 2^14, S[0] = 0: power(h, d, 0, 0) is gpsacq_aided_search_iq8's
 *     power(h, d) bit for bit (a test uses it).
 *   Step 6 (RECORD) is COH's gpsacq_aided_coh with
 *       best, its place (best_d, best_f, best_e, best_h): the largest KEY (power, -d, -g, -e, -h) in lexicographic order, whatever the
 *                 order of any reduction (the kernel compares the pair (power, 31 - d << 15 | 15 - g << 11 | 31 - e << 6 | 63 - h))
 *       noncoh  = the sum over the segments of I_s^2 + Q_s^2 at (best_h, best_d): gpsacq_aided_search_iq8's power there
 *       floor   = IQ's MEASURED FLOOR, 2 * (sum over the samples of the window's segments of v_i^2 + v_q^2): what a +-1 replica
 *                 uncorrelated with the samples leaves in a period of n segments is the sum of its segments' floors, so the
 *                 partition into periods does not change it
 *       ratio, lo_shift, ca_shift, doppler_hz, best_e, reserved, the flags and the OUTPUT PEAK as in COH.
 *   Step 7: powers_out[n_tasks][2K + 1][2F + 1][M][2W + 1] as in COH.
 *
 * in->multibit == GPSACQ_SAMPLES_SIGN: the capture is converted once per call into engine scratch by the path gpsacq_aided_search_iq8
 * uses, and k_aided_coh runs on it with n_bytes = ceil(n_samples / 8) and stride / 16: the result is byte for byte
 * gpsacq_iq8_to_bits_device followed by gpsacq_aided_coh_search_device.
 *
 * DEFAULT RATIO_MIN.  gpsacq_aided_coh_default_params_iq8 (host only) sets gpsacq_aided_coh_default_params' values with ratio_min
 * measured for the multi-bit path; a NULL params of this section's calls means these in multi-bit mode and
 * gpsacq_aided_coh_default_params' in sign mode.  Measured as both sections above did (tools/aided_floor.py --iq8 --coherent, on the
 * CPU with tests/aided_coh_iq_ref.py's quick spellings): the --iq8 scene (eight satellites at amplitude 0.2, noise sigma 1, fs = 5.456
 * MHz, IF 0.4 MHz, scale 16, int8, the mean not removed) with the random navigation bits of --coherent on its eight satellites,
 * searched for its 24 ABSENT PRNs with the defaults, 2304 draws of 13 860 hypotheses each: the largest ratio was 23.0511 (median
 * 7.4827, 99.9 % below 19.0240).  The default is that plus a quarter of its excess over 1: 23.0511 + 22.0511 / 4 = 28.56.  That is 2.7
 * times COH's 10.73, and as there it is not noise: it is the C/A cross-correlation of the eight satellites at amplitude 0.2, which a
 * 20 ms sum adds up coherently wherever a Doppler difference is close to a multiple of 1 kHz, and which keeps both arms and passes no
 * limiter here exactly as the signal sought does.  It belongs to the defaults and to that scene; a caller with fewer or weaker
 * satellites beside the signal measures a lower one and keeps more of the gain.
 * WHAT TO EXPECT.  Measured on the CPU (tests/test_aided_coh_iq.py: tests/test_aided_coh.py's scene -- 16 blocks, five satellites at
 * 0.2 with navigation bits beside the weak one, two absent PRNs -- written as an 8-bit IQ capture, the same bytes searched multi-bit
 * and through the sign path, tests/iq_ref.py's conversion followed by tests/aided_coh_ref.py): at amplitude 0.0337 the weak satellite
 * reads ratio 28.19 multi-bit where the sign path reads 10.64, both at the true code phase, bit edge 7 and 384.8 Hz against the
 * generator's 389.8; the absent PRNs read 3.36 and 7.35 against 3.11 and 3.89, so the weak satellite stands 3.84 times above the
 * larger absent ratio multi-bit and 2.74 times through the sign path.  Over amplitudes (one capture each): 0.02 reads 9.28 against
 * 4.50, 0.025 reads 14.76 against 6.39, 0.03 reads 21.88 against 8.71, 0.035 reads 30.58 against 11.34 and 0.04 reads 40.79 against
 * 14.69 (gpsacq_aided_search_iq8 reads 1.76, 2.07, 2.45, 2.91 and 3.45 there).  The excess over 1 is 2.7 to 2.9 times the sign path's, about 4.5 dB --
 * the arm and the limiter -- but in this scene the measured thresholds rose alike (28.56 against 10.73): both defaults begin to
 * detect at about amplitude 0.034, where gpsacq_aided_search_iq8's 3.44 needs 0.04.  What the multi-bit sums buy with the defaults is
 * the margin over the absent PRNs, not a lower first amplitude; a caller whose scene has no eight satellites at 0.2 measures a lower
 * ratio_min (tools/aided_floor.py --iq8 --coherent) and keeps the 4.5 dB.  Measured on an MI355X
 * (tools/snapshot_bench.py --iq8 --aided-coh, 1024 blocks, eight satellites at 0.2, two weak ones and two absent PRNs per block,
 * navigation bits on, the three searches on the same tasks in the same run with their own defaults, HIP events, shader clock not read):
 * at amplitude 0.03 this search detects 1309 of the 2047 weak tasks the plain search had missed, the sign-path coherent search 960
 * and gpsacq_aided_search_iq8 77 (median ratios 30.23, 10.59 and 2.83); at 0.025 it detects 194 of 2048, the sign path 168 (one of them
 * off the true code phase) and the non-coherent search none (21.60, 7.91, 2.37); at 0.035 1990, 1807 and 878 of 2042 (40.47, 13.82,
 * 3.38).  Every other detection lies at the true code phase, and no search detects any of the 2048 absent tasks (largest ratios 11.45,
 * 6.83 and 2.75).  At 0.03 doppler_hz is 5.6 Hz rms from the generator's (sign path 6.1) and best_e equals its edge in 78 % of the
 * detections, within one segment in 98 % (sign path 64 % and 93 %).  k_aided_coh_iq 44.16 ms for 4095 tasks of 13 860 hypotheses beside
 * k_aided_iq 40.87 ms (1.08 times) and 6.93 ms for the conversion and k_aided_coh (6.4 times).  So on the bench scene, whose measured
 * floor it is, the default detects about a third more weak satellites at 0.03 than the sign path does; DESIGN.md 8.10 has the rest.
 *
 * THE CHAIN.  gpsacq_aided_coh_peaks_iq8_device is gpsacq_aided_coh_peaks_device with (in, d_iq, n_samples) for (d_bits, n_bytes):
 * k_aid_instant (skipped where d_info == NULL; d_prior is then not read), then k_aid_predict, then the search, one stream, no host
 * copy in between; d_fix_instant and d_aid may be NULL (engine scratch).  The results are exactly what the three calls give.
 *
 * gpsacq_aided_coh_search_iq8: host pointers, returns after completion.  The _device forms: iq, tasks, aid, peaks and the records are
 * device pointers (iq 16-byte aligned), `in`, eph and the params stay host pointers; work on the engine's stream, sync != 0 waits;
 * host and device form agree byte for byte.  peaks_out must not be peaks_in.  Argument errors are those of gpsacq_aided_search_iq8
 * plus those of gpsacq_aided_coh_search (coh_ms outside its set, F, u, W, K outside their ranges; the chain: coarse-time records
 * without their priors): GPSACQ_ERR_ARG, nothing launched and nothing written.  GPSACQ_ERR_UNSUPPORTED: everything
 * gpsacq_aided_search_iq8 refuses, fit * (2W + 1) > 5120, and the bound of step 5; nothing launched and nothing written either.
 * Kernel (csrc/aided_coh_iq_kernels.hip).  k_aided_coh_iq<M>: one workgroup of four wave64 per task, two stages per d.  The
 * CORRELATION STAGE is k_aided_iq's WIPE / STREAM / SUM by summation by parts at one pass (W <= 31: lane h serves hypothesis h), the
 * one chunk walk both kernels call (csrc/aided_iq_walk.hpp), entered once per (segment, d) and never per g or e; lane h stores (I, Q)
 * as an int32 pair into z[s][h] in LDS, and the floor's sum rides along at the first valid d.  The COHERENT STAGE is k_aided_coh's
 * walk over the work items (h, g) -- prefix sums of the turned series, M accumulators with constant indices, edge e = s mod M closed
 * at segment s -- with 64-bit products, reducing the pair key.  A chunk of 512 samples keeps its LDS at 70 864 bytes: two workgroups
 * per CU.  No atomics, no scratch, no float before the ratio; every loop is bounded by kernel arguments, every LDS index by the
 * host-checked limits.  DESIGN.md 8.10 has the rest.
 *
 * OUT OF SCOPE.  W above 31.  Accumulated or re-aligned searches, multi-GPU, gps_test and gps_track.  (C/N0 and weights for the peaks
 * found here: the next section.)
 */
GPSACQ_API int gpsacq_aided_coh_default_params_iq8(gpsacq_aided_coh_params* p);   /* host only */
GPSACQ_API int gpsacq_aided_coh_search_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                           const gpsacq_task* tasks, const gpsacq_aid* aid, const gpsacq_peak* peaks_in /* or NULL */, size_t n_tasks,
                                           const gpsacq_aided_coh_params* params, gpsacq_aided_coh* aided_out, gpsacq_peak* peaks_out,
                                           uint64_t* powers_out /* [n_tasks][2 K + 1][2 F + 1][M][2 W + 1] or NULL */);
GPSACQ_API int gpsacq_aided_coh_search_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                                  const void* d_tasks, const void* d_aid, const void* d_peaks_in, size_t n_tasks,
                                                  const gpsacq_aided_coh_params* params, void* d_aided, void* d_peaks_out, void* d_powers_out, int sync);
GPSACQ_API int gpsacq_aided_coh_peaks_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const void* d_fix, const void* d_info /* or NULL */,
                                                 const void* d_prior, const void* d_vel, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples,
                                                 size_t stride, const void* d_tasks, const void* d_peaks_in, size_t n_fix, int n_chans,
                                                 const gpsacq_aid_params* aid_params, const gpsacq_aided_coh_params* coh_params, void* d_fix_instant,
                                                 void* d_aid, void* d_aided, void* d_peaks_out, int sync);
/* device time of the last call of this section on this engine, milliseconds (HIP events on its stream; waits for them): the 8-bit ->
 * 1-bit conversion (sign mode), k_aid_instant and k_aid_predict (the chain) and the search (k_aided_coh_iq, in sign mode k_aided_coh).
 * A kernel that the last call did not run reads 0.  Any pointer may be NULL. */
GPSACQ_API int gpsacq_aided_coh_iq8_last_ms(const gpsacq_engine* e, float* convert_ms, float* instant_ms, float* predict_ms, float* search_ms);

/*
 * ---- Snapshot signal quality on an 8-bit IQ capture: measured floor, C/N0 and weights ----------------------------------------------
 *
 * gpsacq_aided_search_iq8 and gpsacq_aided_coh_search_iq8 dig out satellites 10 to 15 dB below the search threshold, their peaks go
 * through gpsacq_refine_iq8 and gpsacq_coarse_obs_fine into gpsacq_coarse_fix_batch -- at weight 1.0, the problem "Snapshot signal
 * quality" solved for the 1-bit chain.  Its floor, 2 * spm * segments, is that of a +-1 stream; the prompt power of a multi-bit record
 * scales with the capture's amplitude.  This section measures the floor on the capture's own bytes, by the law of "Aided acquisition
 * on an 8-bit IQ capture", step 5, and everything after the floor is "Snapshot signal quality" word for word.  THE MODEL; the kernels
 * (csrc/snapq_iq_kernels.hip) and the reference of the tests (tests/snapq_iq_ref.py) are both written from this text.
 *
 * INPUTS.  `in`, iq[2 * n_samples], n_samples and stride exactly as for gpsacq_refine_iq8: stride in BYTES, a multiple of 16,
 * 80000 <= stride <= 2^31; the device form takes a 16-byte-aligned device pointer.  tasks[n_tasks] (NULL: the reference schedule,
 * task t = block t).  fine[n_fix][n_chans]: the records gpsacq_refine_iq8 returned for those tasks with the same `in` and stride,
 * n_tasks = n_fix * n_chans, index-parallel.  A gpsacq_snap_quality_params.  spm = gpsacq_info.num_lags and fs are the engine's.
 *
 * in->multibit != 0 (GPSACQ_SAMPLES_REAL and GPSACQ_SAMPLES_COMPLEX alike): THE MULTI-BIT PATH, per record.
 * 1. NO RECORD is step 1 of "Snapshot signal quality" (a flag of GPSACQ_FINE_NO_HIT, _NO_POWER, _FEW, or segments <= 0), and also
 *    a record that is not of this capture: with o = block * (stride / 2), a block < 0, o beyond n_samples or o + segments * spm
 *    beyond n_samples.  The info is the flag GPSACQ_QUALITY_NO_RECORD and zeros, the floor reads 0, the weight is 0.  Nothing at or
 *    beyond byte 2 * n_samples is read, and such a record reads no byte at all.
 * 2. FLOOR.
 *      floor = 2 * (sum over the samples o .. o + segments * spm - 1 of v_i^2 + v_q^2)
 *    with v the SAMPLE of "Snapshot chain on an 8-bit IQ capture": v = byte - off - dc, off = 128 for GPSACQ_IQ_U8 and 0 for
 *    GPSACQ_IQ_S8, dc = nearbyint(mean) (ties to even) when remove_dc, else 0.  The window is the record's own `segments`: there is no
 *    blocks parameter that could disagree with the record.  uint64, below 2^46 by that section's bound (2 * 2^17 per sample, fewer than
 *    2^12 segments of at most 65535 samples for a record of gpsacq_refine_iq8).  For the same task, blocks and min_segments it is bit
 *    for bit the `floor` field of gpsacq_aided_search_iq8's record (a test uses it), and for a +-1 real stream it is 2 * spm * segments.
 *    floor == 0 (an all-zero window): sig = 0, noise = 0 and the flag GPSACQ_QUALITY_NO_POWER, as step 3 below has it.
 * 3. sig = prompt > floor ? prompt - floor : 0 and noise = floor; then steps 3 to 7 of "Snapshot signal quality" word for word: snr,
 *    lin, cn0_dbhz, GPSACQ_QUALITY_SHORT, the gate, the weight.  The INFO record and THE OBSERVATION are that section's.
 *
 * in->multibit == GPSACQ_SAMPLES_SIGN: the records are 1-bit records, the capture is not read, and the result is byte for byte
 * gpsacq_snap_quality's; gpsacq_snap_floor_iq8 writes 2 * spm * segments, 0 where step 1 of "Snapshot signal quality" says NO RECORD.
 *
 * PARAMETERS.  gpsacq_snap_quality_default_params_iq8 (host only): min_segments 1, reserved 0, cn0_min_lin 1432.4, cn0_ref_lin
 * 10^(48.6/10) (pow(10.0, 4.86)); the valid ranges are gpsacq_snap_quality_default_params'.  params NULL = these in multi-bit mode and
 * gpsacq_snap_quality_default_params' in sign mode.  Both are CPU measurements with the references alone, no GPU:
 *   THE REFERENCE LEVEL is the median C/N0 of the amplitude-0.2 satellites of the bench scene rounded to 0.1 dB, as the 1-bit default
 *   was set: `python tools/snap_quality_law.py --iq8 --scene bench` (60 captures of the eight satellites as an 8-bit IQ capture by
 *   tests/gen_ref.py: int8, scale 16, sigma 1, IF 0.4 MHz, the mean not removed; tests/refine_iq_ref.py, tests/snapq_iq_ref.py) reads a
 *   median of 48.565 dB-Hz over 480 records (47.96 .. 48.94).  That is 5.0 dB above the 1-bit chain's 43.5: the arm and the limiter.
 *   THE GATE.  The largest lin of absent PRNs, one hypothesis each at a random code phase and Doppler bin, on the scene of
 *   tools/aided_floor.py --iq8: `python tools/snap_quality_floor.py` (2304 draws: 8 window starts x 6 bins x 24 absent PRNs x 2 code
 *   phases, 16-block windows) reads at most 1145.93 Hz (median 270.13, 99.9 % below 1069.02).  The default is the larger of 500.0 and
 *   that maximum plus a quarter of it: 1145.93 + 286.48 = 1432.4 Hz (31.6 dB-Hz).  Noise alone would stand at 92 Hz as in "Snapshot
 *   signal quality"; the rest is the C/A cross-correlation of eight satellites at 0.2, which keeps both arms and passes no limiter here
 *   exactly as the signal sought does (as DEFAULT RATIO_MIN of "Aided acquisition on an 8-bit IQ capture" found).  A caller with fewer
 *   or weaker satellites beside the signal measures a lower gate with the same tool and keeps more: on a scene of four satellites at
 *   0.2 (tests/test_snap_quality_iq.py, 24 captures) 48 absent records read at most 384 Hz and an amplitude of 0.025 reads 756 Hz
 *   and more.
 *
 * LIMITS OF THE MODEL.  The figure is C over (N0 plus every other satellite's power in the band), not C / N0 of the antenna: the
 * floor is everything in the samples, the strong satellites included -- four of them at 0.2 beside sigma 1 are 0.08 of the power,
 * about 0.3 dB -- and the satellite's own power too.  The prompt replica sits at the peak's whole sample and bin, as in "Snapshot
 * signal quality" (up to 0.9 dB and 0.07 dB low).  An aided peak is the largest of its hypotheses and reads high.  The weights against
 * the measured range variance, on the CPU (`python tools/snap_quality_law.py --iq8`, 60 captures, amplitudes 0.2 .. 0.03 at 16
 * blocks): C/N0 48.5, 42.6, 39.5, 36.7, 34.9 and 32.7 dB-Hz, variance ratio 1, 0.85, 0.42, 0.18, 0.13 and 0.07; the table of the
 * weights is in README.md.  No claim below cn0_min_lin.
 *
 * THE ENERGY PASS.  Every call of the multi-bit path reads the capture once, bytes 0 .. 2 * n_samples - 1 whatever the tasks are
 * (k_iq_energy, below), into engine scratch of n_samples / 1024 uint64: a caller with few tasks on a long capture passes the stretch
 * its tasks lie in.  The floors then cost a few reads per task.  Measured on an MI355X (tools/snapshot_bench.py --iq8 --aided
 * --quality: 2048 blocks, a 169 MB capture that k_refine_iq had just read, 24 576 records, HIP events, best of 5, shader clock not
 * read): k_iq_energy and k_snap_floor together 0.044 ms and k_snap_quality_iq 0.007 ms beside k_refine_iq 26.42 ms of the same call,
 * and a device-to-device copy of the same capture 0.074 ms in the same run; the strong satellites read 48.37 dB-Hz in the median and
 * the weak pair at amplitude 0.05 36.60; position error of the same 2048 blocks, median / worst, 3.53 / 11.75 m from the strong
 * eight, 4.02 / 11.93 m with the weak pair at unit weight, 3.40 / 11.31 m with these weights.  A capture that is not in cache was
 * not measured.
 *
 * gpsacq_snap_floor_iq8 writes floor_out[n_tasks], 0 where step 1 says NO RECORD.  gpsacq_snap_quality_iq8: obs in-out and may be
 * NULL, info out.  Host pointers, return after completion.  The _device forms: iq, tasks, fine, obs, floor and info are device
 * pointers, `in` and params stay host pointers; work on the engine's stream, sync != 0 waits; host and device form agree byte for
 * byte.  d_floor[n_tasks] of gpsacq_snap_quality_iq8_device and of the chain may be NULL (engine scratch), as d_fine elsewhere; in
 * sign mode it is written only where it is given.  gpsacq_coarse_fix_quality_iq8_device is gpsacq_coarse_fix_quality_device with (in,
 * d_iq, n_samples) for (d_bits, n_bytes): refine, observations, floors, weights and fix on one stream with no host copy in between,
 * the same optional buffers.  Argument errors are those of gpsacq_refine_iq8 with fine for peaks -- a NULL in, iq, fine or output, no
 * task, a format or multibit value that gpsacq_search_iq8 refuses, a mean beyond +-128 where it is removed, a stride outside the
 * bounds above, a misaligned device pointer -- plus n_chans outside 1..GPSACQ_FIX_MAX_SATS, a parameter out of range and for the
 * chain those of gpsacq_coarse_fix_fine_iq8_device: GPSACQ_ERR_ARG, nothing launched and nothing written.
 * Kernels (csrc/snapq_iq_kernels.hip).  k_iq_energy: one streaming pass, one wave64 per chunk of 1024 samples; 16-byte loads, bytes
 * XORed with 0x80 for GPSACQ_IQ_U8, the squares of a dword as its 4 x int8 dot product with itself, the mean as the exact correction
 * S2 - 2 (dc_i S_i + dc_q S_q) + n (dc_i^2 + dc_q^2) only where it is not zero; xor shuffles, one writer per chunk.  k_snap_floor: one
 * wave64 per task; the window is a head up to the next chunk boundary, whole chunks (their E entries, summed by the wave) and a tail;
 * only head and tail are read from the bytes.  k_snap_quality_iq: one lane per (fix, channel), k_snap_quality's arithmetic
 * (csrc/snapq_device.hpp, one copy for both).  No atomics, no float before snr, nothing that depends on an order; every loop is
 * bounded by kernel arguments.  DESIGN.md 8.11 has the rest.
 *
 * OUT OF SCOPE.  Per-observation sigmas in gpsacq_raim_params, weights for whole-sample observations without a fine record, a floor
 * for the tracking chain's multi-bit channels, gps_test and gps_track, multi-GPU.
 */
GPSACQ_API int gpsacq_snap_quality_default_params_iq8(gpsacq_snap_quality_params* p);   /* host only */
GPSACQ_API int gpsacq_snap_floor_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                     const gpsacq_task* tasks, const gpsacq_fine* fine, size_t n_tasks, uint64_t* floor_out);
GPSACQ_API int gpsacq_snap_floor_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                            const void* d_tasks, const void* d_fine, size_t n_tasks, void* d_floor, int sync);
GPSACQ_API int gpsacq_snap_quality_iq8(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* iq, size_t n_samples, size_t stride,
                                       const gpsacq_task* tasks, const gpsacq_fine* fine /* [n_fix][n_chans] */, size_t n_fix, int n_chans,
                                       const gpsacq_snap_quality_params* params, gpsacq_obs* obs /* in-out, or NULL */, gpsacq_quality_info* info);
GPSACQ_API int gpsacq_snap_quality_iq8_device(gpsacq_engine* e, const gpsacq_iq8_input* in, const void* d_iq, size_t n_samples, size_t stride,
                                              const void* d_tasks, const void* d_fine, size_t n_fix, int n_chans,
                                              const gpsacq_snap_quality_params* params, void* d_obs, void* d_floor, void* d_info, int sync);
GPSACQ_API int gpsacq_coarse_fix_quality_iq8_device(gpsacq_engine* e, const gpsacq_ephemeris* eph, int n_eph, const gpsacq_iq8_input* in, const void* d_iq,
                                                    size_t n_samples, size_t stride, const void* d_tasks, const void* d_peaks, size_t n_fix, int n_chans,
                                                    const gpsacq_refine_params* refine_params, const gpsacq_snap_quality_params* quality_params,
                                                    const void* d_prior, const gpsacq_coarse_params* params, void* d_fine, void* d_obs, void* d_floor,
                                                    void* d_qinfo, void* d_fix, void* d_info, void* d_obs_out, int sync);
/* device time of the last call of this section on this engine, milliseconds (HIP events on its stream; waits for them): the floor
 * kernels (k_iq_energy and k_snap_floor together) and the quality kernel (k_snap_quality_iq, in sign mode k_snap_quality).  A stage
 * that the last call did not run reads 0.  Either pointer may be NULL. */
GPSACQ_API int gpsacq_snap_quality_iq8_last_ms(const gpsacq_engine* e, float* floor_ms, float* quality_ms);

/* SearchCode(): chips to clock PRN sv's generator until its G1 register reads g1 (-1 if never) */
GPSACQ_API int gpsacq_search_code(int sv, int g1);

/* Parity probes (natural bin order, interleaved re/im, 40000 complex floats each). */
GPSACQ_API int gpsacq_sample_spectrum(gpsacq_engine* e, const uint8_t* block5120, float* out);
GPSACQ_API int gpsacq_code_spectrum(gpsacq_engine* e, int sv, float* out);

#ifdef __cplusplus
}
#endif
#endif /* GPSACQ_H */
