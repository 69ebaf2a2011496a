"""ctypes binding of libgpsacq.so (include/gpsacq.h) -- the MI355X GPS L1 C/A acquisition engine.

Thin on purpose: every number comes out of the HIP kernels behind the C ABI.  If the shared
library (built by `make lib` / __graft_entry__.build()) is missing this module raises; there
is no Python or CPU fallback for the search.

Reference interface mirrored (JiaoXianjun/GNSS-GPS-SDR, c/gps_offline.h:87-91 and the globals
FC/FS/max_fo of c/gps_offline.h:23-25): `Engine(fc, fs, max_fo)` is SearchInit(),
`Engine.search()` is the Sample()+Correlate() body of SearchTask()'s loop
(c/search_offline.cpp:239-246), `Engine.close()` is SearchFree(), `search_code()` is SearchCode().
"""
import ctypes
import os

import numpy as np

FFT_LEN = 40000
NUM_SATS = 32
BLOCK_BYTES = 5120
THRESHOLD = 25.0  # c/search_offline.cpp:248
STAMP_SLOTS = 512  # GPSACQ_STAMP_SLOTS: one cycle-counter slot per (XCD, shader engine, compute unit)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPSACQ_LIB") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libgpsacq.so"))

CELL_DTYPE = np.dtype([("max_pwr", "<f4"), ("max_i", "<i4"), ("tot_pwr", "<f4"), ("snr", "<f4")])
PEAK_DTYPE = np.dtype([("snr", "<f4"), ("lo_shift", "<i4"), ("ca_shift", "<i4"), ("max_pwr", "<f4")])
TASK_DTYPE = np.dtype([("block", "<i4"), ("prn", "<i4")])


class Params(ctypes.Structure):
    _fields_ = [("fc", ctypes.c_double), ("fs", ctypes.c_double), ("max_fo", ctypes.c_double),
                ("device", ctypes.c_int32), ("ref_quirks", ctypes.c_int32)]


class Info(ctypes.Structure):
    _fields_ = [("fft_len", ctypes.c_int32), ("dmax", ctypes.c_int32), ("num_doppler", ctypes.c_int32),
                ("first_doppler", ctypes.c_int32), ("num_lags", ctypes.c_int32), ("acc_columns", ctypes.c_int32), ("device", ctypes.c_int32),
                ("compute_units", ctypes.c_int32), ("device_name", ctypes.c_char * 64),
                ("doppler_sub", ctypes.c_int32), ("doppler_stride", ctypes.c_int32), ("num_doppler_total", ctypes.c_int32),
                ("first_doppler_total", ctypes.c_int32), ("doppler_step_hz", ctypes.c_double)]


class Timing(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_float), ("ms_sample", ctypes.c_float), ("ms_correlate", ctypes.c_float),
                ("ms_peaks", ctypes.c_float), ("correlate_launches", ctypes.c_int32), ("cells", ctypes.c_int64)]


class Handoff(ctypes.Structure):
    _fields_ = [("lo_dop_hz", ctypes.c_double), ("ca_dop_hz", ctypes.c_double), ("lo_rate", ctypes.c_uint32),
                ("ca_rate", ctypes.c_uint32), ("ca_shift", ctypes.c_int32), ("ca_pause", ctypes.c_uint32)]


class Iq8Input(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("remove_dc", ctypes.c_int32), ("mean_i", ctypes.c_double), ("mean_q", ctypes.c_double),
                ("mix_hz", ctypes.c_double), ("fs", ctypes.c_double), ("first_sample", ctypes.c_uint64), ("total_samples", ctypes.c_uint64),
                ("multibit", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Sat(ctypes.Structure):
    _fields_ = [("prn", ctypes.c_int32), ("amplitude", ctypes.c_float), ("doppler_hz", ctypes.c_double),
                ("code_phase_samples", ctypes.c_double), ("carrier_phase_cycles", ctypes.c_double)]


# tracking channels and NAV data (include/gpsacq.h, "Tracking channels and NAV data")
TRACK_OK, TRACK_LOST = 0, 1
TRACK_CHAN_DTYPE = np.dtype([("prn", "<i4"), ("status", "<i4"), ("next_sample", "<u8"), ("lo_phase", "<u4"), ("lo_rate", "<u4"),
                             ("lo_int", "<i8"), ("ca_pos", "<u8"), ("ca_rate", "<u4"), ("epoch", "<i4"), ("ca_int", "<i8"),
                             ("lo_nom", "<i8"), ("ca_nom", "<i8"), ("gain_adj", "<i4"), ("pwr_pos", "<i4"), ("pwr", "<i8", (8,)),
                             ("prev_ip", "<i4"), ("prev_qp", "<i4"), ("fll_left", "<i4"), ("reserved", "<i4")])
TRACK_RECORD_DTYPE = np.dtype([("sample", "<u8"), ("ie", "<i4"), ("qe", "<i4"), ("ip", "<i4"), ("qp", "<i4"), ("il", "<i4"),
                               ("ql", "<i4"), ("lo_rate", "<u4"), ("ca_rate", "<u4")])
SUBFRAME_DTYPE = np.dtype([("bit_offset", "<i4"), ("inverted", "<i4"), ("words", "<u4", (10,)), ("id", "<i4"), ("tow", "<i4")])

# navigation solver (include/gpsacq.h, "Navigation solver")
FIX_OK, FIX_TOO_FEW, FIX_NO_CONVERGE = 0, 1, 2
FIX_MAX_SATS = 12
EPHEMERIS_DTYPE = np.dtype([("prn", "<i4"), ("have", "<i4"), ("week", "<u4"), ("iodc", "<u4"), ("iode2", "<u4"), ("iode3", "<u4"),
                            ("t_oc", "<u4"), ("t_oe", "<u4"), ("tow", "<i4"), ("reserved", "<i4"),
                            ("t_gd", "<f8"), ("a_f0", "<f8"), ("a_f1", "<f8"), ("a_f2", "<f8"),
                            ("c_rs", "<f8"), ("dn", "<f8"), ("m_0", "<f8"), ("c_uc", "<f8"), ("e", "<f8"), ("c_us", "<f8"), ("sqrt_a", "<f8"),
                            ("c_ic", "<f8"), ("omega_0", "<f8"), ("c_is", "<f8"), ("i_0", "<f8"), ("c_rc", "<f8"), ("omega", "<f8"),
                            ("omega_dot", "<f8"), ("idot", "<f8")])
OBS_DTYPE = np.dtype([("eph", "<i4"), ("valid", "<i4"), ("tx_ms", "<i4"), ("reserved", "<i4"), ("tx_frac", "<f8"), ("weight", "<f8")])
SAT_STATE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("clock_corr", "<f8")])
FIX_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("iterations", "<i4"), ("rx_ms", "<i4"), ("rx_frac", "<f8"),
                      ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("lat", "<f8"), ("lon", "<f8"), ("alt", "<f8"), ("rms", "<f8")])
# observables (include/gpsacq.h, "Observables")
TIME_TAG_DTYPE = np.dtype([("epoch", "<i4"), ("ms", "<i4"), ("eph", "<i4"), ("valid", "<i4")])
# carrier observables and velocity (include/gpsacq.h, "Carrier observables", "Velocity and clock drift")
RATE_OBS_DTYPE = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("adr", "<i8"), ("doppler_hz", "<f8"), ("weight", "<f8")])
SAT_RATE_DTYPE = np.dtype([("vx", "<f8"), ("vy", "<f8"), ("vz", "<f8"), ("clock_drift", "<f8")])
VEL_OK, VEL_TOO_FEW, VEL_NO_FIX, VEL_SINGULAR = 0, 1, 2, 3
VEL_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("vx", "<f8"), ("vy", "<f8"), ("vz", "<f8"), ("ve", "<f8"), ("vn", "<f8"),
                      ("vu", "<f8"), ("drift", "<f8"), ("rms", "<f8")])
# atmosphere, elevation mask and DOP (include/gpsacq.h, "Atmosphere, elevation mask and DOP")
ATM_IONO, ATM_TROPO, ATM_ROUNDS = 1, 2, 3
IONO_DTYPE = np.dtype([("valid", "<i4"), ("tow", "<i4"), ("alpha", "<f8", (4,)), ("beta", "<f8", (4,))])
ATM_PARAMS_DTYPE = np.dtype([("alpha", "<f8", (4,)), ("beta", "<f8", (4,)), ("elev_mask", "<f8"), ("flags", "<i4"), ("reserved", "<i4")])
SAT_VIEW_DTYPE = np.dtype([("az", "<f8"), ("el", "<f8"), ("iono_m", "<f8"), ("tropo_m", "<f8")])
FIX_DOP_DTYPE = np.dtype([("used_mask", "<u4"), ("n_masked", "<i4"), ("gdop", "<f8"), ("pdop", "<f8"), ("hdop", "<f8"), ("vdop", "<f8"),
                          ("tdop", "<f8")])
# fix integrity (include/gpsacq.h, "Fix integrity: residual test and single-satellite exclusion")
RAIM_MAX_DOF = 8
RAIM_NONE, RAIM_UNCHECKED, RAIM_PASS, RAIM_EXCLUDED, RAIM_FAILED = 0, 1, 2, 3, 4
RAIM_PARAMS_DTYPE = np.dtype([("sigma_m", "<f8"), ("p_fa", "<f8"), ("threshold", "<f8", (RAIM_MAX_DOF,)), ("exclude", "<i4"), ("reserved", "<i4")])
FIX_RAIM_DTYPE = np.dtype([("status", "<i4"), ("dof", "<i4"), ("excluded", "<i4"), ("n_candidates", "<i4"), ("stat_full", "<f8"), ("stat", "<f8"),
                           ("threshold", "<f8")])
# coarse-time fixes (include/gpsacq.h, "Coarse-time fixes: positions from code phases alone")
COARSE_INCONSISTENT = 1
COARSE_PRIOR_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("rx_ms", "<i4"), ("reserved", "<i4")])
COARSE_PARAMS_DTYPE = np.dtype([("rms_max_m", "<f8"), ("reserved", "<f8")])
COARSE_INFO_DTYPE = np.dtype([("ref", "<i4"), ("flags", "<i4"), ("coarse_s", "<f8"), ("bias_m", "<f8"), ("pdop", "<f8"), ("cdop", "<f8")])
# fine code phases (include/gpsacq.h, "Fine code phases: search peaks refined below a sample")
FINE_NO_HIT, FINE_SHORT, FINE_NO_POWER, FINE_FEW = 1, 2, 4, 8
REFINE_PARAMS_DTYPE = np.dtype([("blocks", "<i4"), ("min_segments", "<i4"), ("half_spacing_chips", "<f8"), ("snr_min", "<f8")])
FINE_DTYPE = np.dtype([("flags", "<i4"), ("segments", "<i4"), ("lo_rate", "<u4"), ("ca_rate", "<u4"), ("early", "<u8"), ("prompt", "<u8"),
                       ("late", "<u8"), ("offset_chips", "<f8"), ("tx_frac", "<f8")])
# cold snapshot fixes (include/gpsacq.h, "Cold snapshot fixes: fine Doppler and a Doppler-only position solver")
DOPFINE_NO_HIT, DOPFINE_SHORT, DOPFINE_NO_POWER, DOPFINE_FEW, DOPFINE_WEAK = 1, 2, 4, 8, 16
DOPPLER_INCONSISTENT = 1
DOPFINE_PARAMS_DTYPE = np.dtype([("blocks", "<i4"), ("min_segments", "<i4"), ("snr_min", "<f8"), ("coherence_min", "<f8")])
DOPFINE_DTYPE = np.dtype([("flags", "<i4"), ("segments", "<i4"), ("lo_rate", "<u4"), ("ca_rate", "<u4"), ("re", "<i8"), ("im", "<i8"),
                          ("mag", "<u8"), ("power", "<u8"), ("coherence", "<f8"), ("df_hz", "<f8"), ("doppler_hz", "<f8")])
DOPPLER_FIX_PARAMS_DTYPE = np.dtype([("rms_max_mps", "<f8"), ("reserved", "<f8")])
DOPPLER_FIX_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("iterations", "<i4"), ("flags", "<i4"), ("x", "<f8"), ("y", "<f8"),
                              ("z", "<f8"), ("lat", "<f8"), ("lon", "<f8"), ("alt", "<f8"), ("drift", "<f8"), ("rms", "<f8"), ("pdop", "<f8")])
# aided acquisition (include/gpsacq.h, "Aided acquisition: predicted code phase and Doppler, windowed search")
AID_NO_FIX, AID_NO_EPH, AID_LOW, AID_OFF_GRID = 1, 2, 4, 8
AIDED_KEPT, AIDED_NO_AID, AIDED_SHORT, AIDED_FEW, AIDED_NO_POWER, AIDED_BELOW = 1, 2, 4, 8, 16, 32
AID_PARAMS_DTYPE = np.dtype([("elev_min_deg", "<f8"), ("reserved", "<f8")])
AID_DTYPE = np.dtype([("flags", "<i4"), ("ca_center", "<i4"), ("lo_center", "<i4"), ("reserved", "<i4"), ("tx_frac", "<f8"), ("doppler_hz", "<f8"),
                      ("elev_deg", "<f8")])
AIDED_PARAMS_DTYPE = np.dtype([("blocks", "<i4"), ("min_segments", "<i4"), ("code_half", "<i4"), ("dop_half", "<i4"), ("keep_snr", "<f8"),
                               ("ratio_min", "<f8")])
AIDED_DTYPE = np.dtype([("flags", "<i4"), ("segments", "<i4"), ("n_code", "<i4"), ("n_dop", "<i4"), ("best_h", "<i4"), ("best_d", "<i4"),
                        ("lo_shift", "<i4"), ("ca_shift", "<i4"), ("best", "<u8"), ("total", "<u8"), ("floor", "<u8"), ("ratio", "<f8")])
# coherent aided acquisition (include/gpsacq.h, "Coherent aided acquisition: 20 ms sums, bit edge and fine Doppler"); the flags are AIDED_*
AIDED_COH_MS = (1, 2, 4, 5, 10, 20)
AIDED_COH_PARAMS_DTYPE = np.dtype([("blocks", "<i4"), ("min_segments", "<i4"), ("code_half", "<i4"), ("dop_half", "<i4"), ("coh_ms", "<i4"),
                                   ("fine_half", "<i4"), ("fine_step", "<i4"), ("reserved", "<i4"), ("keep_snr", "<f8"), ("ratio_min", "<f8")])
AIDED_COH_DTYPE = np.dtype([("flags", "<i4"), ("segments", "<i4"), ("n_code", "<i4"), ("n_dop", "<i4"), ("n_fine", "<i4"), ("n_edge", "<i4"),
                            ("best_h", "<i4"), ("best_d", "<i4"), ("best_f", "<i4"), ("best_e", "<i4"), ("lo_shift", "<i4"), ("ca_shift", "<i4"),
                            ("best", "<u8"), ("noncoh", "<u8"), ("floor", "<u8"), ("ratio", "<f8"), ("doppler_hz", "<f8"), ("reserved", "<f8")])


# carrier-smoothed observables (include/gpsacq.h "Carrier-smoothed observables")
SMOOTH_RESET, SMOOTH_UNLOCKED, SMOOTH_FULL = 1, 2, 4
SMOOTH_PARAMS_DTYPE = np.dtype([("window", "<i4"), ("lock_epochs", "<i4"), ("lock_num", "<i4"), ("lock_den", "<i4"), ("jump", "<i8"),
                                ("invert", "<i4"), ("reserved", "<i4")])
SMOOTH_INFO_DTYPE = np.dtype([("window", "<i4"), ("flags", "<i4"), ("cmc", "<i8"), ("corr", "<i8")])
L1_HZ = 1575.42e6
C_MPS = 299792458.0

# signal quality per observation (include/gpsacq.h "Signal quality per observation")
QUALITY_NO_POWER, QUALITY_SATURATED, QUALITY_UNLOCKED, QUALITY_FULL, QUALITY_SHORT = 1, 2, 4, 8, 16
QUALITY_PARAMS_DTYPE = np.dtype([("epochs", "<i4"), ("min_epochs", "<i4"), ("lock_num", "<i4"), ("lock_den", "<i4"), ("require_lock", "<i4"),
                                 ("reserved", "<i4"), ("cn0_min_lin", "<f8"), ("cn0_ref_lin", "<f8"), ("cn0_cap_dbhz", "<f8")])
QUALITY_INFO_DTYPE = np.dtype([("epochs", "<i4"), ("flags", "<i4"), ("sig", "<u8"), ("noise", "<u8"), ("lin", "<f8"), ("cn0_dbhz", "<f8"),
                               ("weight", "<f8")])
# snapshot signal quality (include/gpsacq.h "Snapshot signal quality"): its info records are QUALITY_INFO_DTYPE with epochs = segments
QUALITY_NO_RECORD = 32
SNAP_QUALITY_PARAMS_DTYPE = np.dtype([("min_segments", "<i4"), ("reserved", "<i4"), ("cn0_min_lin", "<f8"), ("cn0_ref_lin", "<f8")])


class TrackParams(ctypes.Structure):
    _fields_ = [("lo_ki", ctypes.c_int32), ("lo_kp", ctypes.c_int32), ("ca_ki", ctypes.c_int32), ("ca_kp", ctypes.c_int32),
                ("fll_k", ctypes.c_int32), ("fll_epochs", ctypes.c_int32), ("aid_epoch", ctypes.c_int32), ("agc_period", ctypes.c_int32),
                ("agc_lo", ctypes.c_int64), ("agc_hi", ctypes.c_int64), ("lo_window", ctypes.c_int64), ("ca_window", ctypes.c_int64),
                ("min_epoch", ctypes.c_int32), ("max_epoch", ctypes.c_int32)]


EXPORTS = ["gpsacq_generate", "gpsacq_generate_device", "gpsacq_generate_range", "gpsacq_generate_range_device", "gpsacq_generate_sig", "gpsacq_sig_bytes", "gpsacq_handoff", "gpsacq_iq8_to_bits", "gpsacq_iq8_to_bits_device", "gpsacq_create", "gpsacq_destroy", "gpsacq_last_error", "gpsacq_get_info", "gpsacq_search",
           "gpsacq_search_device", "gpsacq_set_doppler_window", "gpsacq_set_cell_handout", "gpsacq_set_doppler_step", "gpsacq_set_noncoherent", "gpsacq_set_creep_compensation", "gpsacq_set_block_alignment", "gpsacq_aligned_stride", "gpsacq_synchronize", "gpsacq_last_timing", "gpsacq_timing_ago", "gpsacq_stream", "gpsacq_search_code",
           "gpsacq_sample_spectrum", "gpsacq_code_spectrum", "gpsacq_multi_create", "gpsacq_multi_destroy",
           "gpsacq_multi_set_doppler_step", "gpsacq_multi_get_info", "gpsacq_multi_search_grid", "gpsacq_multi_search_blocks",
           "gpsacq_pipe_buffer", "gpsacq_pipe_submit", "gpsacq_pipe_collect", "gpsacq_search_iq8", "gpsacq_search_iq8_device",
           "gpsacq_iq8_accumulate_sums", "gpsacq_handoff_step", "gpsacq_handoff_engine", "gpsacq_reserve", "gpsacq_multi_last_call_ms",
           "gpsacq_sig_tx_samples", "gpsacq_generate_sig_tx", "gpsacq_peak_keys_device", "gpsacq_cycle_stamp_device",
           "gpsacq_track_default_params", "gpsacq_track_start", "gpsacq_track", "gpsacq_track_device", "gpsacq_nav_bits",
           "gpsacq_nav_subframes", "gpsacq_generate_nav_range", "gpsacq_generate_nav_range_device",
           "gpsacq_track_iq8", "gpsacq_track_iq8_device", "gpsacq_track_iq8_last_ms", "gpsacq_track_start_iq8",
           "gpsacq_track_default_params_iq8", "gpsacq_iq8_accumulate_power", "gpsacq_generate_iq8_range",
           "gpsacq_generate_iq8_range_device",
           "gpsacq_ephemeris_load", "gpsacq_ephemeris_valid", "gpsacq_sat_states", "gpsacq_sat_states_device", "gpsacq_fix_batch",
           "gpsacq_fix_batch_device", "gpsacq_fix_last_ms",
           "gpsacq_time_tag_from_subframe", "gpsacq_observables", "gpsacq_observables_device", "gpsacq_fix_track_device",
           "gpsacq_observables_last_ms",
           "gpsacq_track_nominal_word_iq8", "gpsacq_rate_observables", "gpsacq_rate_observables_device", "gpsacq_sat_rates",
           "gpsacq_sat_rates_device", "gpsacq_vel_batch", "gpsacq_vel_batch_device", "gpsacq_pvt_track_device", "gpsacq_velocity_last_ms",
           "gpsacq_iono_load", "gpsacq_atm_default_params", "gpsacq_sat_views", "gpsacq_sat_views_device", "gpsacq_fix_atm_batch",
           "gpsacq_fix_atm_batch_device", "gpsacq_fix_atm_last_ms",
           "gpsacq_raim_default_params", "gpsacq_fix_raim_batch", "gpsacq_fix_raim_batch_device", "gpsacq_fix_raim_last_ms",
           "gpsacq_smooth_default_params", "gpsacq_smooth_observables", "gpsacq_smooth_observables_device", "gpsacq_fix_smooth_track_device",
           "gpsacq_smooth_last_ms",
           "gpsacq_quality_default_params", "gpsacq_quality_observables", "gpsacq_quality_observables_device",
           "gpsacq_fix_quality_track_device", "gpsacq_quality_last_ms",
           "gpsacq_coarse_default_params", "gpsacq_coarse_fix_batch", "gpsacq_coarse_fix_batch_device", "gpsacq_coarse_obs",
           "gpsacq_coarse_obs_device", "gpsacq_coarse_fix_peaks_device", "gpsacq_coarse_last_ms",
           "gpsacq_coarse_raim_batch", "gpsacq_coarse_raim_batch_device", "gpsacq_coarse_raim_last_ms",
           "gpsacq_refine_default_params", "gpsacq_refine", "gpsacq_refine_device", "gpsacq_coarse_obs_fine", "gpsacq_coarse_obs_fine_device",
           "gpsacq_coarse_fix_fine_device", "gpsacq_refine_last_ms",
           "gpsacq_snap_quality_default_params", "gpsacq_snap_quality", "gpsacq_snap_quality_device", "gpsacq_coarse_fix_quality_device",
           "gpsacq_snap_quality_last_ms",
           "gpsacq_dopfine_default_params", "gpsacq_doppler_fix_default_params", "gpsacq_fine_doppler", "gpsacq_fine_doppler_device",
           "gpsacq_rate_obs_fine", "gpsacq_rate_obs_fine_device", "gpsacq_doppler_fix_batch", "gpsacq_doppler_fix_batch_device",
           "gpsacq_cold_fix_device", "gpsacq_doppler_last_ms",
           "gpsacq_refine_iq8", "gpsacq_refine_iq8_device", "gpsacq_fine_doppler_iq8", "gpsacq_fine_doppler_iq8_device",
           "gpsacq_coarse_fix_fine_iq8_device", "gpsacq_cold_fix_iq8_device", "gpsacq_snapshot_iq8_last_ms",
           "gpsacq_aid_default_params", "gpsacq_aided_default_params", "gpsacq_aid_predict", "gpsacq_aid_predict_device", "gpsacq_aided_search",
           "gpsacq_aided_search_device", "gpsacq_aided_peaks_device", "gpsacq_aided_last_ms",
           "gpsacq_aided_coh_default_params", "gpsacq_aided_coh_table", "gpsacq_aided_coh_search", "gpsacq_aided_coh_search_device",
           "gpsacq_aid_instant", "gpsacq_aid_instant_device", "gpsacq_aided_coh_peaks_device", "gpsacq_aided_coh_last_ms",
           "gpsacq_aided_default_params_iq8", "gpsacq_aided_search_iq8", "gpsacq_aided_search_iq8_device", "gpsacq_aided_peaks_iq8_device",
           "gpsacq_aided_iq8_last_ms", "gpsacq_aided_coh_default_params_iq8", "gpsacq_aided_coh_search_iq8", "gpsacq_aided_coh_search_iq8_device",
           "gpsacq_aided_coh_peaks_iq8_device", "gpsacq_aided_coh_iq8_last_ms",
           "gpsacq_snap_quality_default_params_iq8", "gpsacq_snap_floor_iq8", "gpsacq_snap_floor_iq8_device", "gpsacq_snap_quality_iq8",
           "gpsacq_snap_quality_iq8_device", "gpsacq_coarse_fix_quality_iq8_device", "gpsacq_snap_quality_iq8_last_ms"]

_lib = None


def _preload_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, the same as
    /opt/rocm's).  Loaded first, torch's copy satisfies libgpsacq's NEEDED libamdhip64.so.7 by SONAME
    and the process has ONE HIP runtime (streams and events are then interchangeable, which
    bench.py relies on).  Loaded second, torch asks for the file name `libamdhip64.so`, gets its own
    second copy next to /opt/rocm's, and its CUDA initialisation finds no GPU (measured on the
    MI355X box, both orders).  So: if torch is installed and not yet imported, import it before the
    dlopen.  GPSACQ_NO_TORCH_PRELOAD=1 skips this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("GPSACQ_NO_TORCH_PRELOAD"):
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    except Exception:
        pass


def load_library(path=None):
    """dlopen libgpsacq.so and declare the prototypes.  Raises OSError if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `make lib` (hipcc --offload-arch=gfx950); "
                      "gpsacq has no CPU fallback")
    _preload_torch()
    lib = ctypes.CDLL(p)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.gpsacq_create.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(vp)]
    lib.gpsacq_create.restype = ctypes.c_int
    lib.gpsacq_destroy.argtypes = [vp]
    lib.gpsacq_destroy.restype = None
    lib.gpsacq_last_error.argtypes = []
    lib.gpsacq_last_error.restype = ctypes.c_char_p
    lib.gpsacq_get_info.argtypes = [vp, ctypes.POINTER(Info)]
    lib.gpsacq_get_info.restype = ctypes.c_int
    lib.gpsacq_search.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp]
    lib.gpsacq_search.restype = ctypes.c_int
    lib.gpsacq_search_device.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_search_device.restype = ctypes.c_int
    lib.gpsacq_set_doppler_window.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.gpsacq_set_doppler_window.restype = ctypes.c_int
    lib.gpsacq_set_cell_handout.argtypes = [vp, ctypes.c_int]
    lib.gpsacq_set_cell_handout.restype = ctypes.c_int
    lib.gpsacq_set_doppler_step.argtypes = [vp, ctypes.c_double]
    lib.gpsacq_set_doppler_step.restype = ctypes.c_int
    lib.gpsacq_set_noncoherent.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.gpsacq_set_noncoherent.restype = ctypes.c_int
    lib.gpsacq_aligned_stride.argtypes = [vp]
    lib.gpsacq_aligned_stride.restype = ctypes.c_int
    lib.gpsacq_synchronize.argtypes = [vp]
    lib.gpsacq_synchronize.restype = ctypes.c_int
    lib.gpsacq_last_timing.argtypes = [vp, ctypes.POINTER(Timing)]
    lib.gpsacq_last_timing.restype = ctypes.c_int
    lib.gpsacq_set_creep_compensation.argtypes = [vp, ctypes.c_int]
    lib.gpsacq_set_creep_compensation.restype = ctypes.c_int
    lib.gpsacq_set_block_alignment.argtypes = [vp, ctypes.c_int]
    lib.gpsacq_set_block_alignment.restype = ctypes.c_int
    lib.gpsacq_timing_ago.argtypes = [vp, ctypes.c_int, ctypes.POINTER(Timing)]
    lib.gpsacq_timing_ago.restype = ctypes.c_int
    lib.gpsacq_stream.argtypes = [vp]
    lib.gpsacq_stream.restype = ctypes.c_void_p
    lib.gpsacq_iq8_to_bits.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, vp]
    lib.gpsacq_iq8_to_bits.restype = ctypes.c_int
    lib.gpsacq_iq8_to_bits_device.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, vp, ctypes.c_int]
    lib.gpsacq_iq8_to_bits_device.restype = ctypes.c_int
    lib.gpsacq_generate.argtypes = [vp, vp, sz, ctypes.POINTER(Sat), ctypes.c_int, ctypes.c_float, ctypes.c_uint64]
    lib.gpsacq_generate.restype = ctypes.c_int
    lib.gpsacq_generate_device.argtypes = [vp, vp, sz, ctypes.POINTER(Sat), ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_int]
    lib.gpsacq_generate_device.restype = ctypes.c_int
    lib.gpsacq_generate_range.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.POINTER(Sat), ctypes.c_int, ctypes.c_float, ctypes.c_uint64]
    lib.gpsacq_generate_range.restype = ctypes.c_int
    lib.gpsacq_generate_range_device.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.POINTER(Sat), ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_int]
    lib.gpsacq_generate_range_device.restype = ctypes.c_int
    lib.gpsacq_sig_bytes.argtypes = [ctypes.c_int]
    lib.gpsacq_sig_bytes.restype = ctypes.c_size_t
    lib.gpsacq_generate_sig.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, vp, sz]
    lib.gpsacq_generate_sig.restype = ctypes.c_int
    lib.gpsacq_handoff.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(Handoff)]
    lib.gpsacq_handoff.restype = ctypes.c_int
    lib.gpsacq_search_code.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.gpsacq_search_code.restype = ctypes.c_int
    lib.gpsacq_sample_spectrum.argtypes = [vp, vp, vp]
    lib.gpsacq_sample_spectrum.restype = ctypes.c_int
    lib.gpsacq_code_spectrum.argtypes = [vp, ctypes.c_int, vp]
    lib.gpsacq_code_spectrum.restype = ctypes.c_int
    lib.gpsacq_multi_create.argtypes = [ctypes.POINTER(Params), vp, ctypes.c_int, ctypes.POINTER(vp)]
    lib.gpsacq_multi_create.restype = ctypes.c_int
    lib.gpsacq_multi_destroy.argtypes = [vp]
    lib.gpsacq_multi_destroy.restype = None
    lib.gpsacq_multi_set_doppler_step.argtypes = [vp, ctypes.c_double]
    lib.gpsacq_multi_set_doppler_step.restype = ctypes.c_int
    lib.gpsacq_multi_get_info.argtypes = [vp, ctypes.POINTER(Info), ctypes.POINTER(ctypes.c_int32)]
    lib.gpsacq_multi_get_info.restype = ctypes.c_int
    lib.gpsacq_multi_search_grid.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    lib.gpsacq_multi_search_grid.restype = ctypes.c_int
    lib.gpsacq_multi_search_blocks.argtypes = [vp, vp, sz, sz, vp, vp]
    lib.gpsacq_multi_search_blocks.restype = ctypes.c_int
    lib.gpsacq_pipe_buffer.argtypes = [vp, ctypes.c_int, sz]
    lib.gpsacq_pipe_buffer.restype = ctypes.c_void_p
    lib.gpsacq_pipe_submit.argtypes = [vp, ctypes.c_int, sz, sz, ctypes.POINTER(Iq8Input)]
    lib.gpsacq_pipe_submit.restype = ctypes.c_int
    lib.gpsacq_pipe_collect.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.gpsacq_pipe_collect.restype = ctypes.c_int
    lib.gpsacq_search_iq8.argtypes = [vp, ctypes.POINTER(Iq8Input), vp, sz, sz, vp, sz, vp, vp]
    lib.gpsacq_search_iq8.restype = ctypes.c_int
    lib.gpsacq_search_iq8_device.argtypes = [vp, ctypes.POINTER(Iq8Input), vp, sz, sz, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_search_iq8_device.restype = ctypes.c_int
    lib.gpsacq_iq8_accumulate_sums.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.gpsacq_iq8_accumulate_sums.restype = ctypes.c_int
    lib.gpsacq_handoff_step.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(Handoff)]
    lib.gpsacq_handoff_step.restype = ctypes.c_int
    lib.gpsacq_handoff_engine.argtypes = [vp, vp, ctypes.c_double, ctypes.POINTER(Handoff)]
    lib.gpsacq_handoff_engine.restype = ctypes.c_int
    lib.gpsacq_reserve.argtypes = [vp, sz]
    lib.gpsacq_reserve.restype = ctypes.c_int
    lib.gpsacq_sig_tx_samples.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.gpsacq_sig_tx_samples.restype = ctypes.c_uint64
    lib.gpsacq_generate_sig_tx.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, sz, vp]
    lib.gpsacq_generate_sig_tx.restype = ctypes.c_int
    lib.gpsacq_peak_keys_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, ctypes.c_int]
    lib.gpsacq_peak_keys_device.restype = ctypes.c_int
    lib.gpsacq_cycle_stamp_device.argtypes = [vp, vp, ctypes.c_int]
    lib.gpsacq_cycle_stamp_device.restype = ctypes.c_int
    lib.gpsacq_multi_last_call_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
    lib.gpsacq_multi_last_call_ms.restype = ctypes.c_int
    lib.gpsacq_track_default_params.argtypes = [vp, ctypes.POINTER(TrackParams)]
    lib.gpsacq_track_default_params.restype = ctypes.c_int
    lib.gpsacq_track_start.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint64, ctypes.POINTER(TrackParams), vp]
    lib.gpsacq_track_start.restype = ctypes.c_int
    lib.gpsacq_track.argtypes = [vp, vp, sz, ctypes.c_uint64, vp, ctypes.c_int, ctypes.POINTER(TrackParams), vp, vp, ctypes.c_int, vp]
    lib.gpsacq_track.restype = ctypes.c_int
    lib.gpsacq_track_device.argtypes = [vp, vp, sz, ctypes.c_uint64, vp, ctypes.c_int, ctypes.POINTER(TrackParams), vp, vp, ctypes.c_int, vp]
    lib.gpsacq_track_device.restype = ctypes.c_int
    lib.gpsacq_nav_bits.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.gpsacq_nav_bits.restype = ctypes.c_int
    lib.gpsacq_nav_subframes.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.gpsacq_nav_subframes.restype = ctypes.c_int
    lib.gpsacq_generate_nav_range.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.POINTER(Sat), ctypes.c_int, vp, ctypes.c_int, ctypes.c_float, ctypes.c_uint64]
    lib.gpsacq_generate_nav_range.restype = ctypes.c_int
    lib.gpsacq_generate_nav_range_device.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.POINTER(Sat), ctypes.c_int, vp, ctypes.c_int, ctypes.c_float,
                                                     ctypes.c_uint64, ctypes.c_int]
    lib.gpsacq_generate_nav_range_device.restype = ctypes.c_int
    iqp = ctypes.POINTER(Iq8Input)
    lib.gpsacq_track_iq8.argtypes = [vp, iqp, vp, sz, ctypes.c_uint64, vp, ctypes.c_int, ctypes.POINTER(TrackParams), vp, vp, ctypes.c_int, vp]
    lib.gpsacq_track_iq8.restype = ctypes.c_int
    lib.gpsacq_track_iq8_device.argtypes = [vp, iqp, vp, sz, ctypes.c_uint64, vp, ctypes.c_int, ctypes.POINTER(TrackParams), vp, vp, ctypes.c_int, vp]
    lib.gpsacq_track_iq8_device.restype = ctypes.c_int
    lib.gpsacq_track_iq8_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.gpsacq_track_iq8_last_ms.restype = ctypes.c_int
    lib.gpsacq_track_start_iq8.argtypes = [vp, iqp, ctypes.c_int, vp, ctypes.c_uint64, ctypes.POINTER(TrackParams), vp]
    lib.gpsacq_track_start_iq8.restype = ctypes.c_int
    lib.gpsacq_track_default_params_iq8.argtypes = [vp, ctypes.c_double, ctypes.POINTER(TrackParams)]
    lib.gpsacq_track_default_params_iq8.restype = ctypes.c_int
    lib.gpsacq_iq8_accumulate_power.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    lib.gpsacq_iq8_accumulate_power.restype = ctypes.c_int
    lib.gpsacq_generate_iq8_range.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.POINTER(Sat),
                                              ctypes.c_int, vp, ctypes.c_int, ctypes.c_float, ctypes.c_uint64]
    lib.gpsacq_generate_iq8_range.restype = ctypes.c_int
    lib.gpsacq_generate_iq8_range_device.argtypes = [vp, vp, sz, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.POINTER(Sat),
                                                     ctypes.c_int, vp, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_int]
    lib.gpsacq_generate_iq8_range_device.restype = ctypes.c_int
    lib.gpsacq_ephemeris_load.argtypes = [vp, vp, ctypes.c_int]
    lib.gpsacq_ephemeris_load.restype = ctypes.c_int
    lib.gpsacq_ephemeris_valid.argtypes = [vp]
    lib.gpsacq_ephemeris_valid.restype = ctypes.c_int
    lib.gpsacq_sat_states.argtypes = [vp, vp, ctypes.c_int, vp, sz, vp]
    lib.gpsacq_sat_states.restype = ctypes.c_int
    lib.gpsacq_sat_states_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, vp, ctypes.c_int]
    lib.gpsacq_sat_states_device.restype = ctypes.c_int
    lib.gpsacq_fix_batch.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp]
    lib.gpsacq_fix_batch.restype = ctypes.c_int
    lib.gpsacq_fix_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp, ctypes.c_int]
    lib.gpsacq_fix_batch_device.restype = ctypes.c_int
    lib.gpsacq_fix_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.gpsacq_fix_last_ms.restype = ctypes.c_int
    lib.gpsacq_time_tag_from_subframe.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.gpsacq_time_tag_from_subframe.restype = ctypes.c_int
    obs_args = [vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, sz, vp]
    lib.gpsacq_observables.argtypes = obs_args
    lib.gpsacq_observables.restype = ctypes.c_int
    lib.gpsacq_observables_device.argtypes = obs_args + [ctypes.c_int]
    lib.gpsacq_observables_device.restype = ctypes.c_int
    lib.gpsacq_fix_track_device.argtypes = [vp, vp, ctypes.c_int] + obs_args[1:] + [vp, ctypes.c_int]
    lib.gpsacq_fix_track_device.restype = ctypes.c_int
    lib.gpsacq_observables_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.gpsacq_observables_last_ms.restype = ctypes.c_int
    u64 = ctypes.c_uint64
    lib.gpsacq_track_nominal_word_iq8.argtypes = [vp, ctypes.POINTER(Iq8Input), ctypes.POINTER(ctypes.c_uint32)]
    lib.gpsacq_track_nominal_word_iq8.restype = ctypes.c_int
    rate_args = [vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, u64, u64, sz, u64, vp]
    lib.gpsacq_rate_observables.argtypes = rate_args
    lib.gpsacq_rate_observables.restype = ctypes.c_int
    lib.gpsacq_rate_observables_device.argtypes = rate_args + [ctypes.c_int]
    lib.gpsacq_rate_observables_device.restype = ctypes.c_int
    lib.gpsacq_sat_rates.argtypes = [vp, vp, ctypes.c_int, vp, sz, vp]
    lib.gpsacq_sat_rates.restype = ctypes.c_int
    lib.gpsacq_sat_rates_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, vp, ctypes.c_int]
    lib.gpsacq_sat_rates_device.restype = ctypes.c_int
    lib.gpsacq_vel_batch.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, sz, ctypes.c_int, vp]
    lib.gpsacq_vel_batch.restype = ctypes.c_int
    lib.gpsacq_vel_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, sz, ctypes.c_int, vp, ctypes.c_int]
    lib.gpsacq_vel_batch_device.restype = ctypes.c_int
    lib.gpsacq_pvt_track_device.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, u64, u64, sz, u64, vp, vp, vp, vp,
                                            ctypes.c_int]
    lib.gpsacq_pvt_track_device.restype = ctypes.c_int
    lib.gpsacq_velocity_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 4
    lib.gpsacq_velocity_last_ms.restype = ctypes.c_int
    lib.gpsacq_iono_load.argtypes = [vp, vp, ctypes.c_int]
    lib.gpsacq_iono_load.restype = ctypes.c_int
    lib.gpsacq_atm_default_params.argtypes = [vp, vp]
    lib.gpsacq_atm_default_params.restype = ctypes.c_int
    lib.gpsacq_sat_views.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp]
    lib.gpsacq_sat_views.restype = ctypes.c_int
    lib.gpsacq_sat_views_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, ctypes.c_int]
    lib.gpsacq_sat_views_device.restype = ctypes.c_int
    lib.gpsacq_fix_atm_batch.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp, vp, vp, vp]
    lib.gpsacq_fix_atm_batch.restype = ctypes.c_int
    lib.gpsacq_fix_atm_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_fix_atm_batch_device.restype = ctypes.c_int
    lib.gpsacq_fix_atm_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_fix_atm_last_ms.restype = ctypes.c_int
    lib.gpsacq_raim_default_params.argtypes = [ctypes.c_double, ctypes.c_double, vp]
    lib.gpsacq_raim_default_params.restype = ctypes.c_int
    lib.gpsacq_fix_raim_batch.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.gpsacq_fix_raim_batch.restype = ctypes.c_int
    lib.gpsacq_fix_raim_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_fix_raim_batch_device.restype = ctypes.c_int
    lib.gpsacq_fix_raim_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_fix_raim_last_ms.restype = ctypes.c_int
    lib.gpsacq_smooth_default_params.argtypes = [vp]
    lib.gpsacq_smooth_default_params.restype = ctypes.c_int
    smooth_args = [vp, vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, u64, u64, sz, vp, vp, vp]
    lib.gpsacq_smooth_observables.argtypes = smooth_args
    lib.gpsacq_smooth_observables.restype = ctypes.c_int
    lib.gpsacq_smooth_observables_device.argtypes = smooth_args + [ctypes.c_int]
    lib.gpsacq_smooth_observables_device.restype = ctypes.c_int
    lib.gpsacq_fix_smooth_track_device.argtypes = [vp, vp, ctypes.c_int] + smooth_args[1:] + [vp, ctypes.c_int]
    lib.gpsacq_fix_smooth_track_device.restype = ctypes.c_int
    lib.gpsacq_smooth_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 4
    lib.gpsacq_smooth_last_ms.restype = ctypes.c_int
    lib.gpsacq_quality_default_params.argtypes = [vp]
    lib.gpsacq_quality_default_params.restype = ctypes.c_int
    quality_args = [vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, u64, u64, sz, vp, vp, vp]
    lib.gpsacq_quality_observables.argtypes = quality_args
    lib.gpsacq_quality_observables.restype = ctypes.c_int
    lib.gpsacq_quality_observables_device.argtypes = quality_args + [ctypes.c_int]
    lib.gpsacq_quality_observables_device.restype = ctypes.c_int
    lib.gpsacq_fix_quality_track_device.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, u64, u64, sz, vp, vp, vp, vp,
                                                    vp, ctypes.c_int]
    lib.gpsacq_fix_quality_track_device.restype = ctypes.c_int
    lib.gpsacq_quality_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_quality_last_ms.restype = ctypes.c_int
    lib.gpsacq_coarse_default_params.argtypes = [vp]
    lib.gpsacq_coarse_default_params.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_batch.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp]
    lib.gpsacq_coarse_fix_batch.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_coarse_fix_batch_device.restype = ctypes.c_int
    lib.gpsacq_coarse_obs.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_double, vp]
    lib.gpsacq_coarse_obs.restype = ctypes.c_int
    lib.gpsacq_coarse_obs_device.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_double, vp, ctypes.c_int]
    lib.gpsacq_coarse_obs_device.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_peaks_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, ctypes.c_int, ctypes.c_double, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_coarse_fix_peaks_device.restype = ctypes.c_int
    lib.gpsacq_coarse_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_coarse_last_ms.restype = ctypes.c_int
    lib.gpsacq_coarse_raim_batch.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    lib.gpsacq_coarse_raim_batch.restype = ctypes.c_int
    lib.gpsacq_coarse_raim_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_coarse_raim_batch_device.restype = ctypes.c_int
    lib.gpsacq_coarse_raim_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_coarse_raim_last_ms.restype = ctypes.c_int
    lib.gpsacq_refine_default_params.argtypes = [vp]
    lib.gpsacq_refine_default_params.restype = ctypes.c_int
    lib.gpsacq_refine.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, vp]
    lib.gpsacq_refine.restype = ctypes.c_int
    lib.gpsacq_refine_device.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_refine_device.restype = ctypes.c_int
    lib.gpsacq_coarse_obs_fine.argtypes = [vp, vp, vp, sz, ctypes.c_int, ctypes.c_double, vp]
    lib.gpsacq_coarse_obs_fine.restype = ctypes.c_int
    lib.gpsacq_coarse_obs_fine_device.argtypes = [vp, vp, vp, sz, ctypes.c_int, ctypes.c_double, vp, ctypes.c_int]
    lib.gpsacq_coarse_obs_fine_device.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_fine_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_coarse_fix_fine_device.restype = ctypes.c_int
    lib.gpsacq_refine_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_refine_last_ms.restype = ctypes.c_int
    lib.gpsacq_snap_quality_default_params.argtypes = [vp]
    lib.gpsacq_snap_quality_default_params.restype = ctypes.c_int
    lib.gpsacq_snap_quality.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, vp]
    lib.gpsacq_snap_quality.restype = ctypes.c_int
    lib.gpsacq_snap_quality_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_snap_quality_device.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_quality_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                     ctypes.c_int]
    lib.gpsacq_coarse_fix_quality_device.restype = ctypes.c_int
    lib.gpsacq_snap_quality_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.gpsacq_snap_quality_last_ms.restype = ctypes.c_int
    lib.gpsacq_dopfine_default_params.argtypes = [vp]
    lib.gpsacq_dopfine_default_params.restype = ctypes.c_int
    lib.gpsacq_doppler_fix_default_params.argtypes = [vp]
    lib.gpsacq_doppler_fix_default_params.restype = ctypes.c_int
    lib.gpsacq_fine_doppler.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, vp]
    lib.gpsacq_fine_doppler.restype = ctypes.c_int
    lib.gpsacq_fine_doppler_device.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_fine_doppler_device.restype = ctypes.c_int
    lib.gpsacq_rate_obs_fine.argtypes = [vp, vp, vp, sz, ctypes.c_int, ctypes.c_double, vp]
    lib.gpsacq_rate_obs_fine.restype = ctypes.c_int
    lib.gpsacq_rate_obs_fine_device.argtypes = [vp, vp, vp, sz, ctypes.c_int, ctypes.c_double, vp, ctypes.c_int]
    lib.gpsacq_rate_obs_fine_device.restype = ctypes.c_int
    lib.gpsacq_doppler_fix_batch.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, sz, ctypes.c_int, vp, vp, vp]
    lib.gpsacq_doppler_fix_batch.restype = ctypes.c_int
    lib.gpsacq_doppler_fix_batch_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, sz, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_doppler_fix_batch_device.restype = ctypes.c_int
    lib.gpsacq_cold_fix_device.argtypes = [vp, vp, ctypes.c_int, vp, sz, sz, vp, vp, vp, sz, ctypes.c_int] + [vp] * 13 + [ctypes.c_int]
    lib.gpsacq_cold_fix_device.restype = ctypes.c_int
    lib.gpsacq_refine_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp, vp]
    lib.gpsacq_refine_iq8.restype = ctypes.c_int
    lib.gpsacq_refine_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_refine_iq8_device.restype = ctypes.c_int
    lib.gpsacq_fine_doppler_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp, vp]
    lib.gpsacq_fine_doppler_iq8.restype = ctypes.c_int
    lib.gpsacq_fine_doppler_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp, vp, ctypes.c_int]
    lib.gpsacq_fine_doppler_iq8_device.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_fine_iq8_device.argtypes = [vp, vp, ctypes.c_int, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int] + [vp] * 8 + [ctypes.c_int]
    lib.gpsacq_coarse_fix_fine_iq8_device.restype = ctypes.c_int
    lib.gpsacq_cold_fix_iq8_device.argtypes = [vp, vp, ctypes.c_int, iqp, vp, sz, sz, vp, vp, vp, sz, ctypes.c_int] + [vp] * 13 + [ctypes.c_int]
    lib.gpsacq_cold_fix_iq8_device.restype = ctypes.c_int
    lib.gpsacq_snapshot_iq8_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_snapshot_iq8_last_ms.restype = ctypes.c_int
    lib.gpsacq_doppler_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_doppler_last_ms.restype = ctypes.c_int
    lib.gpsacq_aid_default_params.argtypes = [vp]
    lib.gpsacq_aid_default_params.restype = ctypes.c_int
    lib.gpsacq_aided_default_params.argtypes = [vp]
    lib.gpsacq_aided_default_params.restype = ctypes.c_int
    lib.gpsacq_aid_predict.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp]
    lib.gpsacq_aid_predict.restype = ctypes.c_int
    lib.gpsacq_aid_predict_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, sz, ctypes.c_int, vp, vp, ctypes.c_int]
    lib.gpsacq_aid_predict_device.restype = ctypes.c_int
    lib.gpsacq_aided_search.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.gpsacq_aided_search.restype = ctypes.c_int
    lib.gpsacq_aided_search_device.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_search_device.restype = ctypes.c_int
    lib.gpsacq_aided_peaks_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_peaks_device.restype = ctypes.c_int
    lib.gpsacq_aided_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_aided_last_ms.restype = ctypes.c_int
    lib.gpsacq_aided_coh_default_params.argtypes = [vp]
    lib.gpsacq_aided_coh_default_params.restype = ctypes.c_int
    lib.gpsacq_aided_coh_table.argtypes = [vp]
    lib.gpsacq_aided_coh_table.restype = ctypes.c_int
    lib.gpsacq_aided_coh_search.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.gpsacq_aided_coh_search.restype = ctypes.c_int
    lib.gpsacq_aided_coh_search_device.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_coh_search_device.restype = ctypes.c_int
    lib.gpsacq_aid_instant.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.gpsacq_aid_instant.restype = ctypes.c_int
    lib.gpsacq_aid_instant_device.argtypes = [vp, vp, vp, vp, sz, vp, ctypes.c_int]
    lib.gpsacq_aid_instant_device.restype = ctypes.c_int
    lib.gpsacq_aided_coh_peaks_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp,
                                                  ctypes.c_int]
    lib.gpsacq_aided_coh_peaks_device.restype = ctypes.c_int
    lib.gpsacq_aided_coh_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_aided_coh_last_ms.restype = ctypes.c_int
    lib.gpsacq_aided_default_params_iq8.argtypes = [vp]
    lib.gpsacq_aided_default_params_iq8.restype = ctypes.c_int
    lib.gpsacq_aided_search_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.gpsacq_aided_search_iq8.restype = ctypes.c_int
    lib.gpsacq_aided_search_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_search_iq8_device.restype = ctypes.c_int
    lib.gpsacq_aided_peaks_iq8_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_peaks_iq8_device.restype = ctypes.c_int
    lib.gpsacq_aided_iq8_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    lib.gpsacq_aided_iq8_last_ms.restype = ctypes.c_int
    lib.gpsacq_aided_coh_default_params_iq8.argtypes = [vp]
    lib.gpsacq_aided_coh_default_params_iq8.restype = ctypes.c_int
    lib.gpsacq_aided_coh_search_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.gpsacq_aided_coh_search_iq8.restype = ctypes.c_int
    lib.gpsacq_aided_coh_search_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_aided_coh_search_iq8_device.restype = ctypes.c_int
    lib.gpsacq_aided_coh_peaks_iq8_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp,
                                                      ctypes.c_int]
    lib.gpsacq_aided_coh_peaks_iq8_device.restype = ctypes.c_int
    lib.gpsacq_aided_coh_iq8_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 4
    lib.gpsacq_aided_coh_iq8_last_ms.restype = ctypes.c_int
    lib.gpsacq_snap_quality_default_params_iq8.argtypes = [vp]
    lib.gpsacq_snap_quality_default_params_iq8.restype = ctypes.c_int
    lib.gpsacq_snap_floor_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp]
    lib.gpsacq_snap_floor_iq8.restype = ctypes.c_int
    lib.gpsacq_snap_floor_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, vp, ctypes.c_int]
    lib.gpsacq_snap_floor_iq8_device.restype = ctypes.c_int
    lib.gpsacq_snap_quality_iq8.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp]
    lib.gpsacq_snap_quality_iq8.restype = ctypes.c_int
    lib.gpsacq_snap_quality_iq8_device.argtypes = [vp, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int]
    lib.gpsacq_snap_quality_iq8_device.restype = ctypes.c_int
    lib.gpsacq_coarse_fix_quality_iq8_device.argtypes = [vp, vp, ctypes.c_int, iqp, vp, sz, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                         vp, vp, ctypes.c_int]
    lib.gpsacq_coarse_fix_quality_iq8_device.restype = ctypes.c_int
    lib.gpsacq_snap_quality_iq8_last_ms.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    lib.gpsacq_snap_quality_iq8_last_ms.restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


class GpsAcqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpsacq error {code}: {msg}")
        self.code = code


def _check(lib, rc):
    if rc != 0:
        raise GpsAcqError(rc, lib.gpsacq_last_error().decode(errors="replace"))


def handoff(peak, fc, fs, secs_since_sample=0.0, step_hz=0.0):
    """CHANNEL::Start()'s NCO set-up from a search hit (c/channel.cpp:134-163).  peak: a PEAK_DTYPE record.
    step_hz: what one unit of lo_shift is worth -- 0 for the reference grid (FFT bins of fs/40000), else the engine's
    doppler_step_hz after set_doppler_step() (Engine.handoff() passes it by itself)."""
    lib = load_library()
    pk = np.zeros(1, dtype=PEAK_DTYPE)
    pk[0] = peak
    h = Handoff()
    _check(lib, lib.gpsacq_handoff_step(pk.ctypes.data_as(ctypes.c_void_p), float(fc), float(fs), float(step_hz), float(secs_since_sample), ctypes.byref(h)))
    return {k: getattr(h, k) for k, _ in Handoff._fields_}


def nav_bits(ip, first_epoch=0, sync_epochs=0):
    """gpsacq_nav_bits: bit sync on the prompt I arm, then one NAV bit (0/1, 1 = negative I) per whole 20-epoch window.
    Returns (bits uint8 array, epoch where bit 0 starts); (empty array, -1) when there is no bit sync."""
    lib = load_library()
    a = np.ascontiguousarray(np.asarray(ip, dtype=np.int32))
    out = np.zeros(a.size // 20 + 1, dtype=np.uint8)
    e0, nb = ctypes.c_int(), ctypes.c_int()
    rc = lib.gpsacq_nav_bits(a.ctypes.data_as(ctypes.c_void_p), int(a.size), int(first_epoch), int(sync_epochs),
                             out.ctypes.data_as(ctypes.c_void_p), int(out.size), ctypes.byref(e0), ctypes.byref(nb))
    if rc != 0:
        return np.zeros(0, dtype=np.uint8), -1
    return out[:nb.value].copy(), e0.value


def nav_subframes(bits):
    """gpsacq_nav_subframes: (SUBFRAME_DTYPE array, parity failures) of a 0/1 bit stream."""
    lib = load_library()
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8))
    out = np.zeros(b.size // 300 + 1, dtype=SUBFRAME_DTYPE)
    n, nf = ctypes.c_int(), ctypes.c_int()
    _check(lib, lib.gpsacq_nav_subframes(b.ctypes.data_as(ctypes.c_void_p), int(b.size), out.ctypes.data_as(ctypes.c_void_p), int(out.size),
                                         ctypes.byref(n), ctypes.byref(nf)))
    return out[:n.value].copy(), nf.value


def ephemeris(subframes, prn, eph=None):
    """gpsacq_ephemeris_load: subframes 1-3 of a SUBFRAME_DTYPE array (nav_subframes) folded, in order, into an EPHEMERIS_DTYPE
    record of shape (1,) for PRN `prn` -- a fresh one, or a copy of `eph` to carry on from."""
    lib = load_library()
    sf = np.ascontiguousarray(np.asarray(subframes, dtype=SUBFRAME_DTYPE).ravel())
    out = np.zeros(1, dtype=EPHEMERIS_DTYPE) if eph is None else np.array(eph, dtype=EPHEMERIS_DTYPE).reshape(1).copy()
    out["prn"] = int(prn)
    _check(lib, lib.gpsacq_ephemeris_load(out.ctypes.data_as(ctypes.c_void_p), sf.ctypes.data_as(ctypes.c_void_p) if sf.size else None,
                                          int(sf.size)))
    return out


def ephemeris_valid(eph):
    """gpsacq_ephemeris_valid of one EPHEMERIS_DTYPE record: subframes 1-3 loaded and IODC's low byte == both IODEs != 0."""
    rec = np.array(eph, dtype=EPHEMERIS_DTYPE).reshape(1).copy()
    return bool(load_library().gpsacq_ephemeris_valid(rec.ctypes.data_as(ctypes.c_void_p)))


def iono(subframes, io=None):
    """gpsacq_iono_load: every page 18 (subframe 4, SV/page ID 56) of a SUBFRAME_DTYPE array folded, in order, into an IONO_DTYPE
    record of shape (1,) -- a fresh one (valid == 0 until a page 18 is seen), or a copy of `io` to carry on from."""
    lib = load_library()
    sf = np.ascontiguousarray(np.asarray(subframes, dtype=SUBFRAME_DTYPE).ravel())
    out = np.zeros(1, dtype=IONO_DTYPE) if io is None else np.array(io, dtype=IONO_DTYPE).reshape(1).copy()
    _check(lib, lib.gpsacq_iono_load(out.ctypes.data_as(ctypes.c_void_p), sf.ctypes.data_as(ctypes.c_void_p) if sf.size else None, int(sf.size)))
    return out


def atm_params(iono=None, elev_mask=None, flags=None):
    """gpsacq_atm_default_params: an ATM_PARAMS_DTYPE record of shape (1,) -- the coefficients of `iono` (an IONO_DTYPE record;
    zeros when None or not valid), a 5-degree mask, ionosphere and troposphere on -- with elev_mask (radians) and flags replaced
    where given.  The entry points that take it check it."""
    lib = load_library()
    io = None if iono is None else np.array(iono, dtype=IONO_DTYPE).reshape(1).copy()
    out = np.zeros(1, dtype=ATM_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_atm_default_params(None if io is None else io.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)))
    if elev_mask is not None:
        out["elev_mask"] = float(elev_mask)
    if flags is not None:
        out["flags"] = int(flags)
    return out


def raim_params(sigma_m, p_fa=1e-3):
    """gpsacq_raim_default_params: a RAIM_PARAMS_DTYPE record of shape (1,) -- sigma_m the standard deviation (metres) of a
    pseudorange of weight 1, threshold[d - 1] the chi-square quantile with upper tail p_fa at d degrees of freedom, exclude = 1.
    The caller may overwrite thresholds and exclude; the entry points that take the record check it."""
    lib = load_library()
    out = np.zeros(1, dtype=RAIM_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_raim_default_params(float(sigma_m), float(p_fa), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def coarse_params(rms_max_m=None):
    """gpsacq_coarse_default_params: a COARSE_PARAMS_DTYPE record of shape (1,) -- rms_max_m one C/A chip, 293.05 m -- with
    rms_max_m replaced where given.  The entry points that take it check it."""
    lib = load_library()
    out = np.zeros(1, dtype=COARSE_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_coarse_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    if rms_max_m is not None:
        out["rms_max_m"] = float(rms_max_m)
    return out


def refine_params(**overrides):
    """gpsacq_refine_default_params: a REFINE_PARAMS_DTYPE record of shape (1,) -- a window of 16 blocks, min_segments 1, early
    and late a quarter chip from the prompt, snr_min the search threshold -- with the named fields replaced.  Values outside the
    bounds of include/gpsacq.h ("Fine code phases", INPUTS) raise ValueError here; the entry points check them again."""
    lib = load_library()
    out = np.zeros(1, dtype=REFINE_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_refine_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    for k, v in overrides.items():
        if k not in REFINE_PARAMS_DTYPE.names:
            raise TypeError("refine_params: no field %r" % k)
        if k in ("blocks", "min_segments") and int(v) != v:
            raise ValueError("refine_params: %s = %r is no whole number" % (k, v))
        out[k] = v
    r = out[0]
    if not 1 <= r["blocks"] <= 64:
        raise ValueError("refine_params: blocks %d outside 1 .. 64" % r["blocks"])
    if r["min_segments"] < 1:
        raise ValueError("refine_params: min_segments %d (must be >= 1)" % r["min_segments"])
    if not 1.0 / 64 <= r["half_spacing_chips"] <= 0.5:
        raise ValueError("refine_params: half_spacing_chips %g outside [1/64, 0.5]" % r["half_spacing_chips"])
    if not np.isfinite(r["snr_min"]):
        raise ValueError("refine_params: snr_min %g (must be finite)" % r["snr_min"])
    return out


def dopfine_params(**overrides):
    """gpsacq_dopfine_default_params: a DOPFINE_PARAMS_DTYPE record of shape (1,) -- a window of 16 blocks, min_segments 2, snr_min
    the search threshold, coherence_min 0 (no gate) -- with the named fields replaced.  Values outside the bounds of
    include/gpsacq.h ("Cold snapshot fixes", 1.) raise ValueError here; the entry points check them again."""
    lib = load_library()
    out = np.zeros(1, dtype=DOPFINE_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_dopfine_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    for k, v in overrides.items():
        if k not in DOPFINE_PARAMS_DTYPE.names:
            raise TypeError("dopfine_params: no field %r" % k)
        if k in ("blocks", "min_segments") and int(v) != v:
            raise ValueError("dopfine_params: %s = %r is no whole number" % (k, v))
        out[k] = v
    r = out[0]
    if not 1 <= r["blocks"] <= 64:
        raise ValueError("dopfine_params: blocks %d outside 1 .. 64" % r["blocks"])
    if r["min_segments"] < 2:
        raise ValueError("dopfine_params: min_segments %d (must be >= 2)" % r["min_segments"])
    if not np.isfinite(r["snr_min"]):
        raise ValueError("dopfine_params: snr_min %g (must be finite)" % r["snr_min"])
    if not (np.isfinite(r["coherence_min"]) and r["coherence_min"] >= 0):
        raise ValueError("dopfine_params: coherence_min %g (must be finite and >= 0)" % r["coherence_min"])
    return out


def doppler_fix_params(rms_max_mps=None):
    """gpsacq_doppler_fix_default_params: a DOPPLER_FIX_PARAMS_DTYPE record of shape (1,) -- rms_max_mps 3.0 m/s -- with rms_max_mps
    replaced where given.  The entry points that take it check it."""
    lib = load_library()
    out = np.zeros(1, dtype=DOPPLER_FIX_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_doppler_fix_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    if rms_max_mps is not None:
        out["rms_max_mps"] = float(rms_max_mps)
    return out


def aid_params(elev_min_deg=None):
    """gpsacq_aid_default_params: an AID_PARAMS_DTYPE record of shape (1,) -- elev_min_deg 5.0 -- with elev_min_deg replaced where
    given (finite, -90 .. 90: ValueError otherwise; the entry points check it again)."""
    lib = load_library()
    out = np.zeros(1, dtype=AID_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_aid_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    if elev_min_deg is not None:
        if not -90.0 <= float(elev_min_deg) <= 90.0:
            raise ValueError("aid_params: elev_min_deg %g outside [-90, 90]" % elev_min_deg)
        out["elev_min_deg"] = float(elev_min_deg)
    return out


def aided_params(**overrides):
    """gpsacq_aided_default_params: an AIDED_PARAMS_DTYPE record of shape (1,) -- a window of 16 blocks, min_segments 1, code_half 16,
    dop_half 1, keep_snr the search threshold, ratio_min the measured default -- with the named fields replaced.  Values outside
    the bounds of include/gpsacq.h ("Aided acquisition", B) raise ValueError here; the entry points check them again."""
    lib = load_library()
    out = np.zeros(1, dtype=AIDED_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_aided_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    for k, v in overrides.items():
        if k not in AIDED_PARAMS_DTYPE.names:
            raise TypeError("aided_params: no field %r" % k)
        if k in ("blocks", "min_segments", "code_half", "dop_half") and int(v) != v:
            raise ValueError("aided_params: %s = %r is no whole number" % (k, v))
        out[k] = v
    r = out[0]
    if not 1 <= r["blocks"] <= 64:
        raise ValueError("aided_params: blocks %d outside 1 .. 64" % r["blocks"])
    if r["min_segments"] < 1:
        raise ValueError("aided_params: min_segments %d (must be >= 1)" % r["min_segments"])
    if not 0 <= r["code_half"] <= 127:
        raise ValueError("aided_params: code_half %d outside 0 .. 127" % r["code_half"])
    if not 0 <= r["dop_half"] <= 8:
        raise ValueError("aided_params: dop_half %d outside 0 .. 8" % r["dop_half"])
    if not (np.isfinite(r["keep_snr"]) and np.isfinite(r["ratio_min"])):
        raise ValueError("aided_params: keep_snr %g, ratio_min %g (must be finite)" % (r["keep_snr"], r["ratio_min"]))
    return out


def aided_params_iq8(**overrides):
    """gpsacq_aided_default_params_iq8: aided_params() with the ratio_min measured for the multi-bit path of aided_search_iq8()
    (include/gpsacq.h, "Aided acquisition on an 8-bit IQ capture"), the named fields replaced."""
    lib = load_library()
    d = np.zeros(1, dtype=AIDED_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_aided_default_params_iq8(d.ctypes.data_as(ctypes.c_void_p)))
    overrides.setdefault("ratio_min", float(d["ratio_min"][0]))
    return aided_params(**overrides)


def aided_coh_params(**overrides):
    """gpsacq_aided_coh_default_params: an AIDED_COH_PARAMS_DTYPE record of shape (1,) -- a window of 16 blocks, min_segments 20,
    code_half 16, dop_half 1, coh_ms 20, fine_half 3, fine_step 25, keep_snr the search threshold, ratio_min the measured default --
    with the named fields replaced.  Values outside the bounds of include/gpsacq.h ("Coherent aided acquisition", A) raise
    ValueError here; the entry points check them again."""
    lib = load_library()
    out = np.zeros(1, dtype=AIDED_COH_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_aided_coh_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    for k, v in overrides.items():
        if k not in AIDED_COH_PARAMS_DTYPE.names:
            raise TypeError("aided_coh_params: no field %r" % k)
        if k not in ("keep_snr", "ratio_min") and int(v) != v:
            raise ValueError("aided_coh_params: %s = %r is no whole number" % (k, v))
        out[k] = v
    r = out[0]
    for k, lo, hi in (("blocks", 1, 64), ("min_segments", 1, 2 ** 31 - 1), ("code_half", 0, 31), ("dop_half", 0, 8), ("fine_half", 0, 7),
                      ("fine_step", 1, 512)):
        if not lo <= r[k] <= hi:
            raise ValueError("aided_coh_params: %s %d outside %d .. %d" % (k, r[k], lo, hi))
    if r["coh_ms"] not in AIDED_COH_MS:
        raise ValueError("aided_coh_params: coh_ms %d is none of %s" % (r["coh_ms"], AIDED_COH_MS))
    if not (np.isfinite(r["keep_snr"]) and np.isfinite(r["ratio_min"])):
        raise ValueError("aided_coh_params: keep_snr %g, ratio_min %g (must be finite)" % (r["keep_snr"], r["ratio_min"]))
    return out


def aided_coh_params_iq8(**overrides):
    """gpsacq_aided_coh_default_params_iq8: aided_coh_params() with the ratio_min measured for the multi-bit path of
    aided_coh_search_iq8() (include/gpsacq.h, "Coherent aided acquisition on an 8-bit IQ capture"), the named fields replaced."""
    lib = load_library()
    d = np.zeros(1, dtype=AIDED_COH_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_aided_coh_default_params_iq8(d.ctypes.data_as(ctypes.c_void_p)))
    overrides.setdefault("ratio_min", float(d["ratio_min"][0]))
    return aided_coh_params(**overrides)


def aided_coh_table():
    """gpsacq_aided_coh_table: the rotation table of the coherent sums, int16 (2, 1024): row 0 is C, row 1 is S"""
    lib = load_library()
    out = np.zeros((2, 1024), dtype=np.int16)
    _check(lib, lib.gpsacq_aided_coh_table(out.ctypes.data_as(ctypes.c_void_p)))
    return out


def coarse_prior(xyz, rx_ms, n_fix=None):
    """COARSE_PRIOR_DTYPE records: the prior place xyz (ECEF metres, (3,) or (n, 3)) and receive time rx_ms (millisecond of week,
    one or n of them), each broadcast to n_fix rows (n_fix None: as many as the longer of the two)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    ms = np.asarray(rx_ms, dtype=np.int64).reshape(-1)
    n = max(xyz.shape[0], ms.size) if n_fix is None else int(n_fix)
    out = np.zeros(n, dtype=COARSE_PRIOR_DTYPE)
    out["x"], out["y"], out["z"] = np.broadcast_to(xyz, (n, 3)).T
    out["rx_ms"] = np.broadcast_to(ms, (n,))
    return out


def smooth_params(**overrides):
    """gpsacq_smooth_default_params: a SMOOTH_PARAMS_DTYPE record of shape (1,) -- window 1000 instants, phase lock over 20 epochs
    at a ratio of 1 / 2, a jump test at a quarter chip (385 << 32), spectrum not inverted -- with the named fields replaced.  The
    entry points that take it check it."""
    lib = load_library()
    out = np.zeros(1, dtype=SMOOTH_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_smooth_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    for k, v in overrides.items():
        if k not in SMOOTH_PARAMS_DTYPE.names:
            raise TypeError("smooth_params: no field %r" % k)
        out[k] = int(v)
    return out


def quality_params(cn0_min_dbhz=30, cn0_ref_dbhz=45, **overrides):
    """gpsacq_quality_default_params: a QUALITY_PARAMS_DTYPE record of shape (1,) -- a window of 200 epochs, at least 20 of them,
    phase lock at a ratio of 1 / 2 and required, cn0_cap_dbhz 99 -- with the gate cn0_min_lin = 10^(cn0_min_dbhz / 10), the
    reference level cn0_ref_lin = 10^(cn0_ref_dbhz / 10) (weight 1 from there up), and then the named fields replaced.  The entry
    points that take it check it."""
    lib = load_library()
    out = np.zeros(1, dtype=QUALITY_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_quality_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    out["cn0_min_lin"] = 10.0 ** (float(cn0_min_dbhz) / 10.0)
    out["cn0_ref_lin"] = 10.0 ** (float(cn0_ref_dbhz) / 10.0)
    for k, v in overrides.items():
        if k not in QUALITY_PARAMS_DTYPE.names:
            raise TypeError("quality_params: no field %r" % k)
        out[k] = v
    return out


def snap_quality_params(min_segments=1, cn0_min_dbhz=None, cn0_ref_dbhz=None, **overrides):
    """gpsacq_snap_quality_default_params: a SNAP_QUALITY_PARAMS_DTYPE record of shape (1,) -- min_segments 1, the gate cn0_min_lin
    500.0 (27.0 dB-Hz: 5.4 sigma of noise alone over 117 segments), the reference level cn0_ref_lin 10^4.35 (43.5 dB-Hz, weight 1
    from there up) -- with min_segments, then the gate 10^(cn0_min_dbhz / 10) and the level 10^(cn0_ref_dbhz / 10) where given, then
    the named fields replaced.  The entry points that take it check it."""
    lib = load_library()
    out = np.zeros(1, dtype=SNAP_QUALITY_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_snap_quality_default_params(out.ctypes.data_as(ctypes.c_void_p)))
    out["min_segments"] = min_segments
    if cn0_min_dbhz is not None:
        out["cn0_min_lin"] = 10.0 ** (float(cn0_min_dbhz) / 10.0)
    if cn0_ref_dbhz is not None:
        out["cn0_ref_lin"] = 10.0 ** (float(cn0_ref_dbhz) / 10.0)
    for k, v in overrides.items():
        if k not in SNAP_QUALITY_PARAMS_DTYPE.names:
            raise TypeError("snap_quality_params: no field %r" % k)
        out[k] = v
    return out


def snap_quality_params_iq8(min_segments=1, cn0_min_dbhz=None, cn0_ref_dbhz=None, **overrides):
    """gpsacq_snap_quality_default_params_iq8: snap_quality_params() with the gate and the reference level measured for the multi-bit
    records of refine_iq8() (include/gpsacq.h, "Snapshot signal quality on an 8-bit IQ capture": cn0_min_lin 1432.4, 31.6 dB-Hz, and
    cn0_ref_lin 10^4.86, 48.6 dB-Hz), then the arguments applied as snap_quality_params() applies them."""
    lib = load_library()
    d = np.zeros(1, dtype=SNAP_QUALITY_PARAMS_DTYPE)
    _check(lib, lib.gpsacq_snap_quality_default_params_iq8(d.ctypes.data_as(ctypes.c_void_p)))
    if cn0_min_dbhz is None:
        overrides.setdefault("cn0_min_lin", float(d["cn0_min_lin"][0]))
    if cn0_ref_dbhz is None:
        overrides.setdefault("cn0_ref_lin", float(d["cn0_ref_lin"][0]))
    return snap_quality_params(min_segments, cn0_min_dbhz, cn0_ref_dbhz, **overrides)


def code_sigma_m(info):
    """The measured pseudorange sigma per channel, metres: the standard deviation of corr * (c / L1) / 2^32 over the observations of
    info (SMOOTH_INFO_DTYPE [n_fix][n_chans]) flagged SMOOTH_FULL; NaN where a channel has none.  The number raim_params(sigma_m=...)
    asks for."""
    info = np.asarray(info)
    if info.dtype != SMOOTH_INFO_DTYPE or info.ndim != 2:
        raise TypeError("info must be a SMOOTH_INFO_DTYPE array [n_fix][n_chans]")
    out = np.full(info.shape[1], np.nan)
    for c in range(info.shape[1]):
        full = (info["flags"][:, c] & SMOOTH_FULL) != 0
        if full.any():
            out[c] = float(np.std(info["corr"][full, c].astype(np.float64) * (C_MPS / L1_HZ / 4294967296.0)))
    return out


def time_tag(subframe, bit_epoch0, eph_index):
    """gpsacq_time_tag_from_subframe: the TIME_TAG_DTYPE record (shape (1,)) of a channel from one of its subframes (a
    SUBFRAME_DTYPE record of nav_subframes), bit_epoch0 being nav_bits' second result for the bit stream the subframe was found in,
    and eph_index the row of the ephemeris table the channel's observations will name."""
    lib = load_library()
    sf = np.zeros(1, dtype=SUBFRAME_DTYPE)
    sf[0] = subframe
    tag = np.zeros(1, dtype=TIME_TAG_DTYPE)
    _check(lib, lib.gpsacq_time_tag_from_subframe(sf.ctypes.data_as(ctypes.c_void_p), int(bit_epoch0), int(eph_index),
                                                  tag.ctypes.data_as(ctypes.c_void_p)))
    return tag


def search_code(sv, g1):
    """SearchCode(), c/search_offline.cpp:205-209."""
    return load_library().gpsacq_search_code(int(sv), int(g1))


class Engine:
    """SearchInit() for one (FC, FS, max_fo); owns the device state."""

    def __init__(self, fc, fs, max_fo=5000.0, device=0, ref_quirks=False):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        prm = Params(float(fc), float(fs), float(max_fo), int(device), 1 if ref_quirks else 0)
        _check(self._lib, self._lib.gpsacq_create(ctypes.byref(prm), ctypes.byref(self._h)))
        self._refresh_info()
        self.fc, self.fs, self.max_fo = float(fc), float(fs), float(max_fo)
        self._quirks = bool(ref_quirks)
        # run-time hand-out of the correlate kernel's cells (gpsacq_set_cell_handout): on unless the environment said 0 at gpsacq_create
        self.cell_handout = os.environ.get("GPSACQ_CORR_PERSIST") != "0"

    def _refresh_info(self):
        info = Info()
        _check(self._lib, self._lib.gpsacq_get_info(self._h, ctypes.byref(info)))
        self.dmax = info.dmax
        self.num_doppler = info.num_doppler
        self.first_doppler = info.first_doppler
        self.num_lags = info.num_lags
        self.acc_columns = info.acc_columns
        self.device = info.device
        self.compute_units = info.compute_units
        self.device_name = info.device_name.decode(errors="replace")
        self.doppler_sub = info.doppler_sub
        self.doppler_stride = info.doppler_stride
        self.num_doppler_total = info.num_doppler_total
        self.first_doppler_total = info.first_doppler_total
        self.kmax = -info.first_doppler_total  # grid points run -kmax..+kmax (= dmax on the reference grid)
        self.doppler_step_hz = info.doppler_step_hz

    def set_doppler_window(self, first_bin, n_bins):
        """Search only bins first_bin .. first_bin+n_bins-1 (multi-GPU Doppler-slab sharding)."""
        _check(self._lib, self._lib.gpsacq_set_doppler_window(self._h, int(first_bin), int(n_bins)))
        self._refresh_info()

    def set_cell_handout(self, on):
        """Run-time hand-out of the correlate kernel's cells to persistent workgroups (default on) or one workgroup per cell
        (gpsacq_set_cell_handout): the same cells bit for bit, a different time."""
        _check(self._lib, self._lib.gpsacq_set_cell_handout(self._h, 1 if on else 0))
        self.cell_handout = bool(on)

    def set_doppler_step(self, step_hz):
        """Doppler grid step in Hz: finer than fs/40000 through sub-bin spectra, coarser through a bin stride
        (include/gpsacq.h).  lo_shift / windows / cells columns then count grid points of doppler_step_hz."""
        _check(self._lib, self._lib.gpsacq_set_doppler_step(self._h, float(step_hz)))
        self._refresh_info()

    def set_noncoherent(self, n_acc, block_step=1):
        """Sum |IFFT|^2 over n_acc blocks (block_step apart) per cell before the peak scan; 1 = reference."""
        _check(self._lib, self._lib.gpsacq_set_noncoherent(self._h, int(n_acc), int(block_step)))

    def set_creep_compensation(self, on=True):
        """Non-coherent mode: re-align each accumulated block by the code creep of the cell's Doppler bin."""
        _check(self._lib, self._lib.gpsacq_set_creep_compensation(self._h, 1 if on else 0))

    def set_block_alignment(self, on=True):
        """Non-coherent mode: re-align each accumulated block by the code phase between block starts (any stride)."""
        _check(self._lib, self._lib.gpsacq_set_block_alignment(self._h, 1 if on else 0))

    def aligned_stride(self):
        """Bytes between block starts that keep lags aligned for non-coherent sums (whole C/A periods)."""
        return self._lib.gpsacq_aligned_stride(self._h)

    def close(self):
        if self._h:
            self._lib.gpsacq_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def handoff(self, peak, secs_since_sample=0.0):
        """Hand-off record of a hit of THIS engine: its fc, fs and current Doppler grid step."""
        pk = np.zeros(1, dtype=PEAK_DTYPE)
        pk[0] = peak
        h = Handoff()
        _check(self._lib, self._lib.gpsacq_handoff_engine(self._h, pk.ctypes.data_as(ctypes.c_void_p), float(secs_since_sample), ctypes.byref(h)))
        return {k: getattr(h, k) for k, _ in Handoff._fields_}

    # ---- 8-bit IQ capture searched directly (no 1-bit intermediate) -------------------------
    @staticmethod
    def iq8_input(signed=False, remove_dc=True, mean=(0.0, 0.0), mix_hz=0.0, fs=0.0, first_sample=0, total_samples=0, multibit=False):
        return Iq8Input(1 if signed else 0, 1 if remove_dc else 0, float(mean[0]), float(mean[1]), float(mix_hz), float(fs),
                        int(first_sample), int(total_samples), int(multibit), 0)  # multibit: False/0 sign, True/1 real IF, 2 complex baseband

    def iq8_mean(self, iq, signed=False, chunk_samples=1 << 22):
        """Complex mean of a whole 8-bit IQ capture as (mean_i, mean_q): exact integer sums on the device, in pieces."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        n = buf.size // 2
        sums = (ctypes.c_int64 * 2)(0, 0)
        for s0 in range(0, n, chunk_samples):
            m = min(chunk_samples, n - s0)
            part = buf[2 * s0:2 * (s0 + m)]
            _check(self._lib, self._lib.gpsacq_iq8_accumulate_sums(self._h, part.ctypes.data_as(ctypes.c_void_p), m, 1 if signed else 0, sums))
        return sums[0] / n, sums[1] / n

    def search_iq8(self, iq, inp, tasks=None, stride=16 * BLOCK_BYTES, want_cells=True):
        """Search interleaved 8-bit I,Q bytes directly (gpsacq_search_iq8): blocks `stride` bytes apart (81920 = the 40960
        samples of one Sample() call).  inp: Engine.iq8_input(...)."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        need = 16 * (BLOCK_BYTES if self._quirks else 5000)
        n_blocks = (buf.size - min(stride, need)) // stride + 1 if buf.size >= min(stride, need) else 0
        if n_blocks <= 0:
            raise ValueError("capture shorter than one block")
        if tasks is None:
            n_tasks, tptr = n_blocks, None
        else:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            n_tasks, tptr = t.shape[0], t.ctypes.data_as(ctypes.c_void_p)
        cells = np.zeros((n_tasks, self.num_doppler), dtype=CELL_DTYPE) if want_cells else None
        peaks = np.zeros(n_tasks, dtype=PEAK_DTYPE)
        _check(self._lib, self._lib.gpsacq_search_iq8(
            self._h, ctypes.byref(inp), buf.ctypes.data_as(ctypes.c_void_p), n_blocks, stride, tptr, n_tasks,
            cells.ctypes.data_as(ctypes.c_void_p) if want_cells else None, peaks.ctypes.data_as(ctypes.c_void_p)))
        return cells, peaks

    def search_iq8_device(self, d_iq_ptr, inp, n_blocks, d_peaks_ptr, stride=16 * BLOCK_BYTES, sync=True, d_tasks_ptr=None, n_tasks=None):
        """gpsacq_search_iq8_device: the capture (device, 16-byte aligned) searched on the reference schedule, or on a task list in
        device memory (d_tasks_ptr, n_tasks)."""
        _check(self._lib, self._lib.gpsacq_search_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, n_blocks, stride, d_tasks_ptr,
                                                             n_blocks if n_tasks is None else int(n_tasks), None, d_peaks_ptr, 1 if sync else 0))

    # ---- pipelined host-buffer searches (gpsacq_pipe_*) --------------------------------------
    def pipe_buffer(self, slot, nbytes):
        """The slot's pinned staging buffer as a writable uint8 array of nbytes."""
        ptr = self._lib.gpsacq_pipe_buffer(self._h, int(slot), int(nbytes))
        if not ptr:
            raise GpsAcqError(-1, self._lib.gpsacq_last_error().decode(errors="replace"))
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(int(nbytes),))

    def pipe_submit(self, slot, n_blocks, stride=BLOCK_BYTES, iq=None):
        _check(self._lib, self._lib.gpsacq_pipe_submit(self._h, int(slot), int(n_blocks), int(stride), ctypes.byref(iq) if iq is not None else None))

    def pipe_collect(self, slot):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self._lib, self._lib.gpsacq_pipe_collect(self._h, int(slot), ctypes.byref(p), ctypes.byref(n)))
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value * PEAK_DTYPE.itemsize,))
        return arr.view(PEAK_DTYPE).copy()

    # ---- host-buffer path ----------------------------------------------------------------
    def search(self, bits, tasks=None, stride=BLOCK_BYTES, want_cells=True, n_tasks=None):
        """bits: bytes-like / uint8 array holding whole 5120-byte blocks.  tasks: None for the
        reference schedule (block t against PRN t % 32) or an array of (block, prn) pairs.
        Returns (cells[n_tasks, num_doppler] or None, peaks[n_tasks])."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        n_blocks = (buf.size - min(stride, BLOCK_BYTES)) // stride + 1 if buf.size >= min(stride, BLOCK_BYTES) else 0
        if n_blocks <= 0:
            raise ValueError("capture shorter than one block")
        if tasks is None:
            n_tasks, tptr = (n_blocks if n_tasks is None else int(n_tasks)), None
        else:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            n_tasks, tptr = t.shape[0], t.ctypes.data_as(ctypes.c_void_p)
        cells = np.zeros((n_tasks, self.num_doppler), dtype=CELL_DTYPE) if want_cells else None
        peaks = np.zeros(n_tasks, dtype=PEAK_DTYPE)
        _check(self._lib, self._lib.gpsacq_search(
            self._h, buf.ctypes.data_as(ctypes.c_void_p), n_blocks, stride, tptr, n_tasks,
            cells.ctypes.data_as(ctypes.c_void_p) if want_cells else None, peaks.ctypes.data_as(ctypes.c_void_p)))
        return cells, peaks

    # ---- device-buffer path (torch tensors on this engine's device) ----------------------
    def search_device(self, d_bits_ptr, n_blocks, d_peaks_ptr, stride=BLOCK_BYTES, d_tasks_ptr=None, n_tasks=None,
                      d_cells_ptr=None, sync=True):
        n_tasks = n_blocks if n_tasks is None else n_tasks
        _check(self._lib, self._lib.gpsacq_search_device(self._h, d_bits_ptr, n_blocks, stride, d_tasks_ptr, n_tasks,
                                                         d_cells_ptr, d_peaks_ptr, 1 if sync else 0))

    def peak_keys_device(self, d_peaks_ptr, n_peaks, d_keys_ptr, per_prn=True, sync=False):
        """gpsacq_peak_keys_device: the multi-GPU merge keys of a device search's peaks, on the engine's stream.  per_prn: 32 keys
        (best per PRN, reference schedule); else one per peak.  d_keys: int64 / uint64 device memory."""
        _check(self._lib, self._lib.gpsacq_peak_keys_device(self._h, d_peaks_ptr if n_peaks else None, int(n_peaks), 1 if per_prn else 0,
                                                            d_keys_ptr, 1 if sync else 0))

    def cycle_stamp_device(self, d_stamp_ptr, sync=False):
        """gpsacq_cycle_stamp_device: every compute unit's shader-cycle counter written to d_stamp[xcc << 6 | se << 4 | cu]
        (STAMP_SLOTS x 8 bytes of zeroed device memory), on the engine's stream."""
        _check(self._lib, self._lib.gpsacq_cycle_stamp_device(self._h, d_stamp_ptr, 1 if sync else 0))

    def synchronize(self):
        _check(self._lib, self._lib.gpsacq_synchronize(self._h))

    def reserve(self, n_blocks):
        """Scratch (and the cached reference schedule) for batches of up to n_blocks blocks, once (gpsacq_reserve)."""
        _check(self._lib, self._lib.gpsacq_reserve(self._h, int(n_blocks)))

    def last_timing(self, n_back=0):
        """Stage times (ms) of the search n_back calls ago (0 = the last one); waits for that search only."""
        t = Timing()
        _check(self._lib, self._lib.gpsacq_timing_ago(self._h, int(n_back), ctypes.byref(t)))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    @property
    def stream_ptr(self):
        """The engine's hipStream_t as an integer (e.g. for torch.cuda.ExternalStream)."""
        return int(self._lib.gpsacq_stream(self._h) or 0)

    # ---- synthetic captures ---------------------------------------------------------------
    @staticmethod
    def _sats(sats):
        arr = (Sat * max(1, len(sats)))()
        for i, (prn, amp, dop, ca, ph) in enumerate(sats):
            arr[i] = Sat(int(prn), float(amp), float(dop), float(ca), float(ph))
        return arr

    def generate(self, n_bytes, sats=(), noise_sigma=1.0, seed=1, first_sample=0, nav=None):
        """Synthetic 1-bit real-IF capture made on the device: sats = [(prn, amplitude, doppler_hz,
        code_phase_samples, carrier_phase_cycles), ...] on top of white noise (gps_sig_gen.m's role).  first_sample (a multiple
        of 8): the n_bytes that start there in the stream -- any range of one capture, bit for bit.  nav: None, or
        [len(sats)][n_nav_bits] navigation bits +-1 (gpsacq_generate_nav_range: 20 code periods per bit, repeating)."""
        out = np.zeros(int(n_bytes), dtype=np.uint8)
        if nav is None:
            _check(self._lib, self._lib.gpsacq_generate_range(self._h, out.ctypes.data_as(ctypes.c_void_p), int(n_bytes), int(first_sample),
                                                              self._sats(sats), len(sats), float(noise_sigma), int(seed)))
            return out
        nv = np.ascontiguousarray(np.asarray(nav, dtype=np.int8).reshape(len(sats), -1))
        _check(self._lib, self._lib.gpsacq_generate_nav_range(self._h, out.ctypes.data_as(ctypes.c_void_p), int(n_bytes), int(first_sample),
                                                              self._sats(sats), len(sats), nv.ctypes.data_as(ctypes.c_void_p), int(nv.shape[1]),
                                                              float(noise_sigma), int(seed)))
        return out

    # ---- tracking channels ----------------------------------------------------------------
    def track_params(self, **overrides):
        """gpsacq_track_default_params for this engine's fs, with any field overridden by name."""
        p = TrackParams()
        _check(self._lib, self._lib.gpsacq_track_default_params(self._h, ctypes.byref(p)))
        for k, v in overrides.items():
            if k not in dict(TrackParams._fields_):
                raise KeyError(f"no tracking parameter {k!r}")
            setattr(p, k, int(v))
        return p

    def _params(self, params):
        if params is None:
            return self.track_params()
        if isinstance(params, dict):
            return self.track_params(**params)
        return params

    def track_start(self, prn, peak, block_first_sample, params=None, **overrides):
        """gpsacq_track_start: a channel (TRACK_CHAN_DTYPE, shape (1,)) for PRN `prn` from a search hit (a PEAK_DTYPE record) of the
        block that starts at absolute sample block_first_sample."""
        p = self._params(params) if not overrides else self.track_params(**overrides)
        pk = np.zeros(1, dtype=PEAK_DTYPE)
        pk[0] = peak
        ch = np.zeros(1, dtype=TRACK_CHAN_DTYPE)
        _check(self._lib, self._lib.gpsacq_track_start(self._h, int(prn), pk.ctypes.data_as(ctypes.c_void_p), int(block_first_sample),
                                                       ctypes.byref(p), ch.ctypes.data_as(ctypes.c_void_p)))
        return ch

    def track(self, bits, chans, first_sample=0, max_epochs=None, records=False, params=None):
        """gpsacq_track over a window (bytes / uint8 array of samples first_sample.. ).  chans: TRACK_CHAN_DTYPE array, updated in
        place.  Returns (prompt int32 [n_chans][max_epochs][2], records [n_chans][max_epochs] or None, n_epochs int32 [n_chans]);
        only the first n_epochs[c] rows of channel c are defined."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        if chans.dtype != TRACK_CHAN_DTYPE or not chans.flags.c_contiguous:
            raise TypeError("chans must be a contiguous TRACK_CHAN_DTYPE array")
        if max_epochs is None:
            max_epochs = int(buf.size * 8 // max(1, self.num_lags // 2)) + 1
        p = self._params(params)
        n = chans.size
        prompt = np.zeros((n, max_epochs, 2), dtype=np.int32)
        rec = np.zeros((n, max_epochs), dtype=TRACK_RECORD_DTYPE) if records else None
        ne = np.zeros(n, dtype=np.int32)
        _check(self._lib, self._lib.gpsacq_track(self._h, buf.ctypes.data_as(ctypes.c_void_p), int(buf.size), int(first_sample),
                                                 chans.ctypes.data_as(ctypes.c_void_p), int(n), ctypes.byref(p),
                                                 prompt.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p) if records else None,
                                                 int(max_epochs), ne.ctypes.data_as(ctypes.c_void_p)))
        return prompt, rec, ne

    def track_device(self, d_bits_ptr, n_bytes, chans, first_sample=0, max_epochs=0, d_prompt_ptr=None, d_records_ptr=None, params=None):
        """gpsacq_track_device: the capture window and the outputs in device memory; chans (host) updated in place.  Returns n_epochs."""
        p = self._params(params)
        ne = np.zeros(chans.size, dtype=np.int32)
        _check(self._lib, self._lib.gpsacq_track_device(self._h, d_bits_ptr, int(n_bytes), int(first_sample), chans.ctypes.data_as(ctypes.c_void_p),
                                                        int(chans.size), ctypes.byref(p), d_prompt_ptr, d_records_ptr, int(max_epochs),
                                                        ne.ctypes.data_as(ctypes.c_void_p)))
        return ne

    # ---- navigation solver ----------------------------------------------------------------
    @staticmethod
    def _nav_arrays(eph, obs):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        if not isinstance(obs, np.ndarray) or obs.dtype != OBS_DTYPE:
            raise TypeError("obs must be an OBS_DTYPE array")
        return ep, np.ascontiguousarray(obs)

    def sat_states(self, eph, obs):
        """gpsacq_sat_states: ECEF position and clock correction (SAT_STATE_DTYPE, obs's shape) of every observation (OBS_DTYPE:
        index into eph, an EPHEMERIS_DTYPE array, and the uncorrected satellite time as tx_ms, tx_frac)."""
        ep, ob = self._nav_arrays(eph, obs)
        out = np.zeros(ob.shape, dtype=SAT_STATE_DTYPE)
        _check(self._lib, self._lib.gpsacq_sat_states(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), ob.ctypes.data_as(ctypes.c_void_p),
                                                      int(ob.size), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def sat_states_device(self, eph, d_obs_ptr, n_obs, d_out_ptr, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        _check(self._lib, self._lib.gpsacq_sat_states_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, int(n_obs),
                                                             d_out_ptr, 1 if sync else 0))

    def fix(self, eph, obs):
        """gpsacq_fix_batch: obs is an OBS_DTYPE array [n_fix][sats_per_fix] (1 .. FIX_MAX_SATS per row, unusable entries are
        skipped); returns FIX_DTYPE [n_fix]."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        out = np.zeros(ob.shape[0], dtype=FIX_DTYPE)
        _check(self._lib, self._lib.gpsacq_fix_batch(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), ob.ctypes.data_as(ctypes.c_void_p),
                                                     int(ob.shape[0]), int(ob.shape[1]), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def fix_device(self, eph, d_obs_ptr, n_fix, sats_per_fix, d_out_ptr, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        _check(self._lib, self._lib.gpsacq_fix_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, int(n_fix),
                                                            int(sats_per_fix), d_out_ptr, 1 if sync else 0))

    def fix_last_ms(self):
        """Device milliseconds of the last fix* call: (satellite-state kernel, fix kernel)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_fix_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- atmosphere, elevation mask and DOP -----------------------------------------------
    @staticmethod
    def _atm_params(params):
        if params is None:
            return None, None
        pr = np.array(params, dtype=ATM_PARAMS_DTYPE).reshape(1).copy()
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def fix_atm(self, eph, obs, params, dop=True, views=False):
        """gpsacq_fix_atm_batch: fix() with the ionosphere, the troposphere and the elevation mask of params (atm_params()).
        Returns FIX_DTYPE [n_fix], then FIX_DOP_DTYPE [n_fix] if dop, then SAT_VIEW_DTYPE [n_fix][sats_per_fix] if views (a tuple
        when more than the fixes is asked for)."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        pr, pp = self._atm_params(params)
        out = np.zeros(ob.shape[0], dtype=FIX_DTYPE)
        dp = np.zeros(ob.shape[0], dtype=FIX_DOP_DTYPE) if dop else None
        vw = np.zeros(ob.shape, dtype=SAT_VIEW_DTYPE) if views else None
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fix_atm_batch(self._h, p(ep), int(ep.size), p(ob), int(ob.shape[0]), int(ob.shape[1]), pp, p(out),
                                                         p(dp), p(vw)))
        res = (out,) + ((dp,) if dop else ()) + ((vw,) if views else ())
        return res if len(res) > 1 else out

    def fix_atm_device(self, eph, d_obs_ptr, n_fix, sats_per_fix, params, d_fix_ptr, d_dop_ptr=None, d_views_ptr=None, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        pr, pp = self._atm_params(params)
        _check(self._lib, self._lib.gpsacq_fix_atm_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, int(n_fix),
                                                                int(sats_per_fix), pp, d_fix_ptr, d_dop_ptr, d_views_ptr, 1 if sync else 0))

    def sat_views(self, eph, obs, fixes, params):
        """gpsacq_sat_views: azimuth, elevation and the two delays (SAT_VIEW_DTYPE [n_fix][sats_per_fix]) of every observation of
        obs (OBS_DTYPE [n_fix][sats_per_fix]) seen from its row's fix (FIX_DTYPE [n_fix])."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        if not isinstance(fixes, np.ndarray) or fixes.dtype != FIX_DTYPE or fixes.shape != (ob.shape[0],):
            raise TypeError("fixes must be a FIX_DTYPE array [n_fix]")
        fx = np.ascontiguousarray(fixes)
        pr, pp = self._atm_params(params)
        out = np.zeros(ob.shape, dtype=SAT_VIEW_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_sat_views(self._h, p(ep), int(ep.size), p(ob), p(fx), int(ob.shape[0]), int(ob.shape[1]), pp, p(out)))
        return out

    def sat_views_device(self, eph, d_obs_ptr, d_fix_ptr, n_fix, sats_per_fix, params, d_out_ptr, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        pr, pp = self._atm_params(params)
        _check(self._lib, self._lib.gpsacq_sat_views_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, d_fix_ptr,
                                                            int(n_fix), int(sats_per_fix), pp, d_out_ptr, 1 if sync else 0))

    def fix_atm_last_ms(self):
        """Device milliseconds of the last fix_atm* call: (satellite-state kernel, corrected-fix kernel, view kernel or 0)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_fix_atm_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- fix integrity ---------------------------------------------------------------------
    @staticmethod
    def _raim_params(params):
        if params is None:
            return None, None
        pr = np.array(params, dtype=RAIM_PARAMS_DTYPE).reshape(1).copy()
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def fix_raim(self, eph, obs, atm_params, raim_params):
        """gpsacq_fix_raim_batch: fix_atm() followed by the chi-square test of its residuals against raim_params (raim_params())
        and, where the test fails, the exclusion of the one observation whose removal mends the fix.  Returns (FIX_DTYPE [n_fix],
        FIX_DOP_DTYPE [n_fix], FIX_RAIM_DTYPE [n_fix])."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        ar, ap = self._atm_params(atm_params)
        rr, rp = self._raim_params(raim_params)
        out = np.zeros(ob.shape[0], dtype=FIX_DTYPE)
        dp = np.zeros(ob.shape[0], dtype=FIX_DOP_DTYPE)
        rm = np.zeros(ob.shape[0], dtype=FIX_RAIM_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fix_raim_batch(self._h, p(ep), int(ep.size), p(ob), int(ob.shape[0]), int(ob.shape[1]), ap, rp, p(out),
                                                          p(dp), p(rm)))
        return out, dp, rm

    def fix_raim_device(self, eph, d_obs_ptr, n_fix, sats_per_fix, atm_params, raim_params, d_fix_ptr, d_dop_ptr, d_raim_ptr, sync=True):
        """gpsacq_fix_raim_batch_device: device pointers for the observations and the three outputs; d_dop_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._atm_params(atm_params)
        rr, rp = self._raim_params(raim_params)
        _check(self._lib, self._lib.gpsacq_fix_raim_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, int(n_fix),
                                                                 int(sats_per_fix), ap, rp, d_fix_ptr, d_dop_ptr, d_raim_ptr, 1 if sync else 0))

    def fix_raim_last_ms(self):
        """Device milliseconds of the last fix_raim* call: (satellite-state kernel, detect kernel, exclude kernel)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_fix_raim_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- coarse-time fixes ------------------------------------------------------------------
    @staticmethod
    def _coarse_params(params):
        if params is None:
            return None, None
        pr = np.array(params, dtype=COARSE_PARAMS_DTYPE).reshape(1).copy()
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def coarse_fix(self, eph, obs, prior, params=None):
        """gpsacq_coarse_fix_batch: one position per row of obs (OBS_DTYPE [n_fix][sats_per_fix], of which only eph, valid, tx_frac
        and weight are read: the code phases) from the prior place and time of prior (COARSE_PRIOR_DTYPE, one record or n_fix;
        coarse_prior()).  Returns (FIX_DTYPE [n_fix], COARSE_INFO_DTYPE [n_fix], OBS_DTYPE [n_fix][sats_per_fix]): the fixes, the
        fifth unknown and the five-state dilutions, and the observations with their whole milliseconds, ready for fix(), fix_atm()
        or fix_raim().  params: coarse_params(), None for the defaults."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        pr = np.ascontiguousarray(np.broadcast_to(np.asarray(prior, dtype=COARSE_PRIOR_DTYPE).ravel(), (ob.shape[0],)))
        cr, cp = self._coarse_params(params)
        out = np.zeros(ob.shape[0], dtype=FIX_DTYPE)
        info = np.zeros(ob.shape[0], dtype=COARSE_INFO_DTYPE)
        oo = np.zeros(ob.shape, dtype=OBS_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_coarse_fix_batch(self._h, p(ep), int(ep.size), p(ob), p(pr), int(ob.shape[0]), int(ob.shape[1]), cp,
                                                            p(out), p(info), p(oo)))
        return out, info, oo

    def coarse_fix_device(self, eph, d_obs_ptr, d_prior_ptr, n_fix, sats_per_fix, d_fix_ptr, d_info_ptr, d_obs_out_ptr=None, params=None, sync=True):
        """gpsacq_coarse_fix_batch_device: device pointers for the observations, the priors and the outputs; d_obs_out_ptr may be
        None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, d_prior_ptr,
                                                                   int(n_fix), int(sats_per_fix), cp, d_fix_ptr, d_info_ptr, d_obs_out_ptr,
                                                                   1 if sync else 0))

    def coarse_fix_raim(self, eph, obs, prior, raim_params, params=None):
        """gpsacq_coarse_raim_batch: coarse_fix() followed by the chi-square test of its residuals against raim_params
        (raim_params(), sigma_m the range sigma of a code phase of weight 1) and, where the test fails, the exclusion of the one
        code phase without which the row passes -- the whole solve again, whole milliseconds included.  Returns (FIX_DTYPE [n_fix],
        COARSE_INFO_DTYPE [n_fix], OBS_DTYPE [n_fix][sats_per_fix], FIX_RAIM_DTYPE [n_fix]); the first three are coarse_fix()'s of the
        row, or of the row without the excluded column.  params: coarse_params(), None for the defaults."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        pr = np.ascontiguousarray(np.broadcast_to(np.asarray(prior, dtype=COARSE_PRIOR_DTYPE).ravel(), (ob.shape[0],)))
        cr, cp = self._coarse_params(params)
        rr, rp = self._raim_params(raim_params)
        out = np.zeros(ob.shape[0], dtype=FIX_DTYPE)
        info = np.zeros(ob.shape[0], dtype=COARSE_INFO_DTYPE)
        oo = np.zeros(ob.shape, dtype=OBS_DTYPE)
        rm = np.zeros(ob.shape[0], dtype=FIX_RAIM_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_coarse_raim_batch(self._h, p(ep), int(ep.size), p(ob), p(pr), int(ob.shape[0]), int(ob.shape[1]), cp, rp,
                                                             p(out), p(info), p(oo), p(rm)))
        return out, info, oo, rm

    def coarse_fix_raim_device(self, eph, d_obs_ptr, d_prior_ptr, n_fix, sats_per_fix, raim_params, d_fix_ptr, d_info_ptr, d_raim_ptr,
                               d_obs_out_ptr=None, params=None, sync=True):
        """gpsacq_coarse_raim_batch_device: device pointers for the observations, the priors and the outputs; d_obs_out_ptr may be
        None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        cr, cp = self._coarse_params(params)
        rr, rp = self._raim_params(raim_params)
        _check(self._lib, self._lib.gpsacq_coarse_raim_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, d_prior_ptr,
                                                                    int(n_fix), int(sats_per_fix), cp, rp, d_fix_ptr, d_info_ptr, d_obs_out_ptr,
                                                                    d_raim_ptr, 1 if sync else 0))

    def coarse_raim_last_ms(self):
        """Device milliseconds of the last coarse_fix_raim* call: (k_coarse_fix, k_coarse_exclude)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_coarse_raim_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def coarse_obs(self, peaks, snr_min=THRESHOLD, fine=None):
        """gpsacq_coarse_obs: search peaks (PEAK_DTYPE [n_fix][n_chans], block outer and channel inner) into code-phase observations
        (OBS_DTYPE, the same shape): valid where snr >= snr_min, eph = the channel, tx_frac = ca_shift / fs, weight 1.
        fine: refine()'s records of those peaks (FINE_DTYPE, as many) -- gpsacq_coarse_obs_fine: valid also needs a usable record,
        and tx_frac is the record's."""
        if not isinstance(peaks, np.ndarray) or peaks.dtype != PEAK_DTYPE or peaks.ndim != 2:
            raise TypeError("peaks must be a PEAK_DTYPE array [n_fix][n_chans]")
        pk = np.ascontiguousarray(peaks)
        out = np.zeros(pk.shape, dtype=OBS_DTYPE)
        if fine is not None:
            if not isinstance(fine, np.ndarray) or fine.dtype != FINE_DTYPE or fine.size != pk.size:
                raise TypeError("fine must be a FINE_DTYPE array with one record per peak")
            fn = np.ascontiguousarray(fine)
            _check(self._lib, self._lib.gpsacq_coarse_obs_fine(self._h, pk.ctypes.data_as(ctypes.c_void_p), fn.ctypes.data_as(ctypes.c_void_p),
                                                               int(pk.shape[0]), int(pk.shape[1]), float(snr_min), out.ctypes.data_as(ctypes.c_void_p)))
            return out
        _check(self._lib, self._lib.gpsacq_coarse_obs(self._h, pk.ctypes.data_as(ctypes.c_void_p), int(pk.shape[0]), int(pk.shape[1]), float(snr_min),
                                                      out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # ---- fine code phases -------------------------------------------------------------------
    @staticmethod
    def _refine_params(params):
        if params is None:
            return None, None
        pr = np.array(params, dtype=REFINE_PARAMS_DTYPE).reshape(1).copy()
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def refine(self, bits, peaks, tasks=None, stride=BLOCK_BYTES, params=None):
        """gpsacq_refine: the peaks of a search of `bits` (PEAK_DTYPE, any shape; tasks as given to search(), None for the reference
        schedule) refined below a sample on a window of consecutive blocks of the capture.  Returns FINE_DTYPE records in the shape
        of peaks.  params: refine_params(), None for the defaults."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        if not isinstance(peaks, np.ndarray) or peaks.dtype != PEAK_DTYPE:
            raise TypeError("peaks must be a PEAK_DTYPE array")
        pk = np.ascontiguousarray(peaks)
        tptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != pk.size:
                raise ValueError("one task per peak")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        rr, rp = self._refine_params(params)
        out = np.zeros(pk.shape, dtype=FINE_DTYPE)
        _check(self._lib, self._lib.gpsacq_refine(self._h, buf.ctypes.data_as(ctypes.c_void_p), int(buf.size), int(stride), tptr,
                                                  pk.ctypes.data_as(ctypes.c_void_p), int(pk.size), rp, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def refine_device(self, d_bits_ptr, n_bytes, d_peaks_ptr, n_tasks, d_fine_ptr, stride=BLOCK_BYTES, d_tasks_ptr=None, params=None, sync=True):
        """gpsacq_refine_device: device pointers for the capture (any byte address), the peaks, the tasks (None: the reference
        schedule) and the records."""
        rr, rp = self._refine_params(params)
        _check(self._lib, self._lib.gpsacq_refine_device(self._h, d_bits_ptr, int(n_bytes), int(stride), d_tasks_ptr, d_peaks_ptr, int(n_tasks), rp,
                                                         d_fine_ptr, 1 if sync else 0))

    def coarse_obs_fine_device(self, d_peaks_ptr, d_fine_ptr, n_fix, n_chans, d_obs_ptr, snr_min=THRESHOLD, sync=True):
        _check(self._lib, self._lib.gpsacq_coarse_obs_fine_device(self._h, d_peaks_ptr, d_fine_ptr, int(n_fix), int(n_chans), float(snr_min), d_obs_ptr,
                                                                  1 if sync else 0))

    def coarse_fix_fine_device(self, eph, d_bits_ptr, n_bytes, d_tasks_ptr, d_peaks_ptr, n_fix, n_chans, d_prior_ptr, d_fix_ptr, d_info_ptr,
                               d_fine_ptr=None, d_obs_ptr=None, d_obs_out_ptr=None, stride=BLOCK_BYTES, refine_params=None, params=None, sync=True):
        """gpsacq_coarse_fix_fine_device: capture, tasks (block outer, channel inner) and peaks -> fine records -> observations ->
        coarse-time fixes in device memory, no host copy in between; d_fine_ptr, d_obs_ptr and d_obs_out_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        rr, rp = self._refine_params(refine_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_fine_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_bits_ptr, int(n_bytes),
                                                                  int(stride), d_tasks_ptr, d_peaks_ptr, int(n_fix), int(n_chans), rp, d_prior_ptr, cp,
                                                                  d_fine_ptr, d_obs_ptr, d_fix_ptr, d_info_ptr, d_obs_out_ptr, 1 if sync else 0))

    def refine_last_ms(self):
        """Device milliseconds of the last refine* calls: (k_refine or 0, k_coarse_obs_fine or 0)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_refine_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- snapshot signal quality -----------------------------------------------------------
    @staticmethod
    def _snap_quality_params(params):
        if params is None:
            return None, None
        pr = np.ascontiguousarray(np.asarray(params, dtype=SNAP_QUALITY_PARAMS_DTYPE).ravel())
        if pr.size != 1:
            raise ValueError("params must be one SNAP_QUALITY_PARAMS_DTYPE record")
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def snap_quality(self, fine, obs=None, params=None):
        """gpsacq_snap_quality: C/N0 (dB-Hz) and the weight of every fine record (FINE_DTYPE [n_fix][n_chans], as refine() returns
        them for peaks of that shape) from its prompt power over the analytic floor.  params: snap_quality_params() (None: the
        defaults).  Returns (None, info) with info QUALITY_INFO_DTYPE [n_fix][n_chans] (epochs = segments); with obs (OBS_DTYPE
        [n_fix][n_chans], made by coarse_obs(peaks, fine=fine)) returns (a copy of obs with the weights set, info)."""
        if not isinstance(fine, np.ndarray) or fine.dtype != FINE_DTYPE or fine.ndim != 2:
            raise TypeError("fine must be a FINE_DTYPE array [n_fix][n_chans]")
        fn = np.ascontiguousarray(fine)
        ob = None
        if obs is not None:
            if not isinstance(obs, np.ndarray) or obs.dtype != OBS_DTYPE or obs.shape != fn.shape:
                raise TypeError("obs must be an OBS_DTYPE array in the shape of fine")
            ob = np.array(obs, order="C")
        pr, pp = self._snap_quality_params(params)
        inf = np.zeros(fn.shape, dtype=QUALITY_INFO_DTYPE)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_snap_quality(self._h, p(fn), int(fn.shape[0]), int(fn.shape[1]), pp, p(ob), p(inf)))
        return ob, inf

    def snap_quality_device(self, d_fine_ptr, n_fix, n_chans, d_info_ptr, d_obs_ptr=None, params=None, sync=True):
        """gpsacq_snap_quality_device: the records, the info and the in-out observations (may be None) in device memory."""
        pr, pp = self._snap_quality_params(params)
        _check(self._lib, self._lib.gpsacq_snap_quality_device(self._h, d_fine_ptr, int(n_fix), int(n_chans), pp, d_obs_ptr, d_info_ptr,
                                                               1 if sync else 0))

    def coarse_fix_quality_device(self, eph, d_bits_ptr, n_bytes, d_tasks_ptr, d_peaks_ptr, n_fix, n_chans, d_prior_ptr, d_fix_ptr, d_info_ptr,
                                  d_fine_ptr=None, d_obs_ptr=None, d_qinfo_ptr=None, d_obs_out_ptr=None, stride=BLOCK_BYTES, refine_params=None,
                                  quality_params=None, params=None, sync=True):
        """gpsacq_coarse_fix_quality_device: coarse_fix_fine_device with the snapshot quality weights between the observations and
        the fix, no host copy in between; d_fine_ptr, d_obs_ptr, d_qinfo_ptr and d_obs_out_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        rr, rp = self._refine_params(refine_params)
        qr, qp = self._snap_quality_params(quality_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_quality_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_bits_ptr,
                                                                     int(n_bytes), int(stride), d_tasks_ptr, d_peaks_ptr, int(n_fix), int(n_chans),
                                                                     rp, qp, d_prior_ptr, cp, d_fine_ptr, d_obs_ptr, d_qinfo_ptr, d_fix_ptr,
                                                                     d_info_ptr, d_obs_out_ptr, 1 if sync else 0))

    def snap_quality_last_ms(self):
        """Device milliseconds of k_snap_quality as last run on this engine."""
        a = ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_snap_quality_last_ms(self._h, ctypes.byref(a)))
        return a.value

    # ---- cold snapshot fixes ----------------------------------------------------------------
    @staticmethod
    def _record(params, dtype):
        if params is None:
            return None, None
        pr = np.array(params, dtype=dtype).reshape(1).copy()
        return pr, pr.ctypes.data_as(ctypes.c_void_p)

    def fine_doppler(self, bits, peaks, tasks=None, stride=BLOCK_BYTES, params=None):
        """gpsacq_fine_doppler: the Doppler of the peaks of a search of `bits` (PEAK_DTYPE, any shape; tasks as given to search(),
        None for the reference schedule) below a bin, from the turn of the 1 ms prompt sums over a window of consecutive blocks.
        Returns DOPFINE_DTYPE records in the shape of peaks.  params: dopfine_params(), None for the defaults."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        if not isinstance(peaks, np.ndarray) or peaks.dtype != PEAK_DTYPE:
            raise TypeError("peaks must be a PEAK_DTYPE array")
        pk = np.ascontiguousarray(peaks)
        tptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != pk.size:
                raise ValueError("one task per peak")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        dr, dp = self._record(params, DOPFINE_PARAMS_DTYPE)
        out = np.zeros(pk.shape, dtype=DOPFINE_DTYPE)
        _check(self._lib, self._lib.gpsacq_fine_doppler(self._h, buf.ctypes.data_as(ctypes.c_void_p), int(buf.size), int(stride), tptr,
                                                        pk.ctypes.data_as(ctypes.c_void_p), int(pk.size), dp, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def fine_doppler_device(self, d_bits_ptr, n_bytes, d_peaks_ptr, n_tasks, d_dopfine_ptr, stride=BLOCK_BYTES, d_tasks_ptr=None, params=None,
                            sync=True):
        """gpsacq_fine_doppler_device: device pointers for the capture (any byte address), the peaks, the tasks (None: the reference
        schedule) and the records."""
        dr, dp = self._record(params, DOPFINE_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_fine_doppler_device(self._h, d_bits_ptr, int(n_bytes), int(stride), d_tasks_ptr, d_peaks_ptr, int(n_tasks),
                                                               dp, d_dopfine_ptr, 1 if sync else 0))

    def rate_obs_fine(self, peaks, dopfine, snr_min=THRESHOLD):
        """gpsacq_rate_obs_fine: search peaks (PEAK_DTYPE [n_fix][n_chans]) and their fine_doppler() records into rate observations
        (RATE_OBS_DTYPE, the same shape): valid where snr >= snr_min and the record is usable, doppler_hz the record's, weight 1."""
        if not isinstance(peaks, np.ndarray) or peaks.dtype != PEAK_DTYPE or peaks.ndim != 2:
            raise TypeError("peaks must be a PEAK_DTYPE array [n_fix][n_chans]")
        if not isinstance(dopfine, np.ndarray) or dopfine.dtype != DOPFINE_DTYPE or dopfine.size != peaks.size:
            raise TypeError("dopfine must be a DOPFINE_DTYPE array with one record per peak")
        pk, df = np.ascontiguousarray(peaks), np.ascontiguousarray(dopfine)
        out = np.zeros(pk.shape, dtype=RATE_OBS_DTYPE)
        _check(self._lib, self._lib.gpsacq_rate_obs_fine(self._h, pk.ctypes.data_as(ctypes.c_void_p), df.ctypes.data_as(ctypes.c_void_p),
                                                         int(pk.shape[0]), int(pk.shape[1]), float(snr_min), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def rate_obs_fine_device(self, d_peaks_ptr, d_dopfine_ptr, n_fix, n_chans, d_rate_obs_ptr, snr_min=THRESHOLD, sync=True):
        _check(self._lib, self._lib.gpsacq_rate_obs_fine_device(self._h, d_peaks_ptr, d_dopfine_ptr, int(n_fix), int(n_chans), float(snr_min),
                                                                d_rate_obs_ptr, 1 if sync else 0))

    def doppler_fix(self, eph, obs, rate_obs, rx_ms, params=None):
        """gpsacq_doppler_fix_batch: one place per row from Dopplers alone, with no prior of place: obs (OBS_DTYPE
        [n_fix][sats_per_fix], of which only eph and valid are read), rate_obs (RATE_OBS_DTYPE, the same shape) and rx_ms (int32,
        one value or n_fix), the receive time to about 30 s.  Returns (DOPPLER_FIX_DTYPE [n_fix], COARSE_PRIOR_DTYPE [n_fix]): the
        fixes, and the priors coarse_fix() takes (NaN where a row failed).  params: doppler_fix_params(), None for the defaults."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        ro = np.ascontiguousarray(np.asarray(rate_obs, dtype=RATE_OBS_DTYPE))
        if ro.shape != ob.shape:
            raise ValueError("rate_obs must have the shape of obs")
        rx = np.ascontiguousarray(np.broadcast_to(np.asarray(rx_ms, dtype=np.int32).ravel(), (ob.shape[0],)))
        fr, fp = self._record(params, DOPPLER_FIX_PARAMS_DTYPE)
        out = np.zeros(ob.shape[0], dtype=DOPPLER_FIX_DTYPE)
        pr = np.zeros(ob.shape[0], dtype=COARSE_PRIOR_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_doppler_fix_batch(self._h, p(ep), int(ep.size), p(ob), p(ro), p(rx), int(ob.shape[0]), int(ob.shape[1]), fp,
                                                             p(out), p(pr)))
        return out, pr

    def doppler_fix_device(self, eph, d_obs_ptr, d_rate_obs_ptr, d_rx_ms_ptr, n_fix, sats_per_fix, d_doppler_fix_ptr, d_prior_ptr=None, params=None,
                           sync=True):
        """gpsacq_doppler_fix_batch_device: device pointers for the observations, the times and the outputs; d_prior_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        fr, fp = self._record(params, DOPPLER_FIX_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_doppler_fix_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, d_rate_obs_ptr,
                                                                    d_rx_ms_ptr, int(n_fix), int(sats_per_fix), fp, d_doppler_fix_ptr, d_prior_ptr,
                                                                    1 if sync else 0))

    def cold_fix_device(self, eph, d_bits_ptr, n_bytes, d_tasks_ptr, d_peaks_ptr, d_rx_ms_ptr, n_fix, n_chans, d_fix_ptr, d_info_ptr,
                        d_doppler_fix_ptr, d_dopfine_ptr=None, d_rate_obs_ptr=None, d_prior_ptr=None, d_fine_ptr=None, d_obs_ptr=None,
                        d_obs_out_ptr=None, stride=BLOCK_BYTES, dopfine_params=None, doppler_params=None, refine_params=None, params=None, sync=True):
        """gpsacq_cold_fix_device: capture, tasks (block outer, channel inner), peaks and rx_ms (int32 [n_fix]) -> fine Dopplers ->
        Doppler fixes -> fine code phases -> coarse-time fixes in device memory, no host copy in between and no prior of place; the
        six optional buffers may be None.  d_obs_out_ptr, d_rate_obs_ptr and d_fix_ptr go into velocity_device() unchanged."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        dr, dp = self._record(dopfine_params, DOPFINE_PARAMS_DTYPE)
        fr, fp = self._record(doppler_params, DOPPLER_FIX_PARAMS_DTYPE)
        rr, rp = self._refine_params(refine_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_cold_fix_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_bits_ptr, int(n_bytes),
                                                           int(stride), d_tasks_ptr, d_peaks_ptr, d_rx_ms_ptr, int(n_fix), int(n_chans), dp, fp, rp, cp,
                                                           d_dopfine_ptr, d_rate_obs_ptr, d_doppler_fix_ptr, d_prior_ptr, d_fine_ptr, d_obs_ptr,
                                                           d_fix_ptr, d_info_ptr, d_obs_out_ptr, 1 if sync else 0))

    def doppler_last_ms(self):
        """Device milliseconds of the last cold-fix calls: (k_fine_dop or 0, k_rate_obs_fine or 0, k_doppler_fix or 0)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_doppler_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- snapshot chain on an 8-bit IQ capture ------------------------------------------------
    @staticmethod
    def _iq8_peaks_tasks(iq, peaks, tasks):
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        if not isinstance(peaks, np.ndarray) or peaks.dtype != PEAK_DTYPE:
            raise TypeError("peaks must be a PEAK_DTYPE array")
        pk = np.ascontiguousarray(peaks)
        t = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != pk.size:
                raise ValueError("one task per peak")
        return buf, pk, t

    def refine_iq8(self, iq, inp, peaks, tasks=None, stride=16 * BLOCK_BYTES, params=None, n_samples=None):
        """gpsacq_refine_iq8: refine() on interleaved 8-bit I, Q bytes, for the peaks of search_iq8() with the same inp
        (Engine.iq8_input(...)): multi-bit complex sums where inp.multibit != 0, the 1-bit path on the converted capture in sign
        mode.  stride in BYTES (a multiple of 16, >= 80000); n_samples: the capture's length (None: all of iq).  Returns
        FINE_DTYPE records in the shape of peaks."""
        buf, pk, t = self._iq8_peaks_tasks(iq, peaks, tasks)
        n = buf.size // 2 if n_samples is None else int(n_samples)
        rr, rp = self._refine_params(params)
        out = np.zeros(pk.shape, dtype=FINE_DTYPE)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_refine_iq8(self._h, ctypes.byref(inp), p(buf), n, int(stride), p(t), p(pk), int(pk.size), rp, p(out)))
        return out

    def refine_iq8_device(self, inp, d_iq_ptr, n_samples, d_peaks_ptr, n_tasks, d_fine_ptr, stride=16 * BLOCK_BYTES, d_tasks_ptr=None, params=None,
                          sync=True):
        """gpsacq_refine_iq8_device: device pointers for the capture (16-byte aligned), the peaks, the tasks (None: the reference
        schedule) and the records."""
        rr, rp = self._refine_params(params)
        _check(self._lib, self._lib.gpsacq_refine_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr, d_peaks_ptr,
                                                             int(n_tasks), rp, d_fine_ptr, 1 if sync else 0))

    def fine_doppler_iq8(self, iq, inp, peaks, tasks=None, stride=16 * BLOCK_BYTES, params=None, n_samples=None):
        """gpsacq_fine_doppler_iq8: fine_doppler() on interleaved 8-bit I, Q bytes, as refine_iq8().  Returns DOPFINE_DTYPE records
        in the shape of peaks; doppler_hz is in the search's own sense."""
        buf, pk, t = self._iq8_peaks_tasks(iq, peaks, tasks)
        n = buf.size // 2 if n_samples is None else int(n_samples)
        dr, dp = self._record(params, DOPFINE_PARAMS_DTYPE)
        out = np.zeros(pk.shape, dtype=DOPFINE_DTYPE)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fine_doppler_iq8(self._h, ctypes.byref(inp), p(buf), n, int(stride), p(t), p(pk), int(pk.size), dp, p(out)))
        return out

    def fine_doppler_iq8_device(self, inp, d_iq_ptr, n_samples, d_peaks_ptr, n_tasks, d_dopfine_ptr, stride=16 * BLOCK_BYTES, d_tasks_ptr=None,
                                params=None, sync=True):
        """gpsacq_fine_doppler_iq8_device: device pointers, as refine_iq8_device()."""
        dr, dp = self._record(params, DOPFINE_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_fine_doppler_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr,
                                                                   d_peaks_ptr, int(n_tasks), dp, d_dopfine_ptr, 1 if sync else 0))

    def coarse_fix_fine_iq8_device(self, eph, inp, d_iq_ptr, n_samples, d_tasks_ptr, d_peaks_ptr, n_fix, n_chans, d_prior_ptr, d_fix_ptr, d_info_ptr,
                                   d_fine_ptr=None, d_obs_ptr=None, d_obs_out_ptr=None, stride=16 * BLOCK_BYTES, refine_params=None, params=None,
                                   sync=True):
        """gpsacq_coarse_fix_fine_iq8_device: coarse_fix_fine_device() on an 8-bit IQ capture."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        rr, rp = self._refine_params(refine_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_fine_iq8_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), ctypes.byref(inp),
                                                                      d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr, d_peaks_ptr, int(n_fix),
                                                                      int(n_chans), rp, d_prior_ptr, cp, d_fine_ptr, d_obs_ptr, d_fix_ptr, d_info_ptr,
                                                                      d_obs_out_ptr, 1 if sync else 0))

    def cold_fix_iq8_device(self, eph, inp, d_iq_ptr, n_samples, d_tasks_ptr, d_peaks_ptr, d_rx_ms_ptr, n_fix, n_chans, d_fix_ptr, d_info_ptr,
                            d_doppler_fix_ptr, d_dopfine_ptr=None, d_rate_obs_ptr=None, d_prior_ptr=None, d_fine_ptr=None, d_obs_ptr=None,
                            d_obs_out_ptr=None, stride=16 * BLOCK_BYTES, dopfine_params=None, doppler_params=None, refine_params=None, params=None,
                            sync=True):
        """gpsacq_cold_fix_iq8_device: cold_fix_device() on an 8-bit IQ capture."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        dr, dp = self._record(dopfine_params, DOPFINE_PARAMS_DTYPE)
        fr, fp = self._record(doppler_params, DOPPLER_FIX_PARAMS_DTYPE)
        rr, rp = self._refine_params(refine_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_cold_fix_iq8_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), ctypes.byref(inp), d_iq_ptr,
                                                               int(n_samples), int(stride), d_tasks_ptr, d_peaks_ptr, d_rx_ms_ptr, int(n_fix),
                                                               int(n_chans), dp, fp, rp, cp, d_dopfine_ptr, d_rate_obs_ptr, d_doppler_fix_ptr,
                                                               d_prior_ptr, d_fine_ptr, d_obs_ptr, d_fix_ptr, d_info_ptr, d_obs_out_ptr,
                                                               1 if sync else 0))

    def snapshot_iq8_last_ms(self):
        """Device milliseconds of the last *_iq8 snapshot call: (conversion or 0, fine-record kernel or 0, fine-Doppler kernel or 0)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_snapshot_iq8_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- aided acquisition ------------------------------------------------------------------
    def aid_predict(self, eph, fix, n_chans, vel=None, params=None):
        """gpsacq_aid_predict: the code phase and Doppler the first n_chans ephemerides of eph should show at the receive instant
        of each fix (FIX_DTYPE [n_fix]; vel: VEL_DTYPE [n_fix] or None, a receiver at rest).  Returns AID_DTYPE [n_fix][n_chans].
        params: aid_params(), None for the defaults."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        fx = np.ascontiguousarray(np.asarray(fix, dtype=FIX_DTYPE).ravel())
        vptr = None
        if vel is not None:
            vl = np.ascontiguousarray(np.asarray(vel, dtype=VEL_DTYPE).ravel())
            if vl.size != fx.size:
                raise ValueError("one velocity per fix")
            vptr = vl.ctypes.data_as(ctypes.c_void_p)
        ar, ap = self._record(params, AID_PARAMS_DTYPE)
        out = np.zeros((fx.size, int(n_chans)), dtype=AID_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aid_predict(self._h, p(ep), int(ep.size), p(fx), vptr, int(fx.size), int(n_chans), ap, p(out)))
        return out

    def aid_predict_device(self, eph, d_fix_ptr, n_fix, n_chans, d_aid_ptr, d_vel_ptr=None, params=None, sync=True):
        """gpsacq_aid_predict_device: device pointers for the fixes, the velocities (None: at rest) and the records."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._record(params, AID_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aid_predict_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_fix_ptr, d_vel_ptr, int(n_fix),
                                                              int(n_chans), ap, d_aid_ptr, 1 if sync else 0))

    def aided_search(self, bits, aid, tasks=None, peaks_in=None, stride=BLOCK_BYTES, params=None, powers=False):
        """gpsacq_aided_search: the capture searched once more around the predictions `aid` (AID_DTYPE, any shape; tasks as given to
        search(), None for the reference schedule) over a window of consecutive blocks; peaks_in (PEAK_DTYPE, as many, or None):
        what the plain search returned, kept where its snr reaches keep_snr.  Returns (AIDED_DTYPE, PEAK_DTYPE) in the shape of aid,
        and with powers=True also the powers, uint64 [n_tasks][2 K + 1][2 W + 1].  The snr of an aided peak is its ratio to the
        noise floor, not a search snr.  params: aided_params(), None for the defaults."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        if not isinstance(aid, np.ndarray) or aid.dtype != AID_DTYPE:
            raise TypeError("aid must be an AID_DTYPE array")
        ad = np.ascontiguousarray(aid)
        tptr = iptr = wptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != ad.size:
                raise ValueError("one task per prediction")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        if peaks_in is not None:
            if not isinstance(peaks_in, np.ndarray) or peaks_in.dtype != PEAK_DTYPE or peaks_in.size != ad.size:
                raise TypeError("peaks_in must be a PEAK_DTYPE array with one peak per prediction")
            pi = np.ascontiguousarray(peaks_in)
            iptr = pi.ctypes.data_as(ctypes.c_void_p)
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        prm = aided_params() if sr is None else sr
        out = np.zeros(ad.shape, dtype=AIDED_DTYPE)
        pk = np.zeros(ad.shape, dtype=PEAK_DTYPE)
        if powers:
            pw = np.zeros((ad.size, 2 * int(prm["dop_half"][0]) + 1, 2 * int(prm["code_half"][0]) + 1), dtype=np.uint64)
            wptr = pw.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aided_search(self._h, buf.ctypes.data_as(ctypes.c_void_p), int(buf.size), int(stride), tptr,
                                                        ad.ctypes.data_as(ctypes.c_void_p), iptr, int(ad.size), sp, out.ctypes.data_as(ctypes.c_void_p),
                                                        pk.ctypes.data_as(ctypes.c_void_p), wptr))
        return (out, pk, pw) if powers else (out, pk)

    def aided_search_device(self, d_bits_ptr, n_bytes, d_aid_ptr, n_tasks, d_aided_ptr, d_peaks_out_ptr, stride=BLOCK_BYTES, d_tasks_ptr=None,
                            d_peaks_in_ptr=None, d_powers_ptr=None, params=None, sync=True):
        """gpsacq_aided_search_device: device pointers for the capture (any byte address), the predictions, the tasks (None: the
        reference schedule), the input peaks (None: nothing is kept), the records, the output peaks and the powers (None)."""
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_search_device(self._h, d_bits_ptr, int(n_bytes), int(stride), d_tasks_ptr, d_aid_ptr, d_peaks_in_ptr,
                                                               int(n_tasks), sp, d_aided_ptr, d_peaks_out_ptr, d_powers_ptr, 1 if sync else 0))

    def aided_peaks_device(self, eph, d_fix_ptr, d_bits_ptr, n_bytes, d_tasks_ptr, n_fix, n_chans, d_aided_ptr, d_peaks_out_ptr, d_vel_ptr=None,
                           d_peaks_in_ptr=None, d_aid_ptr=None, stride=BLOCK_BYTES, aid_params=None, params=None, sync=True):
        """gpsacq_aided_peaks_device: fixes (and velocities) -> predictions -> aided peaks in device memory, no host copy in between;
        tasks block outer and channel inner; d_vel_ptr, d_peaks_in_ptr and d_aid_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._record(aid_params, AID_PARAMS_DTYPE)
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_peaks_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_fix_ptr, d_vel_ptr, d_bits_ptr,
                                                              int(n_bytes), int(stride), d_tasks_ptr, d_peaks_in_ptr, int(n_fix), int(n_chans), ap, sp,
                                                              d_aid_ptr, d_aided_ptr, d_peaks_out_ptr, 1 if sync else 0))

    def aided_last_ms(self):
        """Device milliseconds of the last aided calls: (k_aid_predict or 0, k_aided or 0)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_aided_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- aided acquisition on an 8-bit IQ capture ----------------------------------------------
    def aided_search_iq8(self, iq, inp, aid, tasks=None, peaks_in=None, stride=16 * BLOCK_BYTES, params=None, powers=False, n_samples=None):
        """gpsacq_aided_search_iq8: aided_search() on interleaved 8-bit I, Q bytes, with inp (Engine.iq8_input(...)) as given to
        search_iq8(): multi-bit complex sums against the measured floor where inp.multibit != 0, the 1-bit path on the converted
        capture in sign mode.  stride in BYTES (a multiple of 16, >= 80000); n_samples: the capture's length (None: all of iq).
        params: aided_params_iq8() or aided_params(), None for the defaults of gpsacq_aided_default_params_iq8.  Returns
        (AIDED_DTYPE, PEAK_DTYPE) in the shape of aid, and with powers=True also uint64 [n_tasks][2 K + 1][2 W + 1]."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        n = buf.size // 2 if n_samples is None else int(n_samples)
        if not isinstance(aid, np.ndarray) or aid.dtype != AID_DTYPE:
            raise TypeError("aid must be an AID_DTYPE array")
        ad = np.ascontiguousarray(aid)
        tptr = iptr = wptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != ad.size:
                raise ValueError("one task per prediction")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        if peaks_in is not None:
            if not isinstance(peaks_in, np.ndarray) or peaks_in.dtype != PEAK_DTYPE or peaks_in.size != ad.size:
                raise TypeError("peaks_in must be a PEAK_DTYPE array with one peak per prediction")
            pi = np.ascontiguousarray(peaks_in)
            iptr = pi.ctypes.data_as(ctypes.c_void_p)
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        prm = aided_params_iq8() if sr is None else sr
        out = np.zeros(ad.shape, dtype=AIDED_DTYPE)
        pk = np.zeros(ad.shape, dtype=PEAK_DTYPE)
        if powers:
            pw = np.zeros((ad.size, 2 * int(prm["dop_half"][0]) + 1, 2 * int(prm["code_half"][0]) + 1), dtype=np.uint64)
            wptr = pw.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aided_search_iq8(self._h, ctypes.byref(inp), buf.ctypes.data_as(ctypes.c_void_p), n, int(stride), tptr,
                                                            ad.ctypes.data_as(ctypes.c_void_p), iptr, int(ad.size), sp,
                                                            out.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p), wptr))
        return (out, pk, pw) if powers else (out, pk)

    def aided_search_iq8_device(self, inp, d_iq_ptr, n_samples, d_aid_ptr, n_tasks, d_aided_ptr, d_peaks_out_ptr, stride=16 * BLOCK_BYTES,
                                d_tasks_ptr=None, d_peaks_in_ptr=None, d_powers_ptr=None, params=None, sync=True):
        """gpsacq_aided_search_iq8_device: device pointers for the capture (16-byte aligned), the predictions, the tasks (None: the
        reference schedule), the input peaks (None: nothing is kept), the records, the output peaks and the powers (None)."""
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_search_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr,
                                                                   d_aid_ptr, d_peaks_in_ptr, int(n_tasks), sp, d_aided_ptr, d_peaks_out_ptr,
                                                                   d_powers_ptr, 1 if sync else 0))

    def aided_peaks_iq8_device(self, eph, d_fix_ptr, inp, d_iq_ptr, n_samples, d_tasks_ptr, n_fix, n_chans, d_aided_ptr, d_peaks_out_ptr,
                               d_vel_ptr=None, d_peaks_in_ptr=None, d_aid_ptr=None, stride=16 * BLOCK_BYTES, aid_params=None, params=None,
                               sync=True):
        """gpsacq_aided_peaks_iq8_device: aided_peaks_device() on an 8-bit IQ capture."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._record(aid_params, AID_PARAMS_DTYPE)
        sr, sp = self._record(params, AIDED_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_peaks_iq8_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_fix_ptr, d_vel_ptr,
                                                                  ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr,
                                                                  d_peaks_in_ptr, int(n_fix), int(n_chans), ap, sp, d_aid_ptr, d_aided_ptr,
                                                                  d_peaks_out_ptr, 1 if sync else 0))

    def aided_iq8_last_ms(self):
        """Device milliseconds of the last aided *_iq8 call: (conversion or 0, k_aid_predict or 0, the search kernel)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_aided_iq8_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- coherent aided acquisition -----------------------------------------------------------
    def aided_coh_search(self, bits, aid, tasks=None, peaks_in=None, stride=BLOCK_BYTES, params=None, powers=False):
        """gpsacq_aided_coh_search: aided_search() with coherent sums of coh_ms segments, a hypothesis for the bit edge and fine
        Doppler hypotheses.  Returns (AIDED_COH_DTYPE, PEAK_DTYPE) in the shape of aid, and with powers=True also the powers,
        uint64 [n_tasks][2 K + 1][2 F + 1][M][2 W + 1].  params: aided_coh_params(), None for the defaults."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        if not isinstance(aid, np.ndarray) or aid.dtype != AID_DTYPE:
            raise TypeError("aid must be an AID_DTYPE array")
        ad = np.ascontiguousarray(aid)
        tptr = iptr = wptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != ad.size:
                raise ValueError("one task per prediction")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        if peaks_in is not None:
            if not isinstance(peaks_in, np.ndarray) or peaks_in.dtype != PEAK_DTYPE or peaks_in.size != ad.size:
                raise TypeError("peaks_in must be a PEAK_DTYPE array with one peak per prediction")
            pi = np.ascontiguousarray(peaks_in)
            iptr = pi.ctypes.data_as(ctypes.c_void_p)
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        prm = aided_coh_params() if sr is None else sr
        out = np.zeros(ad.shape, dtype=AIDED_COH_DTYPE)
        pk = np.zeros(ad.shape, dtype=PEAK_DTYPE)
        if powers:
            pw = np.zeros((ad.size, 2 * int(prm["dop_half"][0]) + 1, 2 * int(prm["fine_half"][0]) + 1, max(int(prm["coh_ms"][0]), 1),
                           2 * int(prm["code_half"][0]) + 1), dtype=np.uint64)
            wptr = pw.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aided_coh_search(self._h, buf.ctypes.data_as(ctypes.c_void_p), int(buf.size), int(stride), tptr,
                                                            ad.ctypes.data_as(ctypes.c_void_p), iptr, int(ad.size), sp,
                                                            out.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p), wptr))
        return (out, pk, pw) if powers else (out, pk)

    def aided_coh_search_device(self, d_bits_ptr, n_bytes, d_aid_ptr, n_tasks, d_aided_ptr, d_peaks_out_ptr, stride=BLOCK_BYTES, d_tasks_ptr=None,
                                d_peaks_in_ptr=None, d_powers_ptr=None, params=None, sync=True):
        """gpsacq_aided_coh_search_device: aided_search_device()'s arguments; the records are AIDED_COH_DTYPE."""
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_coh_search_device(self._h, d_bits_ptr, int(n_bytes), int(stride), d_tasks_ptr, d_aid_ptr,
                                                                   d_peaks_in_ptr, int(n_tasks), sp, d_aided_ptr, d_peaks_out_ptr, d_powers_ptr,
                                                                   1 if sync else 0))

    def aid_instant(self, fix, info, prior):
        """gpsacq_aid_instant: the coarse-time fixes (FIX_DTYPE [n_fix]) with the receive instant a prediction needs, from their
        COARSE_INFO_DTYPE records and the COARSE_PRIOR_DTYPE priors they were made from.  Returns FIX_DTYPE [n_fix]."""
        fx = np.ascontiguousarray(np.asarray(fix, dtype=FIX_DTYPE).ravel())
        nf = np.ascontiguousarray(np.asarray(info, dtype=COARSE_INFO_DTYPE).ravel())
        pr = np.ascontiguousarray(np.asarray(prior, dtype=COARSE_PRIOR_DTYPE).ravel())
        if nf.size != fx.size or pr.size != fx.size:
            raise ValueError("one coarse-time record and one prior per fix")
        out = np.zeros(fx.size, dtype=FIX_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aid_instant(self._h, p(fx), p(nf), p(pr), int(fx.size), p(out)))
        return out

    def aid_instant_device(self, d_fix_ptr, d_info_ptr, d_prior_ptr, n_fix, d_fix_out_ptr, sync=True):
        """gpsacq_aid_instant_device: device pointers; d_fix_out_ptr may be d_fix_ptr."""
        _check(self._lib, self._lib.gpsacq_aid_instant_device(self._h, d_fix_ptr, d_info_ptr, d_prior_ptr, int(n_fix), d_fix_out_ptr, 1 if sync else 0))

    def aided_coh_peaks_device(self, eph, d_fix_ptr, d_bits_ptr, n_bytes, d_tasks_ptr, n_fix, n_chans, d_aided_ptr, d_peaks_out_ptr, d_info_ptr=None,
                               d_prior_ptr=None, d_vel_ptr=None, d_peaks_in_ptr=None, d_fix_instant_ptr=None, d_aid_ptr=None, stride=BLOCK_BYTES,
                               aid_params=None, params=None, sync=True):
        """gpsacq_aided_coh_peaks_device: coarse-time fixes -> receive instants -> predictions -> coherent aided peaks in device
        memory, no host copy in between; d_info_ptr None skips the first step (the fixes are taken as they are); d_vel_ptr,
        d_peaks_in_ptr, d_fix_instant_ptr and d_aid_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._record(aid_params, AID_PARAMS_DTYPE)
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_coh_peaks_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_fix_ptr, d_info_ptr,
                                                                  d_prior_ptr, d_vel_ptr, d_bits_ptr, int(n_bytes), int(stride), d_tasks_ptr,
                                                                  d_peaks_in_ptr, int(n_fix), int(n_chans), ap, sp, d_fix_instant_ptr, d_aid_ptr,
                                                                  d_aided_ptr, d_peaks_out_ptr, 1 if sync else 0))

    def aided_coh_last_ms(self):
        """Device milliseconds of the last coherent aided call: (k_aid_instant or 0, k_aid_predict or 0, k_aided_coh or 0)."""
        t = [ctypes.c_float() for _ in range(3)]
        _check(self._lib, self._lib.gpsacq_aided_coh_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- coherent aided acquisition on an 8-bit IQ capture --------------------------------------
    def aided_coh_search_iq8(self, iq, inp, aid, tasks=None, peaks_in=None, stride=16 * BLOCK_BYTES, params=None, powers=False, n_samples=None):
        """gpsacq_aided_coh_search_iq8: aided_coh_search() on interleaved 8-bit I, Q bytes, with inp (Engine.iq8_input(...)) as given
        to search_iq8(): multi-bit segment sums against the measured floor where inp.multibit != 0, the 1-bit path on the converted
        capture in sign mode.  stride in BYTES (a multiple of 16, >= 80000); n_samples: the capture's length (None: all of iq).
        params: aided_coh_params_iq8() or aided_coh_params(), None for the defaults of gpsacq_aided_coh_default_params_iq8 (sign
        mode: gpsacq_aided_coh_default_params).  Returns (AIDED_COH_DTYPE, PEAK_DTYPE) in the shape of aid, and with powers=True also
        uint64 [n_tasks][2 K + 1][2 F + 1][M][2 W + 1]."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        n = buf.size // 2 if n_samples is None else int(n_samples)
        if not isinstance(aid, np.ndarray) or aid.dtype != AID_DTYPE:
            raise TypeError("aid must be an AID_DTYPE array")
        ad = np.ascontiguousarray(aid)
        tptr = iptr = wptr = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != ad.size:
                raise ValueError("one task per prediction")
            tptr = t.ctypes.data_as(ctypes.c_void_p)
        if peaks_in is not None:
            if not isinstance(peaks_in, np.ndarray) or peaks_in.dtype != PEAK_DTYPE or peaks_in.size != ad.size:
                raise TypeError("peaks_in must be a PEAK_DTYPE array with one peak per prediction")
            pi = np.ascontiguousarray(peaks_in)
            iptr = pi.ctypes.data_as(ctypes.c_void_p)
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        prm = aided_coh_params() if sr is None else sr  # the shape of the powers: the two defaults differ in ratio_min alone
        out = np.zeros(ad.shape, dtype=AIDED_COH_DTYPE)
        pk = np.zeros(ad.shape, dtype=PEAK_DTYPE)
        if powers:
            pw = np.zeros((ad.size, 2 * int(prm["dop_half"][0]) + 1, 2 * int(prm["fine_half"][0]) + 1, max(int(prm["coh_ms"][0]), 1),
                           2 * int(prm["code_half"][0]) + 1), dtype=np.uint64)
            wptr = pw.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_aided_coh_search_iq8(self._h, ctypes.byref(inp), buf.ctypes.data_as(ctypes.c_void_p), n, int(stride), tptr,
                                                                ad.ctypes.data_as(ctypes.c_void_p), iptr, int(ad.size), sp,
                                                                out.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p), wptr))
        return (out, pk, pw) if powers else (out, pk)

    def aided_coh_search_iq8_device(self, inp, d_iq_ptr, n_samples, d_aid_ptr, n_tasks, d_aided_ptr, d_peaks_out_ptr, stride=16 * BLOCK_BYTES,
                                    d_tasks_ptr=None, d_peaks_in_ptr=None, d_powers_ptr=None, params=None, sync=True):
        """gpsacq_aided_coh_search_iq8_device: aided_search_iq8_device()'s arguments; the records are AIDED_COH_DTYPE."""
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_coh_search_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr,
                                                                       d_aid_ptr, d_peaks_in_ptr, int(n_tasks), sp, d_aided_ptr, d_peaks_out_ptr,
                                                                       d_powers_ptr, 1 if sync else 0))

    def aided_coh_peaks_iq8_device(self, eph, d_fix_ptr, inp, d_iq_ptr, n_samples, d_tasks_ptr, n_fix, n_chans, d_aided_ptr, d_peaks_out_ptr,
                                   d_info_ptr=None, d_prior_ptr=None, d_vel_ptr=None, d_peaks_in_ptr=None, d_fix_instant_ptr=None, d_aid_ptr=None,
                                   stride=16 * BLOCK_BYTES, aid_params=None, params=None, sync=True):
        """gpsacq_aided_coh_peaks_iq8_device: aided_coh_peaks_device() on an 8-bit IQ capture."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ar, ap = self._record(aid_params, AID_PARAMS_DTYPE)
        sr, sp = self._record(params, AIDED_COH_PARAMS_DTYPE)
        _check(self._lib, self._lib.gpsacq_aided_coh_peaks_iq8_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_fix_ptr, d_info_ptr,
                                                                      d_prior_ptr, d_vel_ptr, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride),
                                                                      d_tasks_ptr, d_peaks_in_ptr, int(n_fix), int(n_chans), ap, sp, d_fix_instant_ptr,
                                                                      d_aid_ptr, d_aided_ptr, d_peaks_out_ptr, 1 if sync else 0))

    def aided_coh_iq8_last_ms(self):
        """Device milliseconds of the last coherent aided *_iq8 call: (conversion or 0, k_aid_instant or 0, k_aid_predict or 0, the
        search kernel)."""
        t = [ctypes.c_float() for _ in range(4)]
        _check(self._lib, self._lib.gpsacq_aided_coh_iq8_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- snapshot signal quality on an 8-bit IQ capture ---------------------------------------
    @staticmethod
    def _iq8_fine_tasks(iq, fine, tasks):
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        if not isinstance(fine, np.ndarray) or fine.dtype != FINE_DTYPE:
            raise TypeError("fine must be a FINE_DTYPE array")
        fn = np.ascontiguousarray(fine)
        t = None
        if tasks is not None:
            t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
            if t.shape[0] != fn.size:
                raise ValueError("one task per fine record")
        return buf, fn, t

    def snap_floor_iq8(self, iq, inp, fine, tasks=None, stride=16 * BLOCK_BYTES, n_samples=None):
        """gpsacq_snap_floor_iq8: the measured noise floor 2 * sum (v_i^2 + v_q^2) over the window of every fine record (FINE_DTYPE,
        as refine_iq8() returned them for these tasks with the same inp and stride); 0 where the record is not usable or not of this
        capture; 2 * spm * segments in sign mode.  Returns uint64 in the shape of fine."""
        buf, fn, t = self._iq8_fine_tasks(iq, fine, tasks)
        n = buf.size // 2 if n_samples is None else int(n_samples)
        out = np.zeros(fn.shape, dtype=np.uint64)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_snap_floor_iq8(self._h, ctypes.byref(inp), p(buf), n, int(stride), p(t), p(fn), int(fn.size), p(out)))
        return out

    def snap_floor_iq8_device(self, inp, d_iq_ptr, n_samples, d_fine_ptr, n_tasks, d_floor_ptr, stride=16 * BLOCK_BYTES, d_tasks_ptr=None, sync=True):
        """gpsacq_snap_floor_iq8_device: device pointers for the capture (16-byte aligned), the records, the tasks (None: the
        reference schedule) and the floors."""
        _check(self._lib, self._lib.gpsacq_snap_floor_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr, d_fine_ptr,
                                                                 int(n_tasks), d_floor_ptr, 1 if sync else 0))

    def snap_quality_iq8(self, iq, inp, fine, tasks=None, obs=None, stride=16 * BLOCK_BYTES, params=None, n_samples=None):
        """gpsacq_snap_quality_iq8: snap_quality() for the records of refine_iq8() (FINE_DTYPE [n_fix][n_chans]) against the floor
        measured on the capture's own bytes; params: snap_quality_params_iq8() (None: those in multi-bit mode, snap_quality_params()
        in sign mode).  Returns (None or a copy of obs with the weights set, info QUALITY_INFO_DTYPE [n_fix][n_chans])."""
        if not isinstance(fine, np.ndarray) or fine.ndim != 2:
            raise TypeError("fine must be a FINE_DTYPE array [n_fix][n_chans]")
        buf, fn, t = self._iq8_fine_tasks(iq, fine, tasks)
        n = buf.size // 2 if n_samples is None else int(n_samples)
        ob = None
        if obs is not None:
            if not isinstance(obs, np.ndarray) or obs.dtype != OBS_DTYPE or obs.shape != fn.shape:
                raise TypeError("obs must be an OBS_DTYPE array in the shape of fine")
            ob = np.array(obs, order="C")
        pr, pp = self._snap_quality_params(params)
        inf = np.zeros(fn.shape, dtype=QUALITY_INFO_DTYPE)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_snap_quality_iq8(self._h, ctypes.byref(inp), p(buf), n, int(stride), p(t), p(fn), int(fn.shape[0]),
                                                            int(fn.shape[1]), pp, p(ob), p(inf)))
        return ob, inf

    def snap_quality_iq8_device(self, inp, d_iq_ptr, n_samples, d_fine_ptr, n_fix, n_chans, d_info_ptr, d_obs_ptr=None, d_floor_ptr=None,
                                stride=16 * BLOCK_BYTES, d_tasks_ptr=None, params=None, sync=True):
        """gpsacq_snap_quality_iq8_device: the capture, the records, the info, the in-out observations (may be None) and the floors
        (may be None: engine scratch) in device memory."""
        pr, pp = self._snap_quality_params(params)
        _check(self._lib, self._lib.gpsacq_snap_quality_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr,
                                                                   d_fine_ptr, int(n_fix), int(n_chans), pp, d_obs_ptr, d_floor_ptr, d_info_ptr,
                                                                   1 if sync else 0))

    def coarse_fix_quality_iq8_device(self, eph, inp, d_iq_ptr, n_samples, d_tasks_ptr, d_peaks_ptr, n_fix, n_chans, d_prior_ptr, d_fix_ptr, d_info_ptr,
                                      d_fine_ptr=None, d_obs_ptr=None, d_floor_ptr=None, d_qinfo_ptr=None, d_obs_out_ptr=None, stride=16 * BLOCK_BYTES,
                                      refine_params=None, quality_params=None, params=None, sync=True):
        """gpsacq_coarse_fix_quality_iq8_device: coarse_fix_quality_device() on an 8-bit IQ capture -- refine, observations, measured
        floors, weights and fix on one stream; d_fine_ptr, d_obs_ptr, d_floor_ptr, d_qinfo_ptr and d_obs_out_ptr may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        rr, rp = self._refine_params(refine_params)
        qr, qp = self._snap_quality_params(quality_params)
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_quality_iq8_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), ctypes.byref(inp),
                                                                         d_iq_ptr, int(n_samples), int(stride), d_tasks_ptr, d_peaks_ptr, int(n_fix),
                                                                         int(n_chans), rp, qp, d_prior_ptr, cp, d_fine_ptr, d_obs_ptr, d_floor_ptr,
                                                                         d_qinfo_ptr, d_fix_ptr, d_info_ptr, d_obs_out_ptr, 1 if sync else 0))

    def snap_quality_iq8_last_ms(self):
        """Device milliseconds of the last snapshot-quality *_iq8 call: (k_iq_energy and k_snap_floor together or 0, the quality kernel or 0)."""
        t = [ctypes.c_float() for _ in range(2)]
        _check(self._lib, self._lib.gpsacq_snap_quality_iq8_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    def coarse_obs_device(self, d_peaks_ptr, n_fix, n_chans, d_obs_ptr, snr_min=THRESHOLD, sync=True):
        _check(self._lib, self._lib.gpsacq_coarse_obs_device(self._h, d_peaks_ptr, int(n_fix), int(n_chans), float(snr_min), d_obs_ptr,
                                                             1 if sync else 0))

    def coarse_fix_peaks_device(self, eph, d_peaks_ptr, n_fix, n_chans, d_prior_ptr, d_fix_ptr, d_info_ptr, d_obs_ptr=None, d_obs_out_ptr=None,
                                snr_min=THRESHOLD, params=None, sync=True):
        """gpsacq_coarse_fix_peaks_device: peaks -> observations -> coarse-time fixes in device memory, no host copy in between;
        d_obs_ptr (the code-phase observations) and d_obs_out_ptr (with their whole milliseconds) may be None."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        cr, cp = self._coarse_params(params)
        _check(self._lib, self._lib.gpsacq_coarse_fix_peaks_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_peaks_ptr, int(n_fix),
                                                                   int(n_chans), float(snr_min), d_prior_ptr, cp, d_obs_ptr, d_fix_ptr, d_info_ptr,
                                                                   d_obs_out_ptr, 1 if sync else 0))

    def coarse_last_ms(self):
        """Device milliseconds of the last coarse* calls: (k_coarse_obs or 0, k_coarse_fix or 0)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_coarse_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- observables ----------------------------------------------------------------------
    @staticmethod
    def _obs_arrays(n_epochs, chans, tags):
        ne = np.ascontiguousarray(np.asarray(n_epochs, dtype=np.int32).ravel())
        ch = np.ascontiguousarray(np.asarray(chans, dtype=TRACK_CHAN_DTYPE).ravel())
        tg = np.ascontiguousarray(np.asarray(tags, dtype=TIME_TAG_DTYPE).ravel())
        if not (ne.size == ch.size == tg.size):
            raise ValueError("n_epochs, chans and tags must hold one entry per channel")
        return ne, ch, tg

    def observables(self, records, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix):
        """gpsacq_observables: the uncorrected transmit time of every channel at the receive samples first_rx_sample + i * rx_step,
        i < n_fix.  records: TRACK_RECORD_DTYPE [n_chans][max_epochs] of ONE track() call, n_epochs its third result, chans the
        channels after it, tags a TIME_TAG_DTYPE array (time_tag).  Returns OBS_DTYPE [n_fix][n_chans], the layout fix() takes."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        if not isinstance(records, np.ndarray) or records.dtype != TRACK_RECORD_DTYPE or records.ndim != 2 or records.shape[0] != ne.size:
            raise TypeError("records must be a TRACK_RECORD_DTYPE array [n_chans][max_epochs]")
        rec = np.ascontiguousarray(records)
        out = np.zeros((int(n_fix), ne.size), dtype=OBS_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_observables(self._h, p(rec), int(rec.shape[1]), p(ne), p(ch), p(tg), int(ne.size), int(first_rx_sample),
                                                       int(rx_step), int(n_fix), p(out)))
        return out

    def observables_device(self, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_obs_ptr, sync=True):
        """gpsacq_observables_device: the records as track_device / track_iq8_device left them in device memory (row stride
        max_epochs), the observations [n_fix][n_chans] into device memory; n_epochs, chans and tags are host arrays."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_observables_device(self._h, d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg), int(ne.size),
                                                              int(first_rx_sample), int(rx_step), int(n_fix), d_obs_ptr, 1 if sync else 0))

    def fix_track_device(self, eph, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_fix_ptr,
                         d_obs_ptr=None, sync=True):
        """gpsacq_fix_track_device: observables_device, then fix_device on them, on the engine's stream with no host copy in
        between.  d_fix: FIX_DTYPE [n_fix] in device memory; d_obs_ptr None keeps the observations in engine scratch."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fix_track_device(self._h, p(ep), int(ep.size), d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg),
                                                            int(ne.size), int(first_rx_sample), int(rx_step), int(n_fix), d_obs_ptr, d_fix_ptr,
                                                            1 if sync else 0))

    def observables_last_ms(self):
        """Device milliseconds of the last observables* / fix_track_device call: (code-position kernel, observation kernel)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_observables_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- carrier observables, velocity ----------------------------------------------------
    @staticmethod
    def _rate_arrays(n_epochs, chans, nom_words):
        ne = np.ascontiguousarray(np.asarray(n_epochs, dtype=np.int32).ravel())
        ch = np.ascontiguousarray(np.asarray(chans, dtype=TRACK_CHAN_DTYPE).ravel())
        if nom_words is None:  # 1-bit and sign-mode channels: the word lo_nom holds
            nom_words = (ch["lo_nom"].view(np.uint64) >> np.uint64(32)).astype(np.uint32)
        nw = np.ascontiguousarray(np.asarray(nom_words, dtype=np.uint32).ravel())
        if not (ne.size == ch.size == nw.size):
            raise ValueError("n_epochs, chans and nom_words must hold one entry per channel")
        return ne, ch, nw

    def nominal_word_iq8(self, inp):
        """gpsacq_track_nominal_word_iq8: the carrier NCO word of zero Doppler of channels started with track_start_iq8 on the
        capture inp describes (multi-bit channels keep their START word in lo_nom, so the default of rate_observables is not
        theirs)."""
        w = ctypes.c_uint32()
        _check(self._lib, self._lib.gpsacq_track_nominal_word_iq8(self._h, ctypes.byref(inp), ctypes.byref(w)))
        return int(w.value)

    def rate_observables(self, records, n_epochs, chans, first_rx_sample, rx_step, n_fix, avg_samples, nom_words=None):
        """gpsacq_rate_observables: accumulated Doppler (adr, cycles * 2^32 from record 0) and Doppler (Hz, averaged over avg_samples
        samples centred on the instant) of every channel at the receive samples first_rx_sample + i * rx_step.  Arguments as
        observables() without the tags; nom_words None: the 1-bit rule, lo_nom >> 32 of chans.  Returns RATE_OBS_DTYPE
        [n_fix][n_chans], index-parallel to observables()."""
        ne, ch, nw = self._rate_arrays(n_epochs, chans, nom_words)
        if not isinstance(records, np.ndarray) or records.dtype != TRACK_RECORD_DTYPE or records.ndim != 2 or records.shape[0] != ne.size:
            raise TypeError("records must be a TRACK_RECORD_DTYPE array [n_chans][max_epochs]")
        rec = np.ascontiguousarray(records)
        out = np.zeros((int(n_fix), ne.size), dtype=RATE_OBS_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_rate_observables(self._h, p(rec), int(rec.shape[1]), p(ne), p(ch), p(nw), int(ne.size),
                                                            int(first_rx_sample), int(rx_step), int(n_fix), int(avg_samples), p(out)))
        return out

    def rate_observables_device(self, d_records_ptr, max_epochs, n_epochs, chans, first_rx_sample, rx_step, n_fix, avg_samples, d_rate_obs_ptr,
                                nom_words=None, sync=True):
        """gpsacq_rate_observables_device: records and rate observations in device memory, the rest host arrays."""
        ne, ch, nw = self._rate_arrays(n_epochs, chans, nom_words)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_rate_observables_device(self._h, d_records_ptr, int(max_epochs), p(ne), p(ch), p(nw), int(ne.size),
                                                                   int(first_rx_sample), int(rx_step), int(n_fix), int(avg_samples),
                                                                   d_rate_obs_ptr, 1 if sync else 0))

    def sat_rates(self, eph, obs):
        """gpsacq_sat_rates: ECEF velocity and clock drift (SAT_RATE_DTYPE, obs's shape) of every observation."""
        ep, ob = self._nav_arrays(eph, obs)
        out = np.zeros(ob.shape, dtype=SAT_RATE_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_sat_rates(self._h, p(ep), int(ep.size), p(ob), int(ob.size), p(out)))
        return out

    def sat_rates_device(self, eph, d_obs_ptr, n_obs, d_out_ptr, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        _check(self._lib, self._lib.gpsacq_sat_rates_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, int(n_obs),
                                                            d_out_ptr, 1 if sync else 0))

    def velocity(self, eph, obs, rate_obs, fixes):
        """gpsacq_vel_batch: receiver velocity and clock drift (VEL_DTYPE [n_fix]) from obs (OBS_DTYPE [n_fix][sats_per_fix]), the
        index-parallel rate_obs (RATE_OBS_DTYPE) and the fixes made from obs (FIX_DTYPE [n_fix])."""
        ep, ob = self._nav_arrays(eph, obs)
        if ob.ndim != 2:
            raise ValueError("obs must be [n_fix][sats_per_fix]")
        if not isinstance(rate_obs, np.ndarray) or rate_obs.dtype != RATE_OBS_DTYPE or rate_obs.shape != ob.shape:
            raise TypeError("rate_obs must be a RATE_OBS_DTYPE array of obs's shape")
        if not isinstance(fixes, np.ndarray) or fixes.dtype != FIX_DTYPE or fixes.shape != (ob.shape[0],):
            raise TypeError("fixes must be a FIX_DTYPE array [n_fix]")
        ro, fx = np.ascontiguousarray(rate_obs), np.ascontiguousarray(fixes)
        out = np.zeros(ob.shape[0], dtype=VEL_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_vel_batch(self._h, p(ep), int(ep.size), p(ob), p(ro), p(fx), int(ob.shape[0]), int(ob.shape[1]), p(out)))
        return out

    def velocity_device(self, eph, d_obs_ptr, d_rate_obs_ptr, d_fix_ptr, n_fix, sats_per_fix, d_out_ptr, sync=True):
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        _check(self._lib, self._lib.gpsacq_vel_batch_device(self._h, ep.ctypes.data_as(ctypes.c_void_p), int(ep.size), d_obs_ptr, d_rate_obs_ptr,
                                                            d_fix_ptr, int(n_fix), int(sats_per_fix), d_out_ptr, 1 if sync else 0))

    def pvt_track_device(self, eph, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, avg_samples, d_fix_ptr,
                         d_vel_ptr, d_obs_ptr=None, d_rate_obs_ptr=None, nom_words=None, sync=True):
        """gpsacq_pvt_track_device: fix_track_device extended by the rate observations and the velocities, all on the engine's
        stream.  d_fix: FIX_DTYPE [n_fix], d_vel: VEL_DTYPE [n_fix] in device memory; d_obs_ptr / d_rate_obs_ptr None keep the
        observations in engine scratch."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        _, _, nw = self._rate_arrays(n_epochs, chans, nom_words)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_pvt_track_device(self._h, p(ep), int(ep.size), d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg), p(nw),
                                                            int(ne.size), int(first_rx_sample), int(rx_step), int(n_fix), int(avg_samples),
                                                            d_obs_ptr, d_rate_obs_ptr, d_fix_ptr, d_vel_ptr, 1 if sync else 0))

    def velocity_last_ms(self):
        """Device milliseconds of the last rate_observables* / velocity* / pvt_track_device calls: (accumulation kernel, rate
        observation kernel, satellite-rate kernel, velocity kernel); a pair whose call has not been made reads 0."""
        t = [ctypes.c_float() for _ in range(4)]
        _check(self._lib, self._lib.gpsacq_velocity_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- carrier-smoothed observables -----------------------------------------------------
    @staticmethod
    def _smooth_params(params):
        if params is None:
            return None
        pr = np.ascontiguousarray(np.asarray(params, dtype=SMOOTH_PARAMS_DTYPE).ravel())
        if pr.size != 1:
            raise ValueError("params must be one SMOOTH_PARAMS_DTYPE record")
        return pr

    def smooth_observables(self, records, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, params=None, nom_words=None, info=True):
        """gpsacq_smooth_observables: observables() with the code position of every phase-locked instant replaced by its mean over
        a window of instants carried by the carrier (a box-window Hatch filter that restarts on loss of lock and on a jump of
        code-minus-carrier).  params: smooth_params() (None: the defaults); nom_words as in rate_observables().  Returns (obs
        OBS_DTYPE [n_fix][n_chans], info SMOOTH_INFO_DTYPE of the same shape), or obs alone with info=False."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        _, _, nw = self._rate_arrays(n_epochs, chans, nom_words)
        pr = self._smooth_params(params)
        if not isinstance(records, np.ndarray) or records.dtype != TRACK_RECORD_DTYPE or records.ndim != 2 or records.shape[0] != ne.size:
            raise TypeError("records must be a TRACK_RECORD_DTYPE array [n_chans][max_epochs]")
        rec = np.ascontiguousarray(records)
        out = np.zeros((int(n_fix), ne.size), dtype=OBS_DTYPE)
        inf = np.zeros((int(n_fix), ne.size), dtype=SMOOTH_INFO_DTYPE) if info else None
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_smooth_observables(self._h, p(rec), int(rec.shape[1]), p(ne), p(ch), p(tg), p(nw), int(ne.size),
                                                              int(first_rx_sample), int(rx_step), int(n_fix), p(pr), p(out), p(inf)))
        return (out, inf) if info else out

    def smooth_observables_device(self, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_obs_ptr,
                                  d_info_ptr=None, params=None, nom_words=None, sync=True):
        """gpsacq_smooth_observables_device: records, observations and info (may be None) in device memory, the rest host arrays."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        _, _, nw = self._rate_arrays(n_epochs, chans, nom_words)
        pr = self._smooth_params(params)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_smooth_observables_device(self._h, d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg), p(nw), int(ne.size),
                                                                     int(first_rx_sample), int(rx_step), int(n_fix), p(pr), d_obs_ptr, d_info_ptr,
                                                                     1 if sync else 0))

    def fix_smooth_track_device(self, eph, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_fix_ptr,
                                d_obs_ptr=None, d_info_ptr=None, params=None, nom_words=None, sync=True):
        """gpsacq_fix_smooth_track_device: smooth_observables_device, then fix_device on them, on the engine's stream with no host
        copy in between.  d_fix: FIX_DTYPE [n_fix] in device memory; d_obs_ptr / d_info_ptr None keep those in engine scratch."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        _, _, nw = self._rate_arrays(n_epochs, chans, nom_words)
        pr = self._smooth_params(params)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fix_smooth_track_device(self._h, p(ep), int(ep.size), d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg),
                                                                   p(nw), int(ne.size), int(first_rx_sample), int(rx_step), int(n_fix), p(pr),
                                                                   d_obs_ptr, d_info_ptr, d_fix_ptr, 1 if sync else 0))

    def smooth_last_ms(self):
        """Device milliseconds of the last smooth_observables* / fix_smooth_track_device call: (lock sums, code-minus-carrier, scan,
        output kernel); the first reads 0 when lock_epochs was 0."""
        t = [ctypes.c_float() for _ in range(4)]
        _check(self._lib, self._lib.gpsacq_smooth_last_ms(self._h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    # ---- signal quality per observation ---------------------------------------------------
    @staticmethod
    def _quality_params(params):
        if params is None:
            return None
        pr = np.ascontiguousarray(np.asarray(params, dtype=QUALITY_PARAMS_DTYPE).ravel())
        if pr.size != 1:
            raise ValueError("params must be one QUALITY_PARAMS_DTYPE record")
        return pr

    def quality(self, records, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, params=None, obs=None):
        """gpsacq_quality_observables: C/N0 (dB-Hz), phase lock and the weight of every channel at the receive samples
        first_rx_sample + i * rx_step, from the prompt sums of the records; arguments as observables().  params: quality_params()
        (None: the defaults).  Returns info, QUALITY_INFO_DTYPE [n_fix][n_chans]; with obs (OBS_DTYPE [n_fix][n_chans] made for the
        same instants by observables() or smooth_observables()) returns (a copy of obs with the weights set, info)."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        pr = self._quality_params(params)
        if not isinstance(records, np.ndarray) or records.dtype != TRACK_RECORD_DTYPE or records.ndim != 2 or records.shape[0] != ne.size:
            raise TypeError("records must be a TRACK_RECORD_DTYPE array [n_chans][max_epochs]")
        rec = np.ascontiguousarray(records)
        ob = None
        if obs is not None:
            if not isinstance(obs, np.ndarray) or obs.dtype != OBS_DTYPE or obs.shape != (int(n_fix), ne.size):
                raise TypeError("obs must be an OBS_DTYPE array [n_fix][n_chans]")
            ob = np.array(obs, order="C")
        inf = np.zeros((int(n_fix), ne.size), dtype=QUALITY_INFO_DTYPE)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_quality_observables(self._h, p(rec), int(rec.shape[1]), p(ne), p(ch), p(tg), int(ne.size),
                                                               int(first_rx_sample), int(rx_step), int(n_fix), p(pr), p(ob), p(inf)))
        return inf if obs is None else (ob, inf)

    def quality_device(self, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_info_ptr, d_obs_ptr=None,
                       params=None, sync=True):
        """gpsacq_quality_observables_device: records, info and the in-out observations (may be None) in device memory, the rest host
        arrays."""
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        pr = self._quality_params(params)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_quality_observables_device(self._h, d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg), int(ne.size),
                                                                      int(first_rx_sample), int(rx_step), int(n_fix), p(pr), d_obs_ptr, d_info_ptr,
                                                                      1 if sync else 0))

    def fix_quality_track_device(self, eph, d_records_ptr, max_epochs, n_epochs, chans, tags, first_rx_sample, rx_step, n_fix, d_fix_ptr,
                                 d_obs_ptr=None, d_info_ptr=None, quality_params=None, smooth_params=None, nom_words=None, sync=True):
        """gpsacq_fix_quality_track_device: observables_device (smooth_params None) or smooth_observables_device, then the quality
        weights, then fix_device, on the engine's stream with no host copy in between.  d_fix: FIX_DTYPE [n_fix] in device memory;
        d_obs_ptr / d_info_ptr None keep those in engine scratch; nom_words as in rate_observables(), read only when smoothing."""
        ep = np.ascontiguousarray(np.asarray(eph, dtype=EPHEMERIS_DTYPE).ravel())
        ne, ch, tg = self._obs_arrays(n_epochs, chans, tags)
        nw = None if smooth_params is None else self._rate_arrays(n_epochs, chans, nom_words)[2]
        qp, sp = self._quality_params(quality_params), self._smooth_params(smooth_params)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        _check(self._lib, self._lib.gpsacq_fix_quality_track_device(self._h, p(ep), int(ep.size), d_records_ptr, int(max_epochs), p(ne), p(ch), p(tg),
                                                                    p(nw), int(ne.size), int(first_rx_sample), int(rx_step), int(n_fix), p(sp), p(qp),
                                                                    d_obs_ptr, d_info_ptr, d_fix_ptr, 1 if sync else 0))

    def quality_last_ms(self):
        """Device milliseconds of the last quality* / fix_quality_track_device call: (prefix-sum kernel, output kernel)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_quality_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- tracking channels on an 8-bit IQ capture -----------------------------------------
    def iq8_power(self, iq, signed=False):
        """gpsacq_iq8_accumulate_power over a whole buffer: (mean of (I - off)^2, mean of (Q - off)^2), from exact integer sums."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        n = buf.size // 2
        pw = (ctypes.c_uint64 * 2)(0, 0)
        _check(self._lib, self._lib.gpsacq_iq8_accumulate_power(self._h, buf.ctypes.data_as(ctypes.c_void_p), n, 1 if signed else 0, pw))
        return pw[0] / n, pw[1] / n

    def iq8_rms(self, iq, inp):
        """RMS of the samples v_i, v_q a multi-bit channel sees (offset and, with inp.remove_dc, the rounded mean removed):
        what track_params_iq8 wants."""
        pi, pq = self.iq8_power(iq, signed=inp.format == 1)
        dci, dcq = (float(np.rint(inp.mean_i)), float(np.rint(inp.mean_q))) if inp.remove_dc else (0.0, 0.0)
        # E[(a - dc)^2] = E[a^2] - 2 dc E[a] + dc^2, E[a] = the capture's mean
        return float(np.sqrt(max(0.0, (pi + pq - 2 * dci * inp.mean_i - 2 * dcq * inp.mean_q + dci * dci + dcq * dcq) / 2)))

    def track_params_iq8(self, sample_rms, **overrides):
        """gpsacq_track_default_params_iq8: the defaults rescaled to the capture's sample RMS, any field overridden by name."""
        p = TrackParams()
        _check(self._lib, self._lib.gpsacq_track_default_params_iq8(self._h, float(sample_rms), ctypes.byref(p)))
        for k, v in overrides.items():
            if k not in dict(TrackParams._fields_):
                raise KeyError(f"no tracking parameter {k!r}")
            setattr(p, k, int(v))
        return p

    def track_start_iq8(self, inp, prn, peak, block_first_sample, params=None):
        """gpsacq_track_start_iq8: a channel (TRACK_CHAN_DTYPE, shape (1,)) from a hit of search_iq8 on the capture inp describes;
        in multi-bit mode its carrier NCO runs at the satellite's frequency in the raw capture (negative ones wrap)."""
        p = self._params(params)
        pk = np.zeros(1, dtype=PEAK_DTYPE)
        pk[0] = peak
        ch = np.zeros(1, dtype=TRACK_CHAN_DTYPE)
        _check(self._lib, self._lib.gpsacq_track_start_iq8(self._h, ctypes.byref(inp), int(prn), pk.ctypes.data_as(ctypes.c_void_p),
                                                           int(block_first_sample), ctypes.byref(p), ch.ctypes.data_as(ctypes.c_void_p)))
        return ch

    def track_iq8(self, iq, inp, chans, first_sample=0, max_epochs=None, records=False, params=None):
        """gpsacq_track_iq8 over a window of interleaved 8-bit I,Q bytes (samples first_sample ..).  inp: Engine.iq8_input(...);
        multibit 0 runs the 1-bit channels on the converted window, else the multi-bit complex channels (params required: see
        track_params_iq8).  chans updated in place.  Returns (prompt, records or None, n_epochs) as track()."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        if chans.dtype != TRACK_CHAN_DTYPE or not chans.flags.c_contiguous:
            raise TypeError("chans must be a contiguous TRACK_CHAN_DTYPE array")
        n_samples = buf.size // 2
        if max_epochs is None:
            max_epochs = int(n_samples // max(1, self.num_lags // 2)) + 1
        if params is None and inp.multibit:
            raise ValueError("multi-bit channels need params (track_params_iq8)")
        p = self._params(params)
        n = chans.size
        prompt = np.zeros((n, max_epochs, 2), dtype=np.int32)
        rec = np.zeros((n, max_epochs), dtype=TRACK_RECORD_DTYPE) if records else None
        ne = np.zeros(n, dtype=np.int32)
        _check(self._lib, self._lib.gpsacq_track_iq8(self._h, ctypes.byref(inp), buf.ctypes.data_as(ctypes.c_void_p), int(n_samples), int(first_sample),
                                                     chans.ctypes.data_as(ctypes.c_void_p), int(n), ctypes.byref(p),
                                                     prompt.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p) if records else None,
                                                     int(max_epochs), ne.ctypes.data_as(ctypes.c_void_p)))
        return prompt, rec, ne

    def track_iq8_device(self, d_iq_ptr, n_samples, inp, chans, first_sample=0, max_epochs=0, d_prompt_ptr=None, d_records_ptr=None, params=None):
        """gpsacq_track_iq8_device: the capture window (16-byte aligned) and the outputs in device memory.  Returns n_epochs."""
        if params is None and inp.multibit:
            raise ValueError("multi-bit channels need params (track_params_iq8)")
        p = self._params(params)
        ne = np.zeros(chans.size, dtype=np.int32)
        _check(self._lib, self._lib.gpsacq_track_iq8_device(self._h, ctypes.byref(inp), d_iq_ptr, int(n_samples), int(first_sample),
                                                            chans.ctypes.data_as(ctypes.c_void_p), int(chans.size), ctypes.byref(p), d_prompt_ptr,
                                                            d_records_ptr, int(max_epochs), ne.ctypes.data_as(ctypes.c_void_p)))
        return ne

    def track_iq8_last_ms(self):
        """Device milliseconds of the last track_iq8* call: (8-bit -> 1-bit conversion, channel kernel)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self._lib, self._lib.gpsacq_track_iq8_last_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def generate_iq8(self, n_samples, sats=(), if_hz=0.0, scale=16.0, signed=True, noise_sigma=1.0, seed=1, first_sample=0, nav=None):
        """Synthetic 8-bit complex capture at residual IF if_hz made on the device (gpsacq_generate_iq8_range): generate()'s law with a
        complex carrier and complex noise, times scale, rounded and clamped.  Returns int8 (signed) or uint8 interleaved I,Q."""
        out = np.zeros(2 * int(n_samples), dtype=np.uint8)
        nv = None if nav is None else np.ascontiguousarray(np.asarray(nav, dtype=np.int8).reshape(len(sats), -1))
        _check(self._lib, self._lib.gpsacq_generate_iq8_range(self._h, out.ctypes.data_as(ctypes.c_void_p), int(n_samples), int(first_sample),
                                                              1 if signed else 0, float(if_hz), float(scale), self._sats(sats), len(sats),
                                                              nv.ctypes.data_as(ctypes.c_void_p) if nv is not None else None,
                                                              int(nv.shape[1]) if nv is not None else 0, float(noise_sigma), int(seed)))
        return out.view(np.int8) if signed else out

    def generate_iq8_device(self, d_iq_ptr, n_samples, sats=(), if_hz=0.0, scale=16.0, signed=True, noise_sigma=1.0, seed=1, first_sample=0,
                            nav=None, sync=True):
        nv = None if nav is None else np.ascontiguousarray(np.asarray(nav, dtype=np.int8).reshape(len(sats), -1))
        _check(self._lib, self._lib.gpsacq_generate_iq8_range_device(self._h, d_iq_ptr, int(n_samples), int(first_sample), 1 if signed else 0,
                                                                     float(if_hz), float(scale), self._sats(sats), len(sats),
                                                                     nv.ctypes.data_as(ctypes.c_void_p) if nv is not None else None,
                                                                     int(nv.shape[1]) if nv is not None else 0, float(noise_sigma), int(seed),
                                                                     1 if sync else 0))

    def generate_sig(self, prn, data_bits):
        """gps_sig_gen.m's signal on the device: PRN `prn`, navigation bits +-1 (20 code periods each), 8.184 Msps,
        IF 2.046 MHz, raised-cosine BPSK, 1 bit per sample.  Returns the packed bytes."""
        d = np.ascontiguousarray(np.asarray(data_bits, dtype=np.int8))
        n = self._lib.gpsacq_sig_bytes(int(d.size))
        out = np.zeros(n, dtype=np.uint8)
        _check(self._lib, self._lib.gpsacq_generate_sig(self._h, int(prn), d.ctypes.data_as(ctypes.c_void_p), int(d.size),
                                                        out.ctypes.data_as(ctypes.c_void_p), n))
        return out

    def generate_sig_tx(self, prn, data_bits, n_repeat=5, first_sample=0, n_samples=None):
        """gps_sig_gen.m:21-30 on the device: complex samples [first_sample, first_sample + n_samples) of the script's HackRF
        transmit file (int8 I = round(50 x), Q = 0, interleaved).  Returns an int8 array of 2 * n_samples."""
        d = np.ascontiguousarray(np.asarray(data_bits, dtype=np.int8))
        total = int(self._lib.gpsacq_sig_tx_samples(int(d.size), int(n_repeat)))
        n = total - int(first_sample) if n_samples is None else int(n_samples)
        out = np.zeros(2 * n, dtype=np.int8)
        _check(self._lib, self._lib.gpsacq_generate_sig_tx(self._h, int(prn), d.ctypes.data_as(ctypes.c_void_p), int(d.size), int(n_repeat),
                                                           int(first_sample), n, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def generate_device(self, d_bits_ptr, n_bytes, sats=(), noise_sigma=1.0, seed=1, sync=True, first_sample=0, nav=None):
        """generate() into device memory; nav as there (gpsacq_generate_nav_range_device)."""
        if nav is None:
            _check(self._lib, self._lib.gpsacq_generate_range_device(self._h, d_bits_ptr, int(n_bytes), int(first_sample), self._sats(sats),
                                                                     len(sats), float(noise_sigma), int(seed), 1 if sync else 0))
            return
        nv = np.ascontiguousarray(np.asarray(nav, dtype=np.int8).reshape(len(sats), -1))
        _check(self._lib, self._lib.gpsacq_generate_nav_range_device(self._h, d_bits_ptr, int(n_bytes), int(first_sample), self._sats(sats),
                                                                     len(sats), nv.ctypes.data_as(ctypes.c_void_p), int(nv.shape[1]),
                                                                     float(noise_sigma), int(seed), 1 if sync else 0))

    # ---- 8-bit IQ ingestion --------------------------------------------------------------
    def iq8_to_bits(self, iq, signed=False, remove_dc=True, mix_hz=0.0, fs=0.0):
        """proc_rtl_bin_for_gps.m / proc_hackrf_bin_for_gps.m on the device: interleaved 8-bit I,Q
        (uint8 offset-128 rtl-sdr, or int8 HackRF with signed=True) -> packed 1-bit real-IF bytes."""
        buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
        n = buf.size // 2
        out = np.zeros((n + 7) // 8, dtype=np.uint8)
        _check(self._lib, self._lib.gpsacq_iq8_to_bits(self._h, buf.ctypes.data_as(ctypes.c_void_p), n, 1 if signed else 0,
                                                       1 if remove_dc else 0, float(mix_hz), float(fs),
                                                       out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # ---- parity probes -------------------------------------------------------------------
    def sample_spectrum(self, block):
        b = np.ascontiguousarray(np.frombuffer(block, dtype=np.uint8)[:BLOCK_BYTES])
        if b.size < BLOCK_BYTES:
            raise ValueError("need 5120 bytes")
        out = np.zeros(2 * FFT_LEN, dtype=np.float32)
        _check(self._lib, self._lib.gpsacq_sample_spectrum(self._h, b.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)))
        return out.view(np.complex64)

    def code_spectrum(self, sv):
        out = np.zeros(2 * FFT_LEN, dtype=np.float32)
        _check(self._lib, self._lib.gpsacq_code_spectrum(self._h, int(sv), out.ctypes.data_as(ctypes.c_void_p)))
        return out.view(np.complex64)


class MultiEngine:
    """gpsacq_multi_*: one capture's PRN x Doppler grid cut into Doppler slabs over several GPUs of this process, the
    per-task peaks merged by one RCCL all-reduce(MAX) of packed keys (include/gpsacq.h)."""

    def __init__(self, fc, fs, max_fo, devices=(0,)):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        prm = Params(float(fc), float(fs), float(max_fo), 0, 0)
        dev = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        _check(self._lib, self._lib.gpsacq_multi_create(ctypes.byref(prm), dev, len(devices), ctypes.byref(self._h)))
        self._refresh()

    def _refresh(self):
        info, n = Info(), ctypes.c_int32()
        _check(self._lib, self._lib.gpsacq_multi_get_info(self._h, ctypes.byref(info), ctypes.byref(n)))
        self.n_devices = n.value
        self.num_doppler_total = info.num_doppler_total
        self.kmax = -info.first_doppler_total
        self.doppler_step_hz = info.doppler_step_hz

    def set_doppler_step(self, step_hz):
        _check(self._lib, self._lib.gpsacq_multi_set_doppler_step(self._h, float(step_hz)))
        self._refresh()

    def search_grid(self, bits, tasks, stride=BLOCK_BYTES):
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        n_blocks = (buf.size - min(stride, BLOCK_BYTES)) // stride + 1
        t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 2))
        peaks = np.zeros(t.shape[0], dtype=PEAK_DTYPE)
        _check(self._lib, self._lib.gpsacq_multi_search_grid(self._h, buf.ctypes.data_as(ctypes.c_void_p), n_blocks, stride,
                                                             t.ctypes.data_as(ctypes.c_void_p), t.shape[0], peaks.ctypes.data_as(ctypes.c_void_p)))
        return peaks

    def search_blocks(self, bits, stride=BLOCK_BYTES):
        """gpsacq_multi_search_blocks: whole runs of the reference schedule split over the devices.  Returns
        (peaks[n_runs * 32] in file order, best[32] = per-PRN best after the all-reduce)."""
        buf = np.ascontiguousarray(np.frombuffer(bits, dtype=np.uint8) if not isinstance(bits, np.ndarray) else bits.view(np.uint8))
        n_blocks = (buf.size - BLOCK_BYTES) // stride + 1 if buf.size >= BLOCK_BYTES else 0
        n_runs = n_blocks // NUM_SATS
        if n_runs <= 0:
            raise ValueError("capture shorter than one run of 32 blocks")
        peaks = np.zeros(n_runs * NUM_SATS, dtype=PEAK_DTYPE)
        best = np.zeros(NUM_SATS, dtype=PEAK_DTYPE)
        _check(self._lib, self._lib.gpsacq_multi_search_blocks(self._h, buf.ctypes.data_as(ctypes.c_void_p), n_runs, stride,
                                                               peaks.ctypes.data_as(ctypes.c_void_p), best.ctypes.data_as(ctypes.c_void_p)))
        return peaks, best

    def last_call_ms(self):
        """Host-side times of the last search_* call: {"enqueue_ms", "total_ms", "rccl_allreduces"} (gpsacq_multi_last_call_ms)."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _check(self._lib, self._lib.gpsacq_multi_last_call_ms(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"enqueue_ms": a.value, "total_ms": b.value, "rccl_allreduces": c.value}

    def close(self):
        if self._h:
            self._lib.gpsacq_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_report(peaks, first_run=0):
    """SearchTask()'s per-run report (c/search_offline.cpp:264-287) for peaks of whole runs
    (32 consecutive tasks per run, reference schedule)."""
    out = []
    n_runs = len(peaks) // NUM_SATS
    for r in range(n_runs):
        pk = peaks[r * NUM_SATS:(r + 1) * NUM_SATS]
        hits = [sv for sv in range(NUM_SATS) if not (pk["snr"][sv] < THRESHOLD)]
        run = first_run + r
        out.append("%2d satellite: " % run + "".join("%5d " % sv for sv in hits) + "\n")
        out.append("%2d SNR(>=25): " % run + "".join("%5.1f " % pk["snr"][sv] for sv in hits) + "\n")
        out.append("%2d  lo_shift: " % run + "".join("%5d " % pk["lo_shift"][sv] for sv in hits) + "\n")
        out.append("%2d  ca_shift: " % run + "".join("%5d " % pk["ca_shift"][sv] for sv in hits) + "\n")
        out.append("".join("%2.0f " % pk["snr"][sv] for sv in range(NUM_SATS)) + "\n\n")
    return "".join(out)
