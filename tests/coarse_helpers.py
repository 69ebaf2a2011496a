"""Cases of the coarse-time fix tests (tests/test_coarse.py on the CPU, tests/test_gpu_coarse.py on the GPU): code phases from the
truth maker of tests/nav_ref.py, and priors a given distance and time away from it."""
import numpy as np

import nav_ref
from nav_helpers import truth_obs


def times(n, first=0):
    """n receive times: whole milliseconds `first` .. and a sub-millisecond part of their own each"""
    k = np.arange(first, first + n)
    return (k * 7).astype(np.int64), (0.137e-3 + k * 0.0131e-3) % 1e-3


def phases(geo, sel, ref_ms, t_rx):
    """What a search gives of geo's receiver at ref_ms[k] + t_rx[k]: OBS_DTYPE [n][len(sel)] with tx_frac only (tx_ms = 0, eph =
    satellite index, valid = 1, weight = 1) -- and the whole milliseconds it does not give, int64 [n][len(sel)]"""
    full = truth_obs(geo, ref_ms, t_rx)[:, sel]
    ob = full.copy()
    ob["tx_ms"] = 0
    return ob, full["tx_ms"].astype(np.int64)


def priors(geo, ref_ms, seed, km=30.0, secs=30.0):
    """COARSE_PRIOR_DTYPE [n]: km kilometres from geo's receiver in a random direction, secs seconds from ref_ms, early and late
    in turn"""
    import gpsacq
    rng = np.random.default_rng(seed)
    n = len(ref_ms)
    d = rng.normal(size=(n, 3))
    d *= km * 1e3 / np.linalg.norm(d, axis=1)[:, None]
    sign = np.where((np.arange(n) + seed) % 2 == 0, 1, -1)
    return gpsacq.coarse_prior(geo["rx"] + d, (np.asarray(ref_ms, np.int64) + sign * int(secs * 1000)) % nav_ref.WEEK_MS)


def truth_s(ref, tx_ms, prior):
    """The fifth unknown the truth has for each row of a reference result: the transmit time of the reference column less t0 + T_r,
    a whole number of milliseconds because T_r carries the truth's own fraction.  Seconds, (n,)."""
    r = np.array([x["ref"] for x in ref])
    N = np.array([x["N"][x["ref"]] for x in ref])
    return (nav_ref.fold_ms(tx_ms[np.arange(len(ref)), r] - prior["rx_ms"].astype(np.int64)) - N) * 1e-3


def rx_error(rx_ms, rx_frac, ref_ms, t_rx):
    return nav_ref.fold_ms(np.asarray(rx_ms, np.int64) - ref_ms) * 1e-3 + (np.asarray(rx_frac) - t_rx)


L1_HZ = 1575.42e6


def block_times(ref_ms, ref_frac, n_blocks, samples_per_block, fs):
    """receive times of the first samples of n_blocks blocks, the first at (ref_ms, ref_frac): (ms of week (n,), frac (n,))"""
    return nav_ref.split_time(ref_ms, ref_frac + np.arange(n_blocks) * (samples_per_block / fs))


def synth_sats(geo, sel, ref_ms, ref_frac, first_sample, fs, amplitude):
    """The generator's satellites (gpsacq_sat tuples) for geo's receiver: sample first_sample of the stream is received at
    (ref_ms, ref_frac); each satellite runs at the Doppler it has there, and its code shows the truth maker's transmit time at
    that sample.  Returns (sats, doppler_hz (n,))."""
    sats, dops = [], []
    for j, k in enumerate(sel):
        eph = geo["ephs"][k]
        t = nav_ref.truth_tx(eph, geo["rx"], ref_ms, np.array([ref_frac - 0.5, ref_frac, ref_frac + 0.5]))
        dop = L1_HZ * ((t[2] - t[0]) - 1.0)
        cp = (t[1] + 0.1) * fs / (1.0 + dop / L1_HZ) - first_sample  # 100 ms on top: a whole number of code periods, and positive
        sats.append((int(eph["prn"]), amplitude, float(dop), float(cp), 0.1 + 0.17 * j))
        dops.append(dop)
    return sats, np.array(dops)
