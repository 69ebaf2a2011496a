"""Cold snapshot fixes on the GPU (gpsacq_fine_doppler*, gpsacq_rate_obs_fine*, gpsacq_doppler_fix_batch*, gpsacq_cold_fix_device)
against tests/dop_ref.py, the numpy restatement of "Cold snapshot fixes: fine Doppler and a Doppler-only position solver" of
include/gpsacq.h.

Every integer field of a fine-Doppler record (flags, segments, lo_rate, ca_rate, re, im, mag, power) must equal the reference;
df_hz and doppler_hz may differ by dop_ref.DF_TOL = 1e-9 Hz and coherence by 1e-12 (two correctly rounded atan2s differ by a few
ulp of pi, under 1e-12 Hz after the division).  Status, n_used, iterations and flags of a Doppler fix must be equal, places may
differ by 1e-3 m and the drift by 1e-13 (two Newton runs with a stop at 1e-3 m from identical starts, in fp64).
fs = 5.456 MHz, fc = 4.092 MHz; the bits come from Engine.generate.  Each test prints what it measured before it asserts
(pytest -s)."""
import ctypes

import numpy as np
import pytest

import dop_ref
import nav_ref
from coarse_helpers import block_times, priors, synth_sats
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu

FS, FC, SPM = 5.456e6, 4.092e6, 5456


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def capture(eng):
    """four blocks, three satellites at amplitude 0.3 (PRN 1 and 32 among them), made once"""
    sats = [(1, 0.3, 1234.0, 100.25, 0.1), (32, 0.3, -2900.0, 4000.7, 0.4), (17, 0.3, 310.0, 2727.4, 0.7)]
    bits = eng.generate(4 * 5120, sats, noise_sigma=1.0, seed=5)
    bits.setflags(write=False)
    return bits


def hand_peaks(eng, n, seed):
    """n hand-made hits that reach the edges whatever a search would find: ca_shift in {0, 1, 2727, 5455} x lo_shift in {-dmax, 0,
    +dmax} x PRN 1 and 32 (24 combinations, cycled), blocks 0 and 1"""
    import gpsacq
    combos = [(ca, lo, prn) for ca in (0, 1, 2727, SPM - 1) for lo in (-eng.dmax, 0, eng.dmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    pk = np.zeros(n, gpsacq.PEAK_DTYPE)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        pk[t] = (30.0 + t, lo, ca, 1.0)
        tasks[t] = (t % 2, prn)
    return tasks, pk


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


# ---- 1. records against the reference ------------------------------------------------------------------------------------------
CASES = [(b, s, 33) for b in (1, 2, 3) for s in (5000, 5003)] + [(2, 5003, 1), (2, 5000, 5)]


@pytest.mark.parametrize("blocks,stride,n_tasks", CASES)
def test_records_against_the_reference(eng, capture, blocks, stride, n_tasks):
    """7, 14 and 21 segments: fewer than two per wave, the four waves uneven, and every wave with five or more"""
    import gpsacq
    tasks, pk = hand_peaks(eng, n_tasks, seed=blocks * 100 + stride)
    got = eng.fine_doppler(capture, pk, tasks=tasks, stride=stride, params=gpsacq.dopfine_params(blocks=blocks))
    ref = dop_ref.fine_doppler(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=blocks)
    worst = dop_ref.same(got, ref, "blocks %d stride %d" % (blocks, stride))
    print("blocks %d, stride %d, %d tasks: coherence within %.3g, df_hz within %.3g Hz, doppler_hz within %.3g Hz" % (blocks, stride, n_tasks, *worst))
    assert (got["flags"] == 0).all() and (got["segments"] == blocks * 40000 // SPM).all() and (got["mag"] > 0).all()
    if n_tasks == 33:
        assert set(pk["ca_shift"].tolist()) == {0, 1, 2727, SPM - 1} and set(pk["lo_shift"].tolist()) == {-eng.dmax, 0, eng.dmax}


def test_zero_to_five_segments(eng, capture):
    """a capture cut so that the window of block 0 holds 0, 1, 2, 3, 4 and 5 segments, the last sample of the last one the last of
    the capture where the byte count allows"""
    import gpsacq
    tasks, pk = hand_peaks(eng, 4, seed=7)
    tasks[:, 0] = 0
    for k in range(6):
        n_bytes = max((k * SPM + 7) // 8, 600)
        got = eng.fine_doppler(capture[:n_bytes], pk, tasks=tasks, params=gpsacq.dopfine_params(blocks=1, min_segments=3))
        ref = dop_ref.fine_doppler(capture, 5120, tasks.tolist(), pk, SPM, FC, FS, blocks=1, min_segments=3, n_bytes=n_bytes)
        dop_ref.same(got, ref, "%d segments" % k)
        want = dop_ref.SHORT | (dop_ref.FEW if k < 3 else 0) | (dop_ref.NO_POWER if k < 2 else 0)
        assert (got["segments"] == k).all() and (got["flags"] == want).all(), (k, got["flags"])
        assert ((got["power"] > 0) == (k > 0)).all() and ((got["mag"] > 0) == (k > 1)).all()


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------
def test_edges(eng, capture):
    import gpsacq
    import torch
    n_bytes, stride = 15000 + 7 * 682, 5000  # the window of a task of block 3 ends with the capture, in the middle of a 32-bit word
    dmax = eng.dmax
    rows = [(1, 0, 40.0, 3, 100),      # 0: the whole window of 21 segments
            (3, 0, 40.0, -dmax, 0),    # 1: SHORT, its last segment ends with the capture
            (2, 31, 40.0, dmax, 5455),  # 2: SHORT, 14 segments and a tail
            (3, 31, 40.0, 0, 2727),    # 3: SHORT
            (4, 0, 40.0, 0, 7),        # 4: the block starts beyond the capture
            (0, 0, 24.5, 0, 7),        # 5: below snr_min
            (0, 0, 40.0, 0, -1),       # 6
            (0, 0, 40.0, 0, SPM),      # 7
            (0, 32, 40.0, 0, 7),       # 8: a task list with prn = 32
            (-1, 0, 40.0, 0, 7),       # 9
            (0, 5, 40.0, 1, 1),        # 10: a PRN that is not in the capture: still a record
            (0, 0, 40.0, 40000, 7),    # 11: fc + lo_dop beyond fs
            (0, 0, float("nan"), 0, 7)]  # 12: not snr >= snr_min
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    pk = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    for t, r in enumerate(rows):
        pk[t] = (r[2], r[3], r[4], 1.0)
    n = len(rows)
    prm = gpsacq.dopfine_params(blocks=3, min_segments=8)
    ref = dop_ref.fine_doppler(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=3, min_segments=8, n_bytes=n_bytes)
    fit = 3 * 40000 // SPM
    assert [r["flags"] for r in ref] == [0, 2 | 8, 2, 2 | 8, 1, 1, 1, 1, 1, 1, 0, 1, 1] and [r["segments"] for r in ref][:4] == [fit, 7, 14, 7]
    host = eng.fine_doppler(capture[:n_bytes], pk, tasks=tasks, stride=stride, params=prm)
    worst = dop_ref.same(host, ref, "host form")
    for t in (4, 5, 6, 7, 8, 9, 11, 12):
        assert host[t].tobytes() == np.int32(1).tobytes() + bytes(68), t
    # the device form at an odd address, sentinel bytes of either kind behind the capture, poison behind the records
    d_tasks, d_pk = dev(tasks), dev(pk)
    outs = []
    for sentinel in (0x00, 0xFF):
        buf = np.full(1 + n_bytes + 67, sentinel, np.uint8)
        buf[1:1 + n_bytes] = capture[:n_bytes]
        d_bits = dev(buf)
        d_out = fill(n * 72 + 72)
        torch.cuda.synchronize()
        eng.fine_doppler_device(d_bits.data_ptr() + 1, n_bytes, d_pk.data_ptr(), n, d_out.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                                params=prm, sync=True)
        back = d_out.cpu().numpy()
        assert (back[n * 72:] == 0xA5).all()
        outs.append(back[:n * 72].tobytes())
    assert outs[0] == host.tobytes() and outs[1] == host.tobytes()
    ms = eng.doppler_last_ms()
    print("edges: coherence within %.3g, df_hz within %.3g Hz, doppler_hz within %.3g Hz; k_fine_dop %.4f ms for %d tasks" % (*worst, ms[0], n))
    assert ms[0] > 0
    # the reference schedule: tasks == NULL is (block t, PRN t % 32)
    sched = eng.fine_doppler(capture[:n_bytes], pk[:4], stride=stride, params=prm)
    dop_ref.same(sched, dop_ref.fine_doppler(capture, stride, None, pk[:4], SPM, FC, FS, blocks=3, min_segments=8, n_bytes=n_bytes), "schedule")
    # the coherence gate just below and just above a record's own coherence
    own = float(host["coherence"][0])
    assert 0 < own < 1
    at = eng.fine_doppler(capture[:n_bytes], pk[:1], tasks=tasks[:1], stride=stride, params=gpsacq.dopfine_params(blocks=3, coherence_min=own))
    above = eng.fine_doppler(capture[:n_bytes], pk[:1], tasks=tasks[:1], stride=stride,
                             params=gpsacq.dopfine_params(blocks=3, coherence_min=np.nextafter(own, 1.0)))
    assert at["flags"][0] == 0 and above["flags"][0] == dop_ref.WEAK and above["doppler_hz"][0] == host["doppler_hz"][0]
    # rate observations of these records: usable needs none of NO_HIT, NO_POWER, FEW, WEAK, and the peak its snr
    ro = eng.rate_obs_fine(pk.reshape(-1, 1), host.reshape(-1, 1), snr_min=25.0)[:, 0]  # thirteen fixes of one channel
    valid, dh, w = (v[:, 0] for v in dop_ref.rate_obs_fine(pk.reshape(-1, 1), host.reshape(-1, 1), 25.0))
    assert ro["valid"].tolist() == valid.astype(int).tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    for t in range(n):
        if ro["valid"][t]:
            assert ro["doppler_hz"][t] == host["doppler_hz"][t] == dh[t] and w[t] == 1.0 and ro["weight"][t] == 1.0 and ro["adr"][t] == 0 and ro["reserved"][t] == 0
        else:
            assert ro[t].tobytes() == bytes(32), t
    weak = host.copy()
    weak["flags"][0] |= dop_ref.WEAK
    weak["doppler_hz"][2] = np.inf
    ro2 = eng.rate_obs_fine(pk.reshape(-1, 1), weak.reshape(-1, 1), snr_min=45.0)[:, 0]
    assert ro2["valid"].tolist() == [0] * n and not ro2.view(np.uint8).any()
    d_host, d_ro = dev(host), fill(n * 32 + 32)
    torch.cuda.synchronize()
    eng.rate_obs_fine_device(d_pk.data_ptr(), d_host.data_ptr(), n, 1, d_ro.data_ptr(), snr_min=25.0, sync=True)
    back = d_ro.cpu().numpy()
    assert back[:n * 32].tobytes() == ro.tobytes() and (back[n * 32:] == 0xA5).all()
    # argument errors return 1, launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out = np.full(n, 0, gpsacq.DOPFINE_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    cap = np.ascontiguousarray(capture[:n_bytes])

    def bad_params(**kw):
        r = gpsacq.dopfine_params()
        for k, v in kw.items():
            r[k] = v
        return r
    for kw in (dict(blocks=0), dict(blocks=65), dict(min_segments=1), dict(snr_min=np.inf), dict(snr_min=np.nan), dict(coherence_min=-1e-9),
               dict(coherence_min=np.nan), dict(coherence_min=np.inf)):
        assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(bad_params(**kw)), p(out)) == 1, kw
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, 4999, p(tasks), p(pk), n, p(prm), p(out)) == 1 and b"stride" in lib.gpsacq_last_error()
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, (1 << 31) + 1, p(tasks), p(pk), n, p(prm), p(out)) == 1
    assert lib.gpsacq_fine_doppler(h, None, n_bytes, stride, p(tasks), p(pk), n, p(prm), p(out)) == 1
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, stride, p(tasks), None, n, p(prm), p(out)) == 1
    assert lib.gpsacq_fine_doppler(h, p(cap), 0, stride, p(tasks), p(pk), n, p(prm), p(out)) == 1
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, stride, p(tasks), p(pk), 0, p(prm), p(out)) == 1
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(prm), None) == 1
    assert lib.gpsacq_fine_doppler(None, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(prm), p(out)) == 1
    rb = np.zeros(n, gpsacq.RATE_OBS_DTYPE)
    rb.view(np.uint8)[:] = 0xA5
    assert lib.gpsacq_rate_obs_fine(h, p(pk), None, n, 1, 25.0, p(rb)) == 1 and lib.gpsacq_rate_obs_fine(h, None, p(host), n, 1, 25.0, p(rb)) == 1
    assert lib.gpsacq_rate_obs_fine(h, p(pk), p(host), 1, 13, 25.0, p(rb)) == 1 and lib.gpsacq_rate_obs_fine(h, p(pk), p(host), 0, 1, 25.0, p(rb)) == 1
    assert lib.gpsacq_rate_obs_fine(h, p(pk), p(host), n, 0, 25.0, p(rb)) == 1 and lib.gpsacq_rate_obs_fine(h, p(pk), p(host), n, 1, float("nan"), p(rb)) == 1
    assert lib.gpsacq_rate_obs_fine(h, p(pk), p(host), n, 1, 25.0, None) == 1
    assert (out.view(np.uint8) == 0xA5).all() and (rb.view(np.uint8) == 0xA5).all()
    assert lib.gpsacq_fine_doppler(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(prm), p(out)) == 0 and out.tobytes() == host.tobytes()


def test_unsupported_at_the_overflow_bound():
    """spm = 10000: 57 blocks keep the lag sums below 2^63, 58 do not (an engine of its own: another sample rate)"""
    import gpsacq
    assert 57 * 160000 * 10000 ** 3 < 2 ** 63 <= 58 * 160000 * 10000 ** 3
    with gpsacq.Engine(2.5e6, 10e6, 5000.0) as e:
        assert e.num_lags == 10000
        bits = np.random.default_rng(8).integers(0, 256, 3 * 10000 // 8 + 1, dtype=np.uint8)
        pk = np.zeros(1, gpsacq.PEAK_DTYPE)
        pk[0] = (50.0, 2, 123, 1.0)
        tasks = np.array([[0, 4]], np.int32)
        ok = e.fine_doppler(bits, pk, tasks=tasks, stride=5000, params=gpsacq.dopfine_params(blocks=57))
        dop_ref.same(ok, dop_ref.fine_doppler(bits, 5000, tasks.tolist(), pk, 10000, 2.5e6, 10e6, blocks=57), "57 blocks")
        assert ok["segments"][0] == 3 and ok["flags"][0] == dop_ref.SHORT
        out = np.zeros(1, gpsacq.DOPFINE_DTYPE)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = e._lib.gpsacq_fine_doppler(e._h, p(bits), bits.size, 5000, p(tasks), p(pk), 1, p(gpsacq.dopfine_params(blocks=58)), p(out))
        assert rc == 3 and not out.view(np.uint8).any(), (rc, e._lib.gpsacq_last_error())


# ---- 3. the solver against the reference ------------------------------------------------------------------------------------------
def doppler_rows(which, n, cols, seed, noise_hz=1.5, drift=2e-6, step_s=0.5, t0=0.25):
    """n rows of `cols` satellites of a geometry at receive times ref_ms + t0 + k step_s: OBS_DTYPE and RATE_OBS_DTYPE [n][len(cols)] with
    the exact Dopplers (the central difference of the truth's transmit times over a second) less L1 drift, plus Gaussian noise"""
    import gpsacq
    geo = geometry(which)
    t_rx = t0 + step_s * np.arange(n)
    obs = np.zeros((n, len(cols)), gpsacq.OBS_DTYPE)
    ro = np.zeros((n, len(cols)), gpsacq.RATE_OBS_DTYPE)
    for j, s in enumerate(cols):
        lo, hi = (nav_ref.truth_tx(geo["ephs"][s], geo["rx"], geo["ref_ms"], t_rx + d) for d in (-0.5, 0.5))
        obs["eph"][:, j], ro["doppler_hz"][:, j] = s, dop_ref.L1 * ((hi - lo) - 1.0) - dop_ref.L1 * drift
    obs["valid"], obs["weight"], ro["valid"], ro["weight"] = 1, 1.0, 1, 1.0
    ro["doppler_hz"] += np.random.default_rng(seed).normal(scale=noise_hz, size=ro.shape)
    rx_ms = ((geo["ref_ms"] + np.floor(t_rx * 1000).astype(np.int64)) % nav_ref.WEEK_MS).astype(np.int32)
    return geo, obs, ro, rx_ms


def both_forms(eng, geo, obs, ro, rx_ms, label, params=None, host=True):
    """device form (poison behind both outputs) and, where the inputs allow it, the host form: byte for byte the same, and both
    against the reference"""
    import torch
    rec = to_records(geo["ephs"])
    n, m = obs.shape
    d_obs, d_ro, d_rx = dev(obs), dev(ro), dev(rx_ms)
    d_fix, d_pr = fill(n * 88 + 88), fill(n * 32 + 32)
    torch.cuda.synchronize()
    eng.doppler_fix_device(rec, d_obs.data_ptr(), d_ro.data_ptr(), d_rx.data_ptr(), n, m, d_fix.data_ptr(), d_pr.data_ptr(), params=params, sync=True)
    import gpsacq
    fb, pb = d_fix.cpu().numpy(), d_pr.cpu().numpy()
    assert (fb[n * 88:] == 0xA5).all() and (pb[n * 32:] == 0xA5).all()
    fix, pr = np.frombuffer(fb[:n * 88].tobytes(), gpsacq.DOPPLER_FIX_DTYPE), np.frombuffer(pb[:n * 32].tobytes(), gpsacq.COARSE_PRIOR_DTYPE)
    if host:
        hfix, hpr = eng.doppler_fix(rec, obs, ro, rx_ms, params=params)
        assert hfix.tobytes() == fix.tobytes() and hpr.tobytes() == pr.tobytes(), label
    ref = dop_ref.doppler_fix(geo["ephs"], obs, ro, rx_ms, rms_max_mps=dop_ref.RMS_MAX_MPS if params is None else float(params["rms_max_mps"][0]))
    worst = dop_ref.same_fix(fix, pr, ref, rx_ms, label)
    return fix, pr, ref, worst


SOLVER_CASES = [(130, 12), (65, 8), (64, 5), (63, 4), (1, 3)]


@pytest.mark.parametrize("n,m", SOLVER_CASES)
def test_doppler_fix_against_the_reference(eng, n, m):
    """1, 63, 64, 65 and 130 rows (one wave, its edges, three workgroups) of 12, 8, 5, 4 and 3 columns with 1.5 Hz of noise"""
    geo = geometry("north")
    cols = geo["subsets"][m] if m in geo["subsets"] else geo["subsets"][4][:m]
    geo, obs, ro, rx_ms = doppler_rows("north", n, cols, seed=n + m)
    fix, pr, ref, worst = both_forms(eng, geo, obs, ro, rx_ms, "%d x %d" % (n, m))
    ms = eng.doppler_last_ms()
    if m >= 4:
        err = np.linalg.norm(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"], axis=1)
        print("%d rows x %d columns: place within %.3g m and drift within %.3g of the reference; %d..%d steps; %.1f km median, %.1f km worst from "
              "the truth; rms %.2f..%.2f m/s; k_doppler_fix %.4f ms" % (n, m, *worst, fix["iterations"].min(), fix["iterations"].max(),
                                                                    np.median(err) / 1e3, err.max() / 1e3, fix["rms"].min(), fix["rms"].max(), ms[2]))
        assert (fix["status"] == 0).all() and (fix["n_used"] == m).all()
        if m >= 8:
            assert (fix["flags"] == 0).all() and err.max() < 59e3
    else:
        assert (fix["status"] == dop_ref.FIX_TOO_FEW).all() and (fix["n_used"] == 3).all() and np.isnan(pr["x"]).all()
    assert ms[2] > 0


def test_doppler_fix_edges(eng):
    """holes, a weight 0, bad weights and times (device form only: the host form refuses them), the end of the week, a Doppler
    200 Hz off, rms_max_mps, and every argument error"""
    import gpsacq
    geo, obs, ro, rx_ms = doppler_rows("north", 12, geometry("north")["subsets"][8], seed=3)
    obs["valid"][0, 2] = 0                      # a hole in the observations
    ro["valid"][1, 5] = 0                       # and in the rate observations
    ro["weight"][2, 1] = 0.0                    # counted in n_used, no part of the solve or of pdop
    obs["eph"][3, 0] = 12                       # no such ephemeris
    obs["eph"][3, 1] = -1
    ro["doppler_hz"][4, 7] = np.nan
    ro["doppler_hz"][5, 3] += 200.0             # INCONSISTENT
    obs["valid"][6, :5] = 0                     # three left: TOO_FEW
    ro["weight"][7, :] = 0.0                    # nothing to solve: NO_CONVERGE
    ro["weight"][8, :] = [1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 4.0, 1.0]
    obs["weight"][9, :] = np.nan                # gpsacq_obs.weight and tx_frac are not read
    obs["tx_frac"][9, :] = np.inf
    fix, pr, ref, worst = both_forms(eng, geo, obs, ro, rx_ms, "edges")
    assert fix["n_used"].tolist() == [7, 7, 8, 6, 7, 8, 3, 8, 8, 8, 8, 8] and fix["status"].tolist() == [0] * 6 + [1, 2] + [0] * 4
    assert fix["flags"].tolist() == [0] * 5 + [1] + [0] * 6 and np.isnan(pr["x"][[5, 6, 7]]).all() and np.isfinite(pr["x"][[0, 1, 2, 3, 4, 8, 9]]).all()
    assert fix["pdop"][2] > fix["pdop"][10] > 0  # seven satellites' dilution against eight's
    print("edges: place within %.3g m, drift within %.3g; the row 200 Hz off has rms %.2f m/s" % (*worst, fix["rms"][5]))
    # a larger rms_max_mps lets the row pass, a smaller one flags the noise
    loose = both_forms(eng, geo, obs, ro, rx_ms, "loose", params=gpsacq.doppler_fix_params(50.0))[0]
    tight = both_forms(eng, geo, obs, ro, rx_ms, "tight", params=gpsacq.doppler_fix_params(1e-3))[0]
    assert loose["flags"][5] == 0 and (tight["flags"][fix["status"] == 0] == 1).all()
    # the device form skips a column with a bad weight and a row with a bad time; the host form refuses both
    bad_w, bad_t = ro.copy(), rx_ms.copy()
    bad_w["weight"][10, 4], bad_w["weight"][11, 0] = -1.0, np.inf
    bad_t[0], bad_t[1] = -1, nav_ref.WEEK_MS
    dfix = both_forms(eng, geo, obs, bad_w, bad_t, "bad weights and times", host=False)[0]
    assert dfix["n_used"].tolist()[:2] == [0, 0] and dfix["status"].tolist()[:2] == [1, 1] and dfix["n_used"].tolist()[10:] == [7, 7]
    rec = to_records(geo["ephs"])
    for o2, r2, t2 in ((obs, bad_w, rx_ms), (obs, ro, bad_t)):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.doppler_fix(rec, o2, r2, t2)
        assert ei.value.code == 1
    # the end of the week: receive times on both sides of it
    gr, ob2, ro2, rx2 = doppler_rows("rollover", 8, geometry("rollover")["subsets"][8], seed=4, step_s=0.02, t0=0.05)
    assert rx2.min() < 1000 and rx2.max() > nav_ref.WEEK_MS - 1000
    f2, _, _, w2 = both_forms(eng, gr, ob2, ro2, rx2, "rollover")
    e2 = np.linalg.norm(np.stack([f2["x"], f2["y"], f2["z"]], 1) - gr["rx"], axis=1)
    print("across the end of the week: place within %.3g m of the reference, %.1f km worst from the truth" % (w2[0], e2.max() / 1e3))
    assert (f2["status"] == 0).all() and e2.max() < 59e3
    # an ephemeris that fails SATELLITE STATE's rule is no column
    rec_bad = rec.copy()
    rec_bad["iode3"][int(obs["eph"][0, 0])] ^= 1
    fb, _ = eng.doppler_fix(rec_bad, obs, ro, rx_ms)
    want = dop_ref.doppler_fix(geo["ephs"], obs, ro, rx_ms, eph_valid=[k != int(obs["eph"][0, 0]) for k in range(12)])
    assert fb["n_used"].tolist() == [r["n_used"] for r in want] and fb["n_used"][10] == 7
    # argument errors return 1 and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    n, m = obs.shape
    out, po = np.zeros(n, gpsacq.DOPPLER_FIX_DTYPE), np.zeros(n, gpsacq.COARSE_PRIOR_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    po.view(np.uint8)[:] = 0xA5
    good = gpsacq.doppler_fix_params()
    call = lambda *a: lib.gpsacq_doppler_fix_batch(h, *a)
    assert call(None, 12, p(obs), p(ro), p(rx_ms), n, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 0, p(obs), p(ro), p(rx_ms), n, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, None, p(ro), p(rx_ms), n, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), None, p(rx_ms), n, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), p(ro), None, n, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), 0, m, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), n, 0, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), n, 13, p(good), p(out), p(po)) == 1
    assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), n, m, p(good), None, p(po)) == 1
    for v in (0.0, -1.0, np.nan, np.inf):
        assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), n, m, p(gpsacq.doppler_fix_params(v)), p(out), p(po)) == 1, v
    assert (out.view(np.uint8) == 0xA5).all() and (po.view(np.uint8) == 0xA5).all()
    assert call(p(rec), 12, p(obs), p(ro), p(rx_ms), n, m, None, p(out), None) == 0 and out.tobytes() == fix.tobytes()  # prior_out may be NULL


# ---- 4. and 5.: the northern receiver's eight satellites, searched and fixed with no prior of place ----------------------------------
@pytest.fixture(scope="module")
def scene(eng):
    """tests/test_gpu_refine.py's scene: eight satellites at amplitude 0.2 in a 19-block capture, blocks 0..3 searched; the time
    prior of every block is 20 s off, early and late in turn"""
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, n_search, spb = 19, 4, 5120 * 8
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3  # the receive time of the first sample of block 0
    sats, dops = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.2)
    bits = eng.generate(n_blocks * 5120, sats, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = np.array([(b, s[0] - 1) for b in range(n_search) for s in sats], np.int32)
    _, peaks = eng.search(bits[:n_search * 5120], tasks=tasks, want_cells=False)
    blk_ms, blk_frac = block_times(ref_ms, ref_frac, n_search, spb, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    bits.setflags(write=False)
    return dict(geo=geo, sel=sel, ephs=ephs, bits=bits, tasks=tasks, peaks=peaks.reshape(n_search, len(sel)), blk_ms=blk_ms, blk_frac=blk_frac,
                prior=prior, rx_ms=np.ascontiguousarray(prior["rx_ms"].astype(np.int32)), rec=to_records(ephs), dops=dops)


def test_chain(eng, scene):
    """gpsacq_cold_fix_device = its seven kernels run one by one through the single entry points, byte for byte, with and without
    the optional buffers"""
    import gpsacq
    import torch
    n, m = scene["peaks"].shape
    d_bits, d_tasks, d_pk, d_rx = dev(scene["bits"]), dev(scene["tasks"]), dev(scene["peaks"]), dev(scene["rx_ms"])
    nb = scene["bits"].size
    sizes = dict(dopfine=n * m * 72, rate=n * m * 32, dfix=n * 88, prior=n * 32, fine=n * m * 56, obs=n * m * 32, fix=n * 80, info=n * 40, out=n * m * 32)
    a = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()
    eng.fine_doppler_device(ptr(d_bits), nb, ptr(d_pk), n * m, ptr(a["dopfine"]), d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_obs_device(ptr(d_pk), n, m, ptr(a["obs"]), sync=False)
    eng.rate_obs_fine_device(ptr(d_pk), ptr(a["dopfine"]), n, m, ptr(a["rate"]), sync=False)
    eng.doppler_fix_device(scene["rec"], ptr(a["obs"]), ptr(a["rate"]), ptr(d_rx), n, m, ptr(a["dfix"]), ptr(a["prior"]), sync=False)
    eng.refine_device(ptr(d_bits), nb, ptr(d_pk), n * m, ptr(a["fine"]), d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_obs_fine_device(ptr(d_pk), ptr(a["fine"]), n, m, ptr(a["obs"]), sync=False)
    eng.coarse_fix_device(scene["rec"], ptr(a["obs"]), ptr(a["prior"]), n, m, ptr(a["fix"]), ptr(a["info"]), ptr(a["out"]), sync=True)
    steps = {k: t.cpu().numpy().tobytes() for k, t in a.items()}
    fix = np.frombuffer(steps["fix"], gpsacq.FIX_DTYPE)
    assert (fix["status"] == 0).all() and (fix["n_used"] == m).all()
    b = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.cold_fix_device(scene["rec"], ptr(d_bits), nb, ptr(d_tasks), ptr(d_pk), ptr(d_rx), n, m, ptr(b["fix"]), ptr(b["info"]), ptr(b["dfix"]),
                        d_dopfine_ptr=ptr(b["dopfine"]), d_rate_obs_ptr=ptr(b["rate"]), d_prior_ptr=ptr(b["prior"]), d_fine_ptr=ptr(b["fine"]),
                        d_obs_ptr=ptr(b["obs"]), d_obs_out_ptr=ptr(b["out"]), sync=True)
    for k, t in b.items():
        assert t.cpu().numpy().tobytes() == steps[k], k
    c = {k: fill(sizes[k]) for k in ("fix", "info", "dfix")}
    torch.cuda.synchronize()
    eng.cold_fix_device(scene["rec"], ptr(d_bits), nb, ptr(d_tasks), ptr(d_pk), ptr(d_rx), n, m, ptr(c["fix"]), ptr(c["info"]), ptr(c["dfix"]), sync=True)
    for k, t in c.items():
        assert t.cpu().numpy().tobytes() == steps[k], k
    ms, rms = eng.doppler_last_ms(), eng.refine_last_ms()
    print("chain: k_fine_dop %.4f ms, k_rate_obs_fine %.4f ms, k_doppler_fix %.4f ms, k_refine %.4f ms for %d tasks of 16 blocks" % (*ms, rms[0], n * m))
    assert min(ms) > 0
    # argument errors: nothing launched, nothing written
    d = {k: fill(sizes[k]) for k in ("fix", "info", "dfix")}
    torch.cuda.synchronize()
    args = lambda **kw: dict(dict(eph=scene["rec"], d_bits_ptr=ptr(d_bits), n_bytes=nb, d_tasks_ptr=ptr(d_tasks), d_peaks_ptr=ptr(d_pk), d_rx_ms_ptr=ptr(d_rx),
                                  n_fix=n, n_chans=m, d_fix_ptr=ptr(d["fix"]), d_info_ptr=ptr(d["info"]), d_doppler_fix_ptr=ptr(d["dfix"])), **kw)
    for kw in (dict(d_bits_ptr=None), dict(d_peaks_ptr=None), dict(d_rx_ms_ptr=None), dict(d_fix_ptr=None), dict(d_info_ptr=None),
               dict(d_doppler_fix_ptr=None), dict(n_fix=0), dict(n_chans=0), dict(n_chans=13), dict(n_bytes=0), dict(stride=4999),
               dict(dopfine_params=np.array([(0, 2, 25.0, 0.0)], gpsacq.DOPFINE_PARAMS_DTYPE)), dict(doppler_params=gpsacq.doppler_fix_params(-1.0)),
               dict(refine_params=np.array([(16, 0, 0.25, 25.0)], gpsacq.REFINE_PARAMS_DTYPE)), dict(params=gpsacq.coarse_params(0.0)),
               dict(d_obs_ptr=ptr(a["obs"]), d_obs_out_ptr=ptr(a["obs"]))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.cold_fix_device(**args(**kw))
        assert ei.value.code == 1, kw
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in d.values())


def test_end_to_end_cold_fixes(eng, scene):
    """Four blocks of a 19-block capture, eight satellites at amplitude 0.2, a time 20 s off and no place at all.

    Measured on an MI355X (printed by this test): Doppler against the generator's over the 32 hits 1.88 Hz rms, 3.63 Hz worst (the bin
    centres 16.53 / 34.30 Hz), coherence 0.830 .. 0.940; Doppler fixes 19.0 / 15.3 / 16.9 / 14.7 km from the truth in 5 steps each,
    rms 0.64 / 0.22 / 0.61 / 0.32 m/s, pdop 17 400 m per m/s; cold fixes 3.24 / 0.48 / 2.54 / 3.01 m from the truth, 1.6e-8 m and less
    from the warm fine fixes; the velocity of the receiver at rest reads 0.55 .. 0.85 m/s with an rms of 0.22 .. 0.26 m/s."""
    import gpsacq
    import torch
    geo, peaks, rec = scene["geo"], scene["peaks"], scene["rec"]
    n, m = peaks.shape
    assert (peaks["snr"] >= gpsacq.THRESHOLD).all()
    dopfine = eng.fine_doppler(scene["bits"], peaks, tasks=scene["tasks"])
    ref = dop_ref.fine_doppler(scene["bits"], 5120, scene["tasks"].tolist(), peaks, SPM, FC, FS)
    worst = dop_ref.same(dopfine, ref, "end to end")
    assert (dopfine["flags"] == 0).all() and (dopfine["segments"] == 16 * 40000 // SPM).all()
    err_hz = dopfine["doppler_hz"] - scene["dops"][None, :]
    bin_hz = peaks["lo_shift"] * (FS / 40000) - scene["dops"][None, :]
    print("records equal the reference: coherence within %.3g, df_hz within %.3g Hz, doppler_hz within %.3g Hz" % tuple(worst))
    print("Doppler against the generator's over %d hits: fine rms %.2f Hz (worst %.2f), bin centres rms %.2f Hz (worst %.2f); coherence %.3f .. %.3f" %
          (n * m, np.sqrt((err_hz ** 2).mean()), np.abs(err_hz).max(), np.sqrt((bin_hz ** 2).mean()), np.abs(bin_hz).max(), dopfine["coherence"].min(),
           dopfine["coherence"].max()))
    assert np.abs(err_hz).max() < np.abs(bin_hz).max()
    # the chain, every buffer kept
    d_bits, d_tasks, d_pk, d_rx = dev(scene["bits"]), dev(scene["tasks"]), dev(peaks), dev(scene["rx_ms"])
    b = dict(rate=fill(n * m * 32), dfix=fill(n * 88), prior=fill(n * 32), fix=fill(n * 80), info=fill(n * 40), out=fill(n * m * 32))
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()
    eng.cold_fix_device(rec, ptr(d_bits), scene["bits"].size, ptr(d_tasks), ptr(d_pk), ptr(d_rx), n, m, ptr(b["fix"]), ptr(b["info"]), ptr(b["dfix"]),
                        d_rate_obs_ptr=ptr(b["rate"]), d_prior_ptr=ptr(b["prior"]), d_obs_out_ptr=ptr(b["out"]), sync=True)
    get = lambda k, dt: np.frombuffer(b[k].cpu().numpy().tobytes(), dt)
    dfix, prior, fix, info = get("dfix", gpsacq.DOPPLER_FIX_DTYPE), get("prior", gpsacq.COARSE_PRIOR_DTYPE), get("fix", gpsacq.FIX_DTYPE), get(
        "info", gpsacq.COARSE_INFO_DTYPE)
    rate, obs_out = get("rate", gpsacq.RATE_OBS_DTYPE).reshape(n, m), get("out", gpsacq.OBS_DTYPE).reshape(n, m)
    # the Doppler fixes against the reference and the truth
    rref = dop_ref.doppler_fix(scene["ephs"], eng.coarse_obs(peaks), rate, scene["rx_ms"])
    dop_ref.same_fix(dfix, prior, rref, scene["rx_ms"], "end to end")
    derr = np.linalg.norm(np.stack([dfix["x"], dfix["y"], dfix["z"]], 1) - geo["rx"], axis=1)
    print("Doppler fixes: %s km from the truth, %s steps, rms %s m/s, pdop %s m per m/s, drift %s" %
          (np.round(derr / 1e3, 2), dfix["iterations"], np.round(dfix["rms"], 3), np.round(dfix["pdop"]), dfix["drift"]))
    assert (dfix["status"] == 0).all() and (dfix["flags"] == 0).all() and (dfix["n_used"] == m).all()
    assert derr.max() < 59e3  # the coarse-time condition at dt = 20 s: (150 km - 1600 m/s * 20 s) / 2
    # the cold fixes against the warm ones of the same blocks: the same five-state optimum from another start
    d_warm = dev(scene["prior"])
    w_fix, w_info = fill(n * 80), fill(n * 40)
    torch.cuda.synchronize()
    eng.coarse_fix_fine_device(rec, ptr(d_bits), scene["bits"].size, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_warm), ptr(w_fix), ptr(w_info), sync=True)
    warm = np.frombuffer(w_fix.cpu().numpy().tobytes(), gpsacq.FIX_DTYPE)
    xyz = lambda f: np.stack([f["x"], f["y"], f["z"]], 1)
    gap = np.linalg.norm(xyz(fix) - xyz(warm), axis=1)
    cold_err, warm_err = np.linalg.norm(xyz(fix) - geo["rx"], axis=1), np.linalg.norm(xyz(warm) - geo["rx"], axis=1)
    print("cold fixes %s m from the truth, warm fine fixes %s m; cold against warm %s m" % (np.round(cold_err, 2), np.round(warm_err, 2), gap))
    assert (fix["status"] == 0).all() and (warm["status"] == 0).all() and (info["flags"] == 0).all() and (fix["n_used"] == m).all()
    assert gap.max() <= 1e-2
    # a snapshot velocity for free: obs_out, the rate observations and the fixes into gpsacq_vel_batch unchanged
    vel = eng.velocity(rec, obs_out, rate, fix)
    speed = np.sqrt(vel["vx"] ** 2 + vel["vy"] ** 2 + vel["vz"] ** 2)
    print("velocity of a receiver at rest: speed %s m/s, drift %s, rms %s m/s" % (np.round(speed, 3), vel["drift"], np.round(vel["rms"], 3)))
    assert (vel["status"] == 0).all() and (vel["n_used"] == m).all()
