"""Aided acquisition on the GPU (gpsacq_aid_predict*, gpsacq_aided_search*, gpsacq_aided_peaks_device) against tests/aided_ref.py,
the numpy restatement of "Aided acquisition: predicted code phase and Doppler, windowed search" of include/gpsacq.h.

Every integer field of a record and every entry of powers_out must equal the reference; ratio may differ by aided_ref.RATIO_TOL =
1e-12 relative (one fp64 division).  Predictions: integers equal, tx_frac within 1e-12 s, elev_deg within 1e-9 degrees, doppler_hz
within 1e-6 Hz.  fs = 5.456 MHz, fc = 4.092 MHz; the bits come from Engine.generate.  The reference's sums are its quick spelling
(Law.powers_stream), which tests/test_aided.py holds against the sample-by-sample one on the CPU.
Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_ref
from coarse_helpers import block_times
from nav_helpers import to_records

pytestmark = pytest.mark.gpu

FS, FC, SPM = ac.FS, ac.FC, ac.SPM


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


def hand_aid(kmax, n, seed):
    """n hand-made predictions that reach the edges: ca_center in {0, 1, 2727, spm - 1} (the wrap on both sides) x lo_center in
    {-kmax, 0, +kmax} (invalid d rows at the grid's ends) x PRN 1 and 32 (24 combinations, cycled), blocks 0 and 1"""
    import gpsacq
    combos = [(ca, lo, prn) for ca in (0, 1, 2727, SPM - 1) for lo in (-kmax, 0, kmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    aid = np.zeros(n, gpsacq.AID_DTYPE)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        aid[t] = (0, ca, lo, 0, ca / FS, lo * ac.STEP_HZ, 45.0)
        tasks[t] = (t % 2, prn)
    return tasks, aid


def reference(eng, bits, stride, tasks, aid, **kw):
    step = 0.0 if eng.doppler_sub == 1 and eng.doppler_stride == 1 else eng.doppler_step_hz
    return aided_ref.aided_search(bits, stride, None if tasks is None else tasks.tolist(), aid, SPM, FC, FS, eng.kmax, step_hz=step, stream=True, **kw)


# ---- 1. exact against the reference --------------------------------------------------------------------------------------------
CASES = [(1, 0, 0, 5000), (1, 5, 1, 5003), (2, 40, 2, 5000), (3, 100, 1, 5003), (2, 100, 0, 5000), (3, 5, 2, 5000), (1, 40, 1, 5000), (2, 0, 1, 5003),
         (3, 16, 1, 5000), (1, 100, 2, 5003), (2, 5, 0, 5003), (3, 40, 0, 5000)]


@pytest.mark.parametrize("blocks,W,K,stride", CASES)
def test_exact_against_the_reference(eng, capture, blocks, W, K, stride):
    import gpsacq
    tasks, aid = hand_aid(eng.kmax, 12, seed=blocks * 1000 + W * 10 + K)
    prm = gpsacq.aided_params(blocks=blocks, code_half=W, dop_half=K, ratio_min=1.2)
    got, pk, pw = eng.aided_search(capture, aid, tasks=tasks, stride=stride, params=prm, powers=True)
    ref = reference(eng, capture, stride, tasks, aid, blocks=blocks, code_half=W, dop_half=K, ratio_min=1.2)
    worst = aided_ref.same(got, ref, pk, pw, "blocks %d W %d K %d stride %d" % (blocks, W, K, stride))
    rows = sum(int(not r["powers"][d].any()) for r in ref for d in range(2 * K + 1))
    print("blocks %d, W %d, K %d, stride %d: 12 records, %d powers and the peaks equal the reference (%d rows of invalid d); ratio within %.3g; "
          "flags %s" % (blocks, W, K, stride, pw.size, rows, worst, sorted(set(got["flags"].tolist()))))
    assert (got["segments"] == blocks * 40000 // SPM).all() and (got["n_code"] == 2 * W + 1).all() and (got["n_dop"] == 2 * K + 1).all()
    assert not (got["flags"] & ~gpsacq.AIDED_BELOW).any() and (got["best"] > 0).all()
    assert (rows > 0) == (K > 0)


def test_powers_are_refines_prompt_sums(eng, capture):
    """against a kernel already merged: for base + h < spm, power(h, d) is the `prompt` k_refine returns for the peak (ca_shift_h,
    lo_shift_d)"""
    import gpsacq
    W, K, blocks = 5, 1, 2
    tasks, aid = hand_aid(eng.kmax - 1, 8, seed=77)  # every d on the grid
    _, _, pw = eng.aided_search(capture, aid, tasks=tasks, params=gpsacq.aided_params(blocks=blocks, code_half=W, dop_half=K), powers=True)
    peaks, ptasks, where = [], [], []
    for t in range(len(aid)):
        base = (int(aid["ca_center"][t]) - W) % SPM
        for d in range(2 * K + 1):
            for h in range(2 * W + 1):
                if base + h < SPM:
                    peaks.append((30.0, int(aid["lo_center"][t]) - K + d, base + h, 0.0))
                    ptasks.append(tuple(tasks[t]))
                    where.append((t, d, h))
    fine = eng.refine(capture, np.array(peaks, gpsacq.PEAK_DTYPE), tasks=np.array(ptasks, np.int32), params=gpsacq.refine_params(blocks=blocks))
    mine = np.array([pw[w] for w in where], np.uint64)
    print("%d of %d powers have a refine peak; all equal its prompt: %s" % (len(where), pw.size, bool((fine["prompt"] == mine).all())))
    assert (fine["flags"] == 0).all() and (fine["prompt"] == mine).all() and 0 < len(where) < pw.size


def test_a_finer_doppler_grid():
    """gpsacq_set_doppler_step(50.0): an engine of its own, its grid is changed; lo_center counts its points"""
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        e.set_doppler_step(50.0)
        assert e.doppler_sub == 3 and e.kmax > 100
        bits = e.generate(2 * 5120, [(7, 0.3, 1000.0, 321.5, 0.2)], noise_sigma=1.0, seed=8)
        tasks, aid = hand_aid(e.kmax, 6, seed=3)
        aid["lo_center"][0], tasks[0] = int(round(1000.0 / e.doppler_step_hz)), (0, 6)
        aid["ca_center"][0] = int(round(ac.law_center((7, 0.3, 1000.0, 321.5, 0.2), 0)[0])) % SPM
        prm = gpsacq.aided_params(blocks=1, code_half=5, dop_half=2)
        got, pk, pw = e.aided_search(bits, aid, tasks=tasks, params=prm, powers=True)
        ref = reference(e, bits, 5120, tasks, aid, blocks=1, code_half=5, dop_half=2)
        aided_ref.same(got, ref, pk, pw, "finer grid")
        print("step %.3f Hz, kmax %d: 6 records equal the reference; the satellite at 1000 Hz reads ratio %.2f at lo_shift %d" %
              (e.doppler_step_hz, e.kmax, got["ratio"][0], got["lo_shift"][0]))
        assert got["flags"][0] == 0 and abs(int(got["lo_shift"][0]) * e.doppler_step_hz - 1000.0) <= 2.5 * e.doppler_step_hz
        e.set_noncoherent(2)
        with pytest.raises(gpsacq.GpsAcqError) as err:
            e.aided_search(bits, aid, tasks=tasks, params=prm)
        assert err.value.code == 3  # GPSACQ_ERR_UNSUPPORTED


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------
def test_edges(eng, capture):
    import gpsacq
    import torch
    n_bytes, stride = 15000 + 7 * 682, 5000  # the window of a task of block 3 ends with the capture, in the middle of a 32-bit word
    kmax = eng.kmax
    rows = [(1, 0, 0, 100, 3),          # 0: the whole window of 21 segments
            (3, 0, 0, 0, -kmax),        # 1: SHORT, its last segment ends with the capture; one invalid d row
            (2, 31, 0, 5455, kmax),     # 2: SHORT, 14 segments and a tail
            (3, 31, 0, 2727, 0),        # 3: SHORT
            (4, 0, 0, 7, 0),            # 4: the block starts beyond the capture
            (0, 0, 4, 7, 0),            # 5: a flagged prediction
            (0, 0, 0, -1, 0),           # 6
            (0, 0, 0, SPM, 0),          # 7
            (0, 32, 0, 7, 0),           # 8: a task list with prn = 32
            (-1, 0, 0, 7, 0),           # 9
            (0, 5, 0, 1, kmax + 2),     # 10: no Doppler hypothesis on the grid
            (0, 5, 0, 1, -kmax - 3),    # 11
            (0, 5, 0, 1, 2 ** 31 - 1),  # 12
            (0, 5, 0, 1, kmax + 1),     # 13: one of three on the grid
            (0, 31, 0, 4000, -21)]      # 14: kept
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    aid = np.zeros(len(rows), gpsacq.AID_DTYPE)
    for t, r in enumerate(rows):
        aid[t] = (r[2], r[3], r[4], 0, 0.0, 0.0, 45.0)
    pin = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    pin["snr"], pin["lo_shift"], pin["ca_shift"], pin["max_pwr"] = 24.99, 5, 6, 7.0
    pin[14] = (25.0, -21, 4001, 1234.5)
    kw = dict(blocks=3, min_segments=8, code_half=40, dop_half=1, ratio_min=1.0)
    prm = gpsacq.aided_params(**kw)
    ref = reference(eng, capture, stride, tasks, aid, peaks_in=pin, n_bytes=n_bytes, **kw)
    fit = 3 * 40000 // SPM
    assert [r["flags"] & 15 for r in ref] == [0, 4 | 8, 4, 4 | 8, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1] and [r["segments"] for r in ref][:4] == [fit, 7, 14, 7]
    host, hpk, hpw = eng.aided_search(capture[:n_bytes], aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True)
    worst = aided_ref.same(host, ref, hpk, hpw, "host form")
    for t in range(4, 13):
        assert host[t].tobytes() == np.int32(2).tobytes() + bytes(60) and hpk[t].tobytes() == bytes(16) and not hpw[t].any(), t
    assert host[14].tobytes() == np.int32(1).tobytes() + bytes(60) and hpk[14].tobytes() == pin[14].tobytes() and not hpw[14].any()
    assert not hpw[1][0].any() and hpw[1][1].any() and not hpw[13][1:].any() and hpw[13][0].any()
    assert hpk[1].tobytes() == bytes(16) and hpk[3].tobytes() == bytes(16)  # FEW: measured, and no peak
    # the device form at odd addresses, sentinel bytes of either kind behind the capture, poisoned outputs
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_tasks, d_aid, d_pin = dev(tasks), dev(aid), dev(pin)
    n = len(rows)
    outs = []
    for sentinel in (0x00, 0xFF):
        buf = np.full(1 + n_bytes + 67, sentinel, np.uint8)
        buf[1:1 + n_bytes] = capture[:n_bytes]
        d_bits = dev(buf)
        d_out, d_pk, d_pw = (torch.full((k,), 0xA5, dtype=torch.uint8, device="cuda:0") for k in ((n + 1) * 64, (n + 1) * 16, (n + 1) * 3 * 81 * 8))
        torch.cuda.synchronize()
        eng.aided_search_device(d_bits.data_ptr() + 1, n_bytes, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), stride=stride,
                                d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=d_pw.data_ptr(), params=prm, sync=True)
        outs.append([x.cpu().numpy().tobytes() for x in (d_out, d_pk, d_pw)])
    for o in outs:
        assert o[0] == host.tobytes() + b"\xa5" * 64 and o[1] == hpk.tobytes() + b"\xa5" * 16 and o[2] == hpw.tobytes() + b"\xa5" * (3 * 81 * 8)
    ms = eng.aided_last_ms()
    print("edges: ratio within %.3g; host and device forms agree byte for byte, nothing written beyond the records; k_aided %.4f ms for %d tasks" %
          (worst, ms[1], n))
    assert ms[1] > 0
    # the reference schedule (tasks == NULL is (block t, PRN t % 32)), and no input peaks: nothing is kept
    sched, spk = eng.aided_search(capture[:n_bytes], aid[:4], stride=stride, params=prm)
    aided_ref.same(sched, reference(eng, capture, stride, None, aid[:4], n_bytes=n_bytes, **kw), spk, None, "schedule")
    # an exact tie: an all-zero capture gives every hypothesis the power of the carrier alone only where the chips agree; W = 0 leaves
    # the three d, and the two ends of the grid have one valid d each
    zeros = np.zeros(2 * 5120, np.uint8)
    tie_aid = aid[[0, 0, 0]].copy()
    tie_aid["lo_center"] = (0, kmax + 1, -kmax - 1)
    tt = np.zeros((3, 2), np.int32)
    tp = gpsacq.aided_params(blocks=1, code_half=2, dop_half=1, ratio_min=0.0)
    got, gpk, gpw = eng.aided_search(zeros, tie_aid, tasks=tt, params=tp, powers=True)
    aided_ref.same(got, reference(eng, zeros, 5120, tt, tie_aid, blocks=1, code_half=2, dop_half=1, ratio_min=0.0), gpk, gpw, "tie")
    ties = int((gpw[0] == gpw[0].max()).sum())
    print("all-zero capture: %d hypotheses tie at the largest power; best (d %d, h %d)" % (ties, got["best_d"][0], got["best_h"][0]))
    first = min((int(d), int(h)) for d, h in zip(*np.nonzero(gpw[0] == gpw[0].max())))
    assert ties >= 2 and (int(got["best_d"][0]), int(got["best_h"][0])) == first  # among equals the smaller d, then the smaller h
    assert got["best_d"].tolist()[1:] == [0, 2]
    # argument errors return 1, launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out, opk = np.zeros(n, gpsacq.AIDED_DTYPE), np.zeros(n, gpsacq.PEAK_DTYPE)
    cap = np.ascontiguousarray(capture[:n_bytes])

    def bad_params(**kv):
        r = gpsacq.aided_params()
        for k, v in kv.items():
            r[k] = v
        return r
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 0
    assert out.tobytes() == host.tobytes() and opk.tobytes() == hpk.tobytes()
    out[:], opk[:] = 0, 0
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(code_half=-1), dict(code_half=128), dict(dop_half=-1), dict(dop_half=9),
               dict(keep_snr=np.nan), dict(ratio_min=np.inf)):
        assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(bad_params(**kv)), p(out), p(opk), None) == 1, kv
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, 4999, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert b"stride" in lib.gpsacq_last_error()
    assert lib.gpsacq_aided_search(h, None, n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), None, p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), 0, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), 0, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), None, p(opk), None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), None, None) == 1
    assert lib.gpsacq_aided_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(opk), n, p(prm), p(out), p(opk), None) == 1
    assert not out.view(np.uint8).any() and not opk.view(np.uint8).any()


# ---- 3. prediction ---------------------------------------------------------------------------------------------------------------
def fixes_of(geo, ref_ms, frac, n, status=0):
    import gpsacq
    blk_ms, blk_frac = block_times(ref_ms, frac, n, 40960, FS)
    fix = np.zeros(n, gpsacq.FIX_DTYPE)
    fix["status"], fix["n_used"], fix["rx_ms"], fix["rx_frac"] = status, 8, blk_ms, blk_frac
    fix["x"], fix["y"], fix["z"] = geo["rx"]
    return fix


def test_prediction_against_the_reference(eng):
    import gpsacq
    geo, sel, present, absent, dops = ac.scene_sats()
    ephs = [geo["ephs"][k] for k in sel]
    rec = to_records(ephs)
    rec["iode3"][7] += 1  # channel 7: an ephemeris that is not valid
    fix = fixes_of(geo, geo["ref_ms"] + 4321, ac.REF_FRAC, 5)
    fix["status"][4] = gpsacq.FIX_NO_CONVERGE
    vel = np.zeros(5, gpsacq.VEL_DTYPE)
    vel["vx"], vel["vy"], vel["vz"], vel["drift"] = 11.0, -7.5, 3.25, 3e-7
    vel["status"][1] = gpsacq.VEL_SINGULAR  # row 1: no velocity after all
    vel["drift"][2] = 1e-5                  # row 2: 15.75 kHz of clock, off the grid
    worst = [0.0, 0.0, 0.0]
    for v, elev, label in ((None, 5.0, "at rest"), (vel, 5.0, "moving"), (None, 40.0, "mask 40 degrees")):
        got = eng.aid_predict(rec, fix, 9, vel=v, params=gpsacq.aid_params(elev))  # 9 channels: the last has no ephemeris at all
        ref = aided_ref.predict(ephs[:7] + [None], fix, v, 9, FS, SPM, eng.doppler_step_hz, eng.kmax, elev_min_deg=elev)
        for f in range(5):
            for c in range(9):
                g, r = got[f][c], ref[f][c]
                if r["flags"] & ~(aided_ref.AID_NO_FIX | aided_ref.AID_NO_EPH) == r["flags"] and r["tx_frac"]:
                    ca, lo = r["tx_frac"] * FS, r["doppler_hz"] / eng.doppler_step_hz
                    assert abs(ca - np.floor(ca) - 0.5) > 1e-6 and abs(lo - np.floor(lo) - 0.5) > 1e-6, (label, f, c)  # no case on a rounding edge
                for k in ("flags", "ca_center", "lo_center", "reserved"):
                    assert int(g[k]) == r[k], (label, f, c, k, int(g[k]), r[k])
                d = [abs(float(g["tx_frac"]) - r["tx_frac"]), abs(float(g["doppler_hz"]) - r["doppler_hz"]), abs(float(g["elev_deg"]) - r["elev_deg"])]
                assert d[0] <= 1e-12 and d[1] <= 1e-6 and d[2] <= 1e-9, (label, f, c, d)
                worst = [max(a, b) for a, b in zip(worst, d)]
        flags = got["flags"]
        assert (flags[4] == gpsacq.AID_NO_FIX).all() and (flags[:4, 7:] == gpsacq.AID_NO_EPH).all()
        for f, c in ((4, 0), (0, 7), (0, 8)):
            assert got[f][c].tobytes()[4:] == bytes(36)
        if label == "at rest":
            assert (flags[:4, :7] == 0).all()
            for c in range(6):  # against the generator's own law at the first block
                ca, lo = ac.law_center((present + absent)[c] if c < 6 else absent[c - 6], 0)
                assert abs((got["ca_center"][0][c] - ca + SPM / 2) % SPM - SPM / 2) <= 1.0 and abs(got["lo_center"][0][c] - lo) <= 1.0
        if label == "moving":
            assert (flags[2, :7] == gpsacq.AID_OFF_GRID).all() and (got[1] == eng.aid_predict(rec, fix, 9)[1]).all() and (flags[0, :7] == 0).all()
        if label == "mask 40 degrees":
            low = got["elev_deg"][:4, :7] < 40.0
            assert low.any() and not low.all() and ((flags[:4, :7] == gpsacq.AID_LOW) == low).all()
    print("predictions equal the reference: tx_frac within %.3g s, doppler_hz within %.3g Hz, elev_deg within %.3g degrees; k_aid_predict %.4f ms" %
          (worst[0], worst[1], worst[2], eng.aided_last_ms()[0]))
    lib, h, p = eng._lib, eng._h, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((5, 9), gpsacq.AID_DTYPE)
    assert lib.gpsacq_aid_predict(h, p(rec), 8, p(fix), None, 5, 13, None, p(out)) == 1 and lib.gpsacq_aid_predict(h, p(rec), 0, p(fix), None, 5, 9, None, p(out)) == 1
    assert lib.gpsacq_aid_predict(h, p(rec), 8, None, None, 5, 9, None, p(out)) == 1 and lib.gpsacq_aid_predict(h, p(rec), 8, p(fix), None, 0, 9, None, p(out)) == 1
    assert lib.gpsacq_aid_predict(h, p(rec), 8, p(fix), None, 5, 9, p(np.array([(91.0, 0.0)], gpsacq.AID_PARAMS_DTYPE)), p(out)) == 1
    assert not out.view(np.uint8).any()


# ---- 4. the chain, end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weak_scene(eng):
    """tests/test_aided.py's scene by Engine.generate: 16 blocks, five satellites at 0.2, one at WEAK_AMPLITUDE, two absent; block 0
    searched for all eight"""
    geo, sel, present, absent, dops = ac.scene_sats()
    bits = eng.generate(16 * 5120, present, noise_sigma=1.0, seed=2024)
    chans = present + absent
    tasks = np.array([(0, s[0] - 1) for s in chans], np.int32)
    _, peaks = eng.search(bits[:5120], tasks=tasks, want_cells=False)
    bits.setflags(write=False)
    return dict(geo=geo, rec=to_records([geo["ephs"][k] for k in sel]), bits=bits, chans=chans, tasks=tasks, peaks=peaks,
                fix=fixes_of(geo, geo["ref_ms"] + 4321, ac.REF_FRAC, 1))


def test_chain_and_end_to_end(eng, weak_scene):
    """Measured on an MI355X (printed by this test): the search of block 0 gives the five strong satellites snr 122 to 173, the weak
    one 14.60 and the absent ones 14.26 and 12.26 (noise peaks).  The aided search keeps the five, finds the weak one at ratio 2.453
    (ratio_min 1.922), ca_shift 4627 against the law's 4626.77 and lo_shift 2 against 2.86 (predicted 3: one-millisecond sums do not
    tell neighbouring grid points apart), and reads the absent ones at 1.2619 and 1.2701 -- the CPU's figures of
    tests/test_aided.py to the digit.  k_aid_predict 0.023 ms, k_aided 0.54 ms for the 8 tasks, 3 of them searched."""
    import gpsacq
    import torch
    w = weak_scene
    n = len(w["chans"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_bits, d_tasks, d_pin, d_fix = dev(w["bits"]), dev(w["tasks"]), dev(w["peaks"]), dev(w["fix"])
    nb = w["bits"].size
    # the two calls
    d_aid, d_out, d_pk = fill(n * 40), fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aid_predict_device(w["rec"], d_fix.data_ptr(), 1, n, d_aid.data_ptr(), sync=False)
    eng.aided_search_device(d_bits.data_ptr(), nb, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(),
                            d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    steps = [x.cpu().numpy().tobytes() for x in (d_aid, d_out, d_pk)]
    # the chain, with and without the optional buffer
    e_aid, e_out, e_pk = fill(n * 40), fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_peaks_device(w["rec"], d_fix.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, e_out.data_ptr(), e_pk.data_ptr(),
                           d_peaks_in_ptr=d_pin.data_ptr(), d_aid_ptr=e_aid.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (e_aid, e_out, e_pk)] == steps
    f_out, f_pk = fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_peaks_device(w["rec"], d_fix.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, f_out.data_ptr(), f_pk.data_ptr(),
                           d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (f_out, f_pk)] == steps[1:]
    ms = eng.aided_last_ms()
    aid = np.frombuffer(steps[0], gpsacq.AID_DTYPE)
    got = np.frombuffer(steps[1], gpsacq.AIDED_DTYPE)
    pk = np.frombuffer(steps[2], gpsacq.PEAK_DTYPE)
    # the host forms and the reference agree with it
    h_aid = eng.aid_predict(w["rec"], w["fix"], n)
    assert h_aid.tobytes() == steps[0]
    ref = reference(eng, w["bits"], 5120, w["tasks"], aid, peaks_in=w["peaks"])
    aided_ref.same(got, ref, pk, None, "end to end")
    snr = w["peaks"]["snr"]
    ca_law, lo_law = ac.law_center(w["chans"][5], 0)
    print("search snr of block 0: strong %s, weak %.2f, absent %.2f %.2f" % (np.round(snr[:5], 1), snr[5], snr[6], snr[7]))
    print("aided: flags %s, ratios %s; weak PRN at ca_shift %d (law %.2f), lo_shift %d (law %.2f, prediction %d); k_aid_predict %.4f ms, k_aided "
          "%.4f ms for %d tasks" % (got["flags"].tolist(), np.round(got["ratio"], 4), got["ca_shift"][5], ca_law, got["lo_shift"][5], lo_law,
                                    aid["lo_center"][5], ms[0], ms[1], n))
    assert (snr[:5] >= gpsacq.THRESHOLD).all() and snr[5] < gpsacq.THRESHOLD
    assert (got["flags"][:5] == gpsacq.AIDED_KEPT).all() and pk[:5].tobytes() == w["peaks"][:5].tobytes()
    assert got["flags"][5] == 0 and got["ratio"][5] >= aided_ref.RATIO_MIN
    assert abs((got["ca_shift"][5] - ca_law + SPM / 2) % SPM - SPM / 2) <= 1.0
    assert got["lo_shift"][5] == ref[5]["lo_shift"] == aid["lo_center"][5] - 1 + got["best_d"][5] and abs(got["lo_shift"][5] - lo_law) <= 1.5
    assert (got["flags"][6:] == gpsacq.AIDED_BELOW).all() and pk[6:].tobytes() == bytes(32)
    # downstream, unchanged: refine accepts the merged peaks at snr_min = ratio_min
    fine = eng.refine(w["bits"], pk.copy(), tasks=w["tasks"], params=gpsacq.refine_params(snr_min=aided_ref.RATIO_MIN))
    print("refine at snr_min = ratio_min: flags %s, offset of the weak PRN %.3f chips" % (fine["flags"].tolist(), fine["offset_chips"][5]))
    assert (fine["flags"][:6] == 0).all() and (fine["flags"][6:] == gpsacq.FINE_NO_HIT).all() and fine["prompt"][5] == got["best"][5]
