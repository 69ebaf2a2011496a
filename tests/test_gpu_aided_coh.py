"""Coherent aided acquisition on the GPU (gpsacq_aided_coh_search*, gpsacq_aid_instant*, gpsacq_aided_coh_peaks_device) against
tests/aided_coh_ref.py, the numpy restatement of "Coherent aided acquisition: 20 ms sums, bit edge and fine Doppler" of
include/gpsacq.h.

Every integer field of a record and every entry of powers_out must equal the reference; ratio may differ by RATIO_TOL = 1e-12
relative (one fp64 division), doppler_hz by DOPPLER_TOL = 1e-9 Hz.  Small shapes: fs = 2.046 MHz, spm 2046, 19 segments per block,
random bits (the sums of a random capture are as good as any for equality).  Each test prints what it measured before it asserts
(pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_coh_ref as cr
from coarse_helpers import block_times
from nav_helpers import to_records

pytestmark = pytest.mark.gpu

FS2, FC2, SPM2 = 2.046e6, 0.4e6, 2046


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC2, FS2, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def capture():
    bits = np.random.default_rng(11).integers(0, 256, 5 * 5120, dtype=np.uint8)
    bits.setflags(write=False)
    return bits


def hand_aid(kmax, n, seed):
    """predictions that reach the edges: ca_center in {0, 1, 1000, spm - 1} (the code wrap on both sides) x lo_center in {-kmax, 0,
    +kmax} (invalid d rows at the grid's ends) x PRN 1 and 32, cycled in a seeded order; blocks 0 and 1"""
    import gpsacq
    combos = [(ca, lo, prn) for ca in (0, 1, 1000, SPM2 - 1) for lo in (-kmax, 0, kmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    aid = np.zeros(n, gpsacq.AID_DTYPE)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        aid[t] = (0, ca, lo, 0, ca / FS2, 0.0, 45.0)
        tasks[t] = (t % 2, prn)
    return tasks, aid


def reference(eng, bits, stride, tasks, aid, spm=SPM2, fc=FC2, fs=FS2, **kw):
    step = 0.0 if eng.doppler_sub == 1 and eng.doppler_stride == 1 else eng.doppler_step_hz
    return cr.aided_coh_search(bits, stride, None if tasks is None else tasks.tolist(), aid, spm, fc, fs, eng.kmax, step_hz=step, **kw)


# ---- 1. exact against the reference --------------------------------------------------------------------------------------------
# blocks (S = 19, 39, 58), M, F, u, W, K, stride: S < M and e beyond S (blocks 1, M 20), S no multiple of M (39 and 58 by 20, 4, 5)
CASES = [(1, 1, 0, 1, 0, 0, 5120), (2, 2, 1, 25, 5, 1, 5003), (3, 4, 7, 512, 31, 0, 5120), (1, 5, 1, 1, 5, 1, 5120), (2, 10, 0, 25, 31, 1, 5003),
         (3, 20, 7, 25, 5, 0, 5120), (1, 20, 1, 512, 0, 1, 5003), (2, 20, 1, 25, 5, 1, 5120), (3, 5, 0, 512, 5, 0, 5003), (2, 4, 7, 1, 0, 1, 5120),
         (1, 10, 7, 25, 31, 0, 5120), (3, 2, 1, 1, 5, 1, 5003)]


@pytest.mark.parametrize("blocks,M,F,u,W,K,stride", CASES)
def test_exact_against_the_reference(eng, capture, blocks, M, F, u, W, K, stride):
    import gpsacq
    tasks, aid = hand_aid(eng.kmax, 4, seed=blocks * 1000 + M * 10 + W)
    kw = dict(blocks=blocks, min_segments=20, code_half=W, dop_half=K, coh_ms=M, fine_half=F, fine_step=u, ratio_min=3.0)
    got, pk, pw = eng.aided_coh_search(capture, aid, tasks=tasks, stride=stride, params=gpsacq.aided_coh_params(**kw), powers=True)
    ref = reference(eng, capture, stride, tasks, aid, **kw)
    worst = cr.same(got, ref, pk, pw, "blocks %d M %d F %d u %d W %d K %d stride %d" % (blocks, M, F, u, W, K, stride))
    print("blocks %d (S %d), M %d, F %d, u %d, W %d, K %d, stride %d: 4 records, %d powers and the peaks equal the reference; ratio within %.3g; "
          "flags %s, best_e %s, best_f %s" % (blocks, got["segments"][0], M, F, u, W, K, stride, pw.size, worst, sorted(set(got["flags"].tolist())),
                                              got["best_e"].tolist(), got["best_f"].tolist()))
    assert (got["segments"] == blocks * 40000 // SPM2).all() and (got["n_edge"] == M).all() and (got["n_fine"] == 2 * F + 1).all()
    assert (got["best"] > 0).all() and ((got["flags"] & gpsacq.AIDED_FEW != 0) == (got["segments"] < 20)).all()


def test_a_finer_doppler_grid():
    """gpsacq_set_doppler_step(20.0): an engine of its own; lo_center and doppler_hz count its points"""
    import gpsacq
    with gpsacq.Engine(FC2, FS2, 5000.0) as e:
        e.set_doppler_step(20.0)
        assert e.doppler_sub > 1
        bits = np.random.default_rng(12).integers(0, 256, 3 * 5120, dtype=np.uint8)
        tasks, aid = hand_aid(e.kmax, 3, seed=3)
        kw = dict(blocks=2, min_segments=1, code_half=5, dop_half=1, coh_ms=20, fine_half=2, fine_step=5, ratio_min=0.0)
        got, pk, pw = e.aided_coh_search(bits, aid, tasks=tasks, params=gpsacq.aided_coh_params(**kw), powers=True)
        cr.same(got, reference(e, bits, 5120, tasks, aid, **kw), pk, pw, "finer grid")
        print("step %.3f Hz, kmax %d: 3 records equal the reference; doppler_hz %s" % (e.doppler_step_hz, e.kmax, np.round(got["doppler_hz"], 3).tolist()))


# ---- 2. against the non-coherent kernel ----------------------------------------------------------------------------------------
def test_against_the_aided_search_on_the_device(eng, capture):
    import gpsacq
    tasks, aid = hand_aid(eng.kmax - 1, 6, seed=77)
    W, K = 5, 1
    non, npk, npw = eng.aided_search(capture, aid, tasks=tasks, params=gpsacq.aided_params(blocks=2, code_half=W, dop_half=K, ratio_min=0.0), powers=True)
    one, opk, opw = eng.aided_coh_search(capture, aid, tasks=tasks, powers=True,
                                         params=gpsacq.aided_coh_params(blocks=2, min_segments=1, code_half=W, dop_half=K, coh_ms=1, fine_half=0, ratio_min=0.0))
    assert opw.shape == (6, 3, 1, 1, 11) and np.array_equal(opw[:, :, 0, 0, :], npw)
    for f in ("flags", "segments", "best_h", "best_d", "lo_shift", "ca_shift", "best", "floor", "ratio"):
        assert np.array_equal(one[f], non[f]), f
    assert np.array_equal(one["noncoh"], one["best"]) and opk.tobytes() == npk.tobytes()
    coh, _ = eng.aided_coh_search(capture, aid, tasks=tasks, params=gpsacq.aided_coh_params(blocks=2, min_segments=1, code_half=W, dop_half=K, ratio_min=0.0))
    want = [int(npw[t, coh["best_d"][t], coh["best_h"][t]]) for t in range(6)]
    print("M = 1, F = 0: %d powers equal k_aided's; M = 20: noncoh %s is k_aided's power at (best_h, best_d)" % (npw.size, coh["noncoh"].tolist()))
    assert coh["noncoh"].tolist() == want and (coh["n_edge"] == 20).all()


# ---- 3. flags, edges, argument errors --------------------------------------------------------------------------------------------
def test_flags_and_edges(eng, capture):
    import gpsacq
    import torch
    n_bytes, stride = 15000 + 7 * 256 + 100, 5000  # the window of block 3 holds 7 segments and a tail that ends inside a 32-bit word
    kmax = eng.kmax
    last = (n_bytes * 8) // (8 * stride)  # a block that starts less than one segment before the capture ends
    rows = [(1, 0, 0, 100, 3),        # 0: the whole window
            (3, 0, 0, 0, -kmax),      # 1: SHORT and FEW; one invalid d row
            (2, 31, 0, SPM2 - 1, kmax),  # 2: SHORT
            (4, 0, 0, 7, 0),          # 3: the block starts beyond the capture: NO_AID
            (0, 0, 4, 7, 0),          # 4: a flagged prediction
            (0, 0, 0, SPM2, 0),       # 5
            (0, 32, 0, 7, 0),         # 6
            (0, 5, 0, 1, kmax + 2),   # 7: no Doppler hypothesis on the grid
            (0, 5, 0, 1, kmax + 1),   # 8: one of three on the grid
            (0, 31, 0, 400, -21)]     # 9: kept
    assert last == 3
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    aid = np.zeros(len(rows), gpsacq.AID_DTYPE)
    for t, r in enumerate(rows):
        aid[t] = (r[2], r[3], r[4], 0, 0.0, 0.0, 45.0)
    pin = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    pin["snr"], pin["lo_shift"], pin["ca_shift"], pin["max_pwr"] = 24.99, 5, 6, 7.0
    pin[9] = (25.0, -21, 401, 1234.5)
    kw = dict(blocks=2, min_segments=8, code_half=20, dop_half=1, coh_ms=5, fine_half=1, fine_step=25, ratio_min=1.0)
    prm = gpsacq.aided_coh_params(**kw)
    ref = reference(eng, capture, stride, tasks, aid, peaks_in=pin, n_bytes=n_bytes, **kw)
    assert [r["flags"] & 15 for r in ref] == [0, 4 | 8, 4, 2, 2, 2, 2, 2, 0, 1] and [r["segments"] for r in ref][:3] == [39, 7, 26]
    host, hpk, hpw = eng.aided_coh_search(capture[:n_bytes], aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True)
    worst = cr.same(host, ref, hpk, hpw, "host form")
    for t in range(3, 8):
        assert host[t].tobytes() == np.int32(2).tobytes() + bytes(92) and hpk[t].tobytes() == bytes(16) and not hpw[t].any(), t
    assert host[9].tobytes() == np.int32(1).tobytes() + bytes(92) and hpk[9].tobytes() == pin[9].tobytes() and not hpw[9].any()
    assert not hpw[1][0].any() and hpw[1][1].any() and not hpw[8][1:].any() and hpw[8][0].any() and hpk[1].tobytes() == bytes(16)
    # the device form at an odd address, sentinel bytes of either kind behind the capture, poison behind every output
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_tasks, d_aid, d_pin = dev(tasks), dev(aid), dev(pin)
    n, per = len(rows), 3 * 3 * 5 * 41 * 8
    for sentinel in (0x00, 0xFF):
        buf = np.full(1 + n_bytes + 67, sentinel, np.uint8)
        buf[1:1 + n_bytes] = capture[:n_bytes]
        d_bits = dev(buf)
        d_out, d_pk, d_pw = (torch.full((k,), 0xA5, dtype=torch.uint8, device="cuda:0") for k in ((n + 1) * 96, (n + 1) * 16, (n + 1) * per))
        torch.cuda.synchronize()
        eng.aided_coh_search_device(d_bits.data_ptr() + 1, n_bytes, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), stride=stride,
                                    d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=d_pw.data_ptr(), params=prm, sync=True)
        o = [x.cpu().numpy().tobytes() for x in (d_out, d_pk, d_pw)]
        assert o[0] == host.tobytes() + b"\xa5" * 96 and o[1] == hpk.tobytes() + b"\xa5" * 16 and o[2] == hpw.tobytes() + b"\xa5" * per
    ms = eng.aided_coh_last_ms()
    print("edges: ratio within %.3g; host and device forms agree byte for byte, nothing written beyond the records; k_aided_coh %.4f ms for %d tasks" % (
        worst, ms[2], n))
    assert ms[0] == 0.0 and ms[1] == 0.0 and ms[2] > 0
    # BELOW; the reference schedule and no input peaks
    below, bpk = eng.aided_coh_search(capture[:n_bytes], aid[:3], stride=stride, params=gpsacq.aided_coh_params(**dict(kw, ratio_min=1e9)))
    cr.same(below, reference(eng, capture, stride, None, aid[:3], n_bytes=n_bytes, **dict(kw, ratio_min=1e9)), bpk, None, "schedule")
    assert (below["flags"] & gpsacq.AIDED_BELOW != 0).all() and bpk.tobytes() == bytes(48)
    # NO_POWER: a window without one whole segment; and an all-zero capture, where hypotheses tie: the smallest (d, g, e, h) wins
    tiny = capture[:2000 // 8 + 3]
    none, _ = eng.aided_coh_search(tiny, aid[:1], tasks=np.zeros((1, 2), np.int32), params=gpsacq.aided_coh_params(**dict(kw, ratio_min=0.0)))
    cr.same(none, reference(eng, tiny, 5120, np.zeros((1, 2), np.int32), aid[:1], **dict(kw, ratio_min=0.0)))
    assert none["flags"][0] == gpsacq.AIDED_SHORT | gpsacq.AIDED_FEW | gpsacq.AIDED_NO_POWER and none["segments"][0] == 0
    zeros = np.zeros(2 * 5120, np.uint8)
    tie_aid = aid[[0, 0, 0]].copy()
    tie_aid["lo_center"] = (0, kmax + 1, -kmax - 1)
    tt = np.zeros((3, 2), np.int32)
    tkw = dict(blocks=1, min_segments=1, code_half=2, dop_half=1, coh_ms=20, fine_half=1, fine_step=512, ratio_min=0.0)
    got, gpk, gpw = eng.aided_coh_search(zeros, tie_aid, tasks=tt, params=gpsacq.aided_coh_params(**tkw), powers=True)
    cr.same(got, reference(eng, zeros, 5120, tt, tie_aid, **tkw), gpk, gpw, "tie")
    ties = int((gpw[0] == gpw[0].max()).sum())
    first = min(tuple(int(x) for x in w) for w in zip(*np.nonzero(gpw[0] == gpw[0].max())))  # (d, g, e, h)
    print("all-zero capture: %d hypotheses tie at the largest power; best (d, g, e, h) = %s" % (ties, first))
    assert ties >= 2 and (int(got["best_d"][0]), int(got["best_f"][0]), int(got["best_e"][0]), int(got["best_h"][0])) == first
    assert got["best_d"].tolist()[1:] == [0, 2]
    # UNSUPPORTED at the z matrix's bound: 78 * 63 = 4914 entries run, 97 * 63 = 6111 do not
    big, _ = eng.aided_coh_search(capture, aid[:1], tasks=tasks[:1], params=gpsacq.aided_coh_params(blocks=4, code_half=31, dop_half=0, ratio_min=0.0))
    assert big["segments"][0] == 78
    with pytest.raises(gpsacq.GpsAcqError) as err:
        eng.aided_coh_search(capture, aid[:1], tasks=tasks[:1], params=gpsacq.aided_coh_params(blocks=5, code_half=31))
    assert err.value.code == 3
    # argument errors return 1, launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out, opk = np.zeros(n, gpsacq.AIDED_COH_DTYPE), np.zeros(n, gpsacq.PEAK_DTYPE)
    cap = np.ascontiguousarray(capture[:n_bytes])

    def bad_params(**kv):
        r = gpsacq.aided_coh_params()
        for k, v in kv.items():
            r[k] = v
        return r
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 0
    assert out.tobytes() == host.tobytes() and opk.tobytes() == hpk.tobytes()
    out[:], opk[:] = 0, 0
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(code_half=-1), dict(code_half=32), dict(dop_half=-1), dict(dop_half=9),
               dict(coh_ms=0), dict(coh_ms=3), dict(coh_ms=40), dict(fine_half=-1), dict(fine_half=8), dict(fine_step=0), dict(fine_step=513),
               dict(keep_snr=np.nan), dict(ratio_min=np.inf)):
        assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(bad_params(**kv)), p(out), p(opk), None) == 1, kv
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, 4999, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, None, n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), None, p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, p(cap), 0, stride, p(tasks), p(aid), p(pin), n, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), 0, p(prm), p(out), p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(pin), n, p(prm), None, p(opk), None) == 1
    assert lib.gpsacq_aided_coh_search(h, p(cap), n_bytes, stride, p(tasks), p(aid), p(opk), n, p(prm), p(out), p(opk), None) == 1
    assert not out.view(np.uint8).any() and not opk.view(np.uint8).any()


# ---- 4. the receive instant ------------------------------------------------------------------------------------------------------
def instant_rows(n, seed):
    import gpsacq
    rng = np.random.default_rng(seed)
    fix = np.zeros(n, gpsacq.FIX_DTYPE)
    fix["n_used"], fix["iterations"], fix["rx_ms"] = 7, 5, rng.integers(0, cr.WEEK_MS, n)
    fix["rx_frac"], fix["rms"] = rng.uniform(0, 1e-3, n), rng.uniform(1, 50, n)
    for k in "xyz":
        fix[k] = rng.uniform(-6e6, 6e6, n)
    info = np.zeros(n, gpsacq.COARSE_INFO_DTYPE)
    info["coarse_s"], info["bias_m"] = rng.uniform(-40.0, 40.0, n), rng.uniform(-3e5, 3e5, n)
    prior = np.zeros(n, gpsacq.COARSE_PRIOR_DTYPE)
    prior["rx_ms"] = rng.integers(0, cr.WEEK_MS, n)
    special = [(0.5e-3, 0.0, 100), (1.5e-3, 0.0, 100), (2.5e-3, 0.0, 100), (-0.5e-3, 0.0, 100),  # ties of nearbyint: 0, 2, 2, -0 ms
               (-3.0, 150.0, 5), (2.0, -1.0, cr.WEEK_MS - 1), (0.0, 1.0, 0),  # negative t; across the end and the start of the week
               (np.nan, 0.0, 7), (1.0, np.inf, 7), (3e6, 0.0, 7), (-3e6, 0.0, 7)]  # not finite; k beyond 32 bits
    for i, (s, b, ms) in enumerate(special[:n]):
        info["coarse_s"][i], info["bias_m"][i], prior["rx_ms"][i] = s, b, ms
    if n > len(special) + 2:
        fix["status"][len(special)], fix["status"][len(special) + 1] = 1, 2  # not OK: copied
        fix["rx_frac"][len(special)] = np.nan
    return fix, info, prior


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_aid_instant(eng, n):
    import torch
    fix, info, prior = instant_rows(n, seed=n)
    want = cr.instant(fix, info, prior)
    host = eng.aid_instant(fix, info, prior)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_fix, d_info, d_prior = dev(fix), dev(info), dev(prior)
    d_out = torch.full(((n + 1) * 80,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.aid_instant_device(d_fix.data_ptr(), d_info.data_ptr(), d_prior.data_ptr(), n, d_out.data_ptr())
    ms = eng.aided_coh_last_ms()
    print("%d fixes: statuses %s; rx_ms and rx_frac equal the formula; k_aid_instant %.4f ms" % (n, np.bincount(host["status"], minlength=3).tolist(), ms[0]))
    assert host.tobytes() == want.tobytes()  # every operation is one IEEE operation on both sides: bit for bit
    assert d_out.cpu().numpy().tobytes() == host.tobytes() + b"\xa5" * 80
    assert ms[0] > 0 and ms[1] == 0.0 and ms[2] == 0.0
    if n >= 63:
        assert host["status"][:11].tolist() == [0] * 7 + [2] * 4 and host["rx_ms"][:4].tolist() == [100, 102, 102, 100]
        assert host["rx_ms"][5] == 1999 and host["rx_ms"][6] == cr.WEEK_MS - 1 and host["rx_frac"][6] > 0.99e-3  # t = -3.3 ns: the millisecond before
        assert host[11].tobytes() == fix[11].tobytes() and host[12].tobytes() == fix[12].tobytes()
        for i in (7, 8, 9, 10):  # refused: the fix with another status
            f = fix[i].copy()
            f["status"] = 2
            assert host[i].tobytes() == f.tobytes()
    # in place
    eng.aid_instant_device(d_fix.data_ptr(), d_info.data_ptr(), d_prior.data_ptr(), n, d_fix.data_ptr())
    assert d_fix.cpu().numpy().tobytes() == host.tobytes()
    lib, h, p = eng._lib, eng._h, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(n, fix.dtype)
    assert lib.gpsacq_aid_instant(h, None, p(info), p(prior), n, p(out)) == 1 and lib.gpsacq_aid_instant(h, p(fix), None, p(prior), n, p(out)) == 1
    assert lib.gpsacq_aid_instant(h, p(fix), p(info), None, n, p(out)) == 1 and lib.gpsacq_aid_instant(h, p(fix), p(info), p(prior), 0, p(out)) == 1
    assert lib.gpsacq_aid_instant(h, p(fix), p(info), p(prior), n, None) == 1 and not out.view(np.uint8).any()


# ---- 5. the chain, 6. end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng5():
    import gpsacq
    with gpsacq.Engine(ac.FC, ac.FS, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def weak_scene(eng5):
    """tests/test_aided_coh.py's scene by Engine.generate: 16 blocks at 5.456 MHz, five satellites at 0.2 and one at 0.03 with random
    navigation bits, two absent; block 0 searched for all eight.  The fix is a coarse-time fix's: its own rx_frac is milliseconds
    off, its coarse_info and prior carry the receive instant"""
    import gpsacq
    geo, sel, present, absent, dops = ac.scene_sats(weak=0.03)
    nav = (1 - 2 * np.random.default_rng(5).integers(0, 2, (len(present), 16))).astype(np.int8)
    bits = eng5.generate(16 * 5120, present, noise_sigma=1.0, seed=2024, nav=nav)
    chans = present + absent
    tasks = np.array([(0, s[0] - 1) for s in chans], np.int32)
    _, peaks = eng5.search(bits[:5120], tasks=tasks, want_cells=False)
    bits.setflags(write=False)
    blk_ms, blk_frac = block_times(geo["ref_ms"] + 4321, ac.REF_FRAC, 1, 40960, ac.FS)
    fix = np.zeros(1, gpsacq.FIX_DTYPE)
    fix["n_used"], fix["rx_ms"], fix["rx_frac"] = 8, (int(blk_ms[0]) + 3) % cr.WEEK_MS, 0.4e-3  # the coarse-time fix's own time: 2.8 ms off
    fix["x"], fix["y"], fix["z"] = geo["rx"]
    # the receive instant is prior.rx_ms + coarse_s - bias_m / c: put the true one there
    prior = np.zeros(1, gpsacq.COARSE_PRIOR_DTYPE)
    prior["rx_ms"] = (int(blk_ms[0]) - 17000) % cr.WEEK_MS
    info = np.zeros(1, gpsacq.COARSE_INFO_DTYPE)
    info["coarse_s"], info["bias_m"] = 17.0003, -float(blk_frac[0]) * cr.C_MPS  # nearbyint(1e3 s) = 17000 ms; -b / c = the fraction
    return dict(geo=geo, rec=to_records([geo["ephs"][k] for k in sel]), bits=bits, chans=chans, tasks=tasks, peaks=peaks, fix=fix, info=info,
                prior=prior, blk=(int(blk_ms[0]), float(blk_frac[0])))


def test_chain_and_end_to_end(eng5, weak_scene):
    """Figures are printed by this test; those measured on an MI355X stand in DESIGN.md 8.5."""
    import gpsacq
    import torch
    eng, w = eng5, weak_scene
    n = len(w["chans"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_bits, d_tasks, d_pin = dev(w["bits"]), dev(w["tasks"]), dev(w["peaks"])
    d_fix, d_info, d_prior = dev(w["fix"]), dev(w["info"]), dev(w["prior"])
    nb = w["bits"].size
    # the three calls
    d_fi, d_aid, d_out, d_pk = fill(80), fill(n * 40), fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aid_instant_device(d_fix.data_ptr(), d_info.data_ptr(), d_prior.data_ptr(), 1, d_fi.data_ptr(), sync=False)
    eng.aid_predict_device(w["rec"], d_fi.data_ptr(), 1, n, d_aid.data_ptr(), sync=False)
    eng.aided_coh_search_device(d_bits.data_ptr(), nb, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(),
                                d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    steps = [x.cpu().numpy().tobytes() for x in (d_fi, d_aid, d_out, d_pk)]
    fi = np.frombuffer(steps[0], gpsacq.FIX_DTYPE)
    assert fi["rx_ms"][0] == w["blk"][0] and abs(fi["rx_frac"][0] - w["blk"][1]) < 1e-12 and fi["status"][0] == 0
    # the chain in the caller's buffers, then in engine scratch
    e_fi, e_aid, e_out, e_pk = fill(80), fill(n * 40), fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_coh_peaks_device(w["rec"], d_fix.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, e_out.data_ptr(), e_pk.data_ptr(),
                               d_info_ptr=d_info.data_ptr(), d_prior_ptr=d_prior.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(),
                               d_fix_instant_ptr=e_fi.data_ptr(), d_aid_ptr=e_aid.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (e_fi, e_aid, e_out, e_pk)] == steps
    ms = eng.aided_coh_last_ms()
    f_out, f_pk = fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_coh_peaks_device(w["rec"], d_fix.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, f_out.data_ptr(), f_pk.data_ptr(),
                               d_info_ptr=d_info.data_ptr(), d_prior_ptr=d_prior.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (f_out, f_pk)] == steps[2:]
    # d_info NULL: the fixes as they are -- here the instants made above
    g_out, g_pk = fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_coh_peaks_device(w["rec"], d_fi.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, g_out.data_ptr(), g_pk.data_ptr(),
                               d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (g_out, g_pk)] == steps[2:] and eng.aided_coh_last_ms()[0] == 0.0
    aid = np.frombuffer(steps[1], gpsacq.AID_DTYPE)
    got = np.frombuffer(steps[2], gpsacq.AIDED_COH_DTYPE)
    pk = np.frombuffer(steps[3], gpsacq.PEAK_DTYPE)
    ref = reference(eng, w["bits"], 5120, w["tasks"], aid, spm=ac.SPM, fc=ac.FC, fs=ac.FS, peaks_in=w["peaks"])
    cr.same(got, ref, pk, None, "end to end")
    # today's chain on the same instants does not detect the weak satellite
    n_out, n_pk = fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_peaks_device(w["rec"], d_fi.data_ptr(), d_bits.data_ptr(), nb, d_tasks.data_ptr(), 1, n, n_out.data_ptr(), n_pk.data_ptr(),
                           d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    non = n_out.cpu().numpy().view(gpsacq.AIDED_DTYPE)
    ms_non = eng.aided_last_ms()
    ca_law, _ = ac.law_center(w["chans"][5], 0)
    print("non-coherent: flags %s, ratios %s (ratio_min 1.922); k_aided %.4f ms" % (non["flags"].tolist(), np.round(non["ratio"], 4).tolist(), ms_non[1]))
    print("coherent: flags %s, ratios %s (ratio_min %.2f); weak PRN ca_shift %d (law %.2f), doppler_hz %.1f (generator %.1f), best_e %d; "
          "k_aid_instant %.4f, k_aid_predict %.4f, k_aided_coh %.4f ms for %d tasks, 3 of them searched" % (
              got["flags"].tolist(), np.round(got["ratio"], 4).tolist(), cr.RATIO_MIN, got["ca_shift"][5], ca_law, got["doppler_hz"][5],
              w["chans"][5][2], got["best_e"][5], ms[0], ms[1], ms[2], n))
    assert non["flags"][5] == gpsacq.AIDED_BELOW and (non["flags"][:5] == gpsacq.AIDED_KEPT).all()
    assert (got["flags"][:5] == gpsacq.AIDED_KEPT).all() and pk[:5].tobytes() == w["peaks"][:5].tobytes()
    assert got["flags"][5] == 0 and got["ratio"][5] >= cr.RATIO_MIN
    assert abs((got["ca_shift"][5] - ca_law + ac.SPM / 2) % ac.SPM - ac.SPM / 2) <= 1.0
    assert (got["flags"][6:] == gpsacq.AIDED_BELOW).all() and pk[6:].tobytes() == bytes(32)
    assert min(ms) > 0
    # downstream, unchanged: refine and the coarse-time observations accept the merged peaks at snr_min = 25 (a coherent peak's snr is
    # its ratio, far below 25; ratio_min serves both kinds)
    fine = eng.refine(w["bits"], pk.copy(), tasks=w["tasks"], params=gpsacq.refine_params(snr_min=cr.RATIO_MIN))
    print("refine at snr_min = ratio_min: flags %s, offset of the weak PRN %.3f chips" % (fine["flags"].tolist(), fine["offset_chips"][5]))
    assert (fine["flags"][:6] == 0).all() and (fine["flags"][6:] == gpsacq.FINE_NO_HIT).all()
    d_obs = fill(n * gpsacq.OBS_DTYPE.itemsize)
    d_pk = dev(pk)
    torch.cuda.synchronize()
    eng.coarse_obs_device(d_pk.data_ptr(), 1, n, d_obs.data_ptr(), snr_min=cr.RATIO_MIN)
    obs = d_obs.cpu().numpy().view(gpsacq.OBS_DTYPE)
    assert obs["valid"].tolist() == [1] * 6 + [0] * 2
    # ... and the fix from everything in view: gpsacq_coarse_fix_fine_device (k_refine, k_coarse_obs_fine, k_coarse_fix) on the merged
    # peaks, from a prior 30 km and 30 s off, beside the same chain on the search's own peaks (the five strong satellites: five
    # unknowns, nothing to spare).  THE BOUND.  Every peak is the whole sample nearest its true code phase (asserted above for the
    # weak one; the strong ones are the search's), so every range going in is within half a sample, c / (2 fs) = 27.5 m, and
    # refinement only moves it towards the truth.  The position rows of the least-squares inverse have Frobenius norm pdop (the
    # record's, unweighted), so |error| <= pdop * sqrt(n_used) * 27.5 m whatever the signs of the range errors.
    from coarse_helpers import priors
    prior30 = priors(w["geo"], np.array([w["blk"][0]]), seed=3, km=30.0, secs=30.0)
    d_prior30 = dev(prior30)
    fixes = []
    for d_p, rp in ((d_pk, gpsacq.refine_params(snr_min=cr.RATIO_MIN)), (d_pin, gpsacq.refine_params())):  # the search's peaks at its own 25
        d_fx, d_nf = fill(gpsacq.FIX_DTYPE.itemsize), fill(gpsacq.COARSE_INFO_DTYPE.itemsize)
        torch.cuda.synchronize()
        eng.coarse_fix_fine_device(w["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_p.data_ptr(), 1, n, d_prior30.data_ptr(), d_fx.data_ptr(),
                                   d_nf.data_ptr(), refine_params=rp, sync=True)
        fx, nf = d_fx.cpu().numpy().view(gpsacq.FIX_DTYPE)[0], d_nf.cpu().numpy().view(gpsacq.COARSE_INFO_DTYPE)[0]
        fixes.append((fx, nf, float(np.linalg.norm(np.array([fx["x"], fx["y"], fx["z"]]) - w["geo"]["rx"]))))
    (fx6, nf6, off6), (fx5, nf5, off5) = fixes
    bound = float(nf6["pdop"]) * np.sqrt(6.0) * cr.C_MPS / (2.0 * ac.FS)
    print("coarse-time fix from the merged peaks: status %d, n_used %d, flags %d, rms %.2f m, pdop %.2f, %.2f m from the truth (bound %.1f m); from "
          "the search's five alone: status %d, n_used %d, pdop %.2f, %.2f m" % (fx6["status"], fx6["n_used"], nf6["flags"], fx6["rms"], nf6["pdop"], off6,
                                                                               bound, fx5["status"], fx5["n_used"], nf5["pdop"], off5))
    assert fx6["status"] == gpsacq.FIX_OK and fx6["n_used"] == 6 and nf6["flags"] == 0 and fx5["n_used"] == 5
    assert np.isfinite(nf6["pdop"]) and nf6["pdop"] > 0 and off6 <= bound
