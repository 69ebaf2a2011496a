"""Fine code phases on the GPU (gpsacq_refine*, gpsacq_coarse_obs_fine*, gpsacq_coarse_fix_fine_device) against tests/refine_ref.py,
the numpy restatement of "Fine code phases: search peaks refined below a sample" of include/gpsacq.h.

Every integer field of a record (flags, segments, lo_rate, ca_rate, early, prompt, late) must equal the reference; offset_chips
may differ by refine_ref.OFFSET_TOL = 1e-12 chips and tx_frac by refine_ref.TX_FRAC_TOL = 1e-15 s: fp64 rounding of a handful of
operations on values <= 1023, times 10^3.  fs = 5.456 MHz, fc = 4.092 MHz; the bits come from Engine.generate.
Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_ref
import nav_ref
import refine_ref
from coarse_helpers import block_times, phases, priors, synth_sats
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


# ---- 1. exact against the reference --------------------------------------------------------------------------------------------
CASES = [(b, d, s, 33) for b in (1, 2, 3) for d in (1.0 / 64, 0.25, 0.5) for s in (5000, 5003)] + [(2, 0.25, 5003, 1), (2, 0.25, 5000, 5)]


@pytest.mark.parametrize("blocks,d,stride,n_tasks", CASES)
def test_exact_against_the_reference(eng, capture, blocks, d, stride, n_tasks):
    import gpsacq
    tasks, pk = hand_peaks(eng, n_tasks, seed=blocks * 100 + stride)
    got = eng.refine(capture, pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=blocks, half_spacing_chips=d))
    ref = refine_ref.refine(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=blocks, half_spacing_chips=d)
    worst = refine_ref.same(got, ref, "blocks %d d %g stride %d" % (blocks, d, stride))
    print("blocks %d, d %g, stride %d, %d tasks: offset_chips within %.3g, tx_frac within %.3g s" % (blocks, d, stride, n_tasks, worst[0], worst[1]))
    assert (got["flags"] == 0).all() and (got["segments"] == blocks * 40000 // SPM).all()
    if n_tasks == 33:
        assert set(pk["ca_shift"].tolist()) == {0, 1, 2727, SPM - 1} and set(pk["lo_shift"].tolist()) == {-eng.dmax, 0, eng.dmax}
        assert (np.abs(got["offset_chips"]) <= 1.0 - d).all() and got["early"].min() > 0


def grid_words(e):
    """the NCO words of k_refine for every lo_shift of e's grid, against Engine.handoff"""
    import gpsacq
    k = e.kmax
    pk = np.zeros(2 * k + 1, gpsacq.PEAK_DTYPE)
    pk["snr"], pk["lo_shift"], pk["ca_shift"] = 100.0, np.arange(-k, k + 1), 11
    tasks = np.zeros((pk.size, 2), np.int32)
    bits = np.random.default_rng(4).integers(0, 256, 5120, dtype=np.uint8)
    got = e.refine(bits, pk, tasks=tasks, params=gpsacq.refine_params(blocks=1))
    want = [e.handoff(p) for p in pk]
    assert (got["flags"] == 0).all() and (got["segments"] == 7).all()
    assert got["lo_rate"].tolist() == [h["lo_rate"] for h in want] and got["ca_rate"].tolist() == [h["ca_rate"] for h in want]
    return pk.size, got


def test_nco_words_are_the_handoff_words():
    """on the reference grid, then on a finer one (gpsacq_set_doppler_step): an engine of its own, its grid is changed"""
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        n0, g0 = grid_words(e)
        e.set_doppler_step(50.0)
        assert e.doppler_sub == 3
        n1, g1 = grid_words(e)
        print("NCO words equal gpsacq_handoff_engine's on %d and %d grid points" % (n0, n1))
        assert n0 == 2 * e.dmax + 1 and n1 > 2 * n0
        # the same Doppler on both grids is the same frequency only up to the rounding of its two spellings
        assert abs(int(g1["lo_rate"][n1 // 2 + 3]) - int(g0["lo_rate"][n0 // 2 + 1])) <= 1


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
            (0, 5, 40.0, 1, 1)]        # 10: a PRN that is not in the capture: still a record
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    pk = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    for t, r in enumerate(rows):
        pk[t] = (r[2], r[3], r[4], 1.0)
    prm = gpsacq.refine_params(blocks=3, min_segments=3)
    ref = refine_ref.refine(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=3, min_segments=3, n_bytes=n_bytes)
    fit = 3 * 40000 // SPM
    assert [r["flags"] for r in ref] == [0, 2, 2, 2, 1, 1, 1, 1, 1, 1, 0] and [r["segments"] for r in ref][:4] == [fit, 7, 14, 7]
    host = eng.refine(capture[:n_bytes], pk, tasks=tasks, stride=stride, params=prm)
    worst = refine_ref.same(host, ref, "host form")
    for t in (4, 5, 6, 7, 8, 9):
        assert host[t].tobytes() == np.int32(1).tobytes() + bytes(52), t
    # the device form at an odd address, sentinel bytes of either kind behind the capture
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_tasks, d_pk = dev(tasks), dev(pk)
    outs = []
    for sentinel in (0x00, 0xFF):
        buf = np.full(1 + n_bytes + 67, sentinel, np.uint8)
        buf[1:1 + n_bytes] = capture[:n_bytes]
        d_bits = dev(buf)
        d_fine = torch.full((len(rows) * 56,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.refine_device(d_bits.data_ptr() + 1, n_bytes, d_pk.data_ptr(), len(rows), d_fine.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                          params=prm, sync=True)
        outs.append(d_fine.cpu().numpy().tobytes())
    assert outs[0] == host.tobytes() and outs[1] == host.tobytes()
    ms = eng.refine_last_ms()
    print("edges: offset_chips within %.3g, tx_frac within %.3g s; k_refine %.4f ms for %d tasks" % (worst[0], worst[1], ms[0], len(rows)))
    assert ms[0] > 0
    # the reference schedule: tasks == NULL is (block t, PRN t % 32)
    sched = eng.refine(capture[:n_bytes], pk[:4], stride=stride, params=prm)
    refine_ref.same(sched, refine_ref.refine(capture, stride, None, pk[:4], SPM, FC, FS, blocks=3, min_segments=3, n_bytes=n_bytes), "schedule")
    # min_segments above what fits: FEW, and no observation
    few = eng.refine(capture[:n_bytes], pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=3, min_segments=8))
    assert few["flags"].tolist() == [0, 2 | 8, 2, 2 | 8, 1, 1, 1, 1, 1, 1, 0] and (few["segments"] == host["segments"]).all()
    obs = eng.coarse_obs(pk.reshape(1, -1), snr_min=25.0, fine=few.reshape(1, -1))[0]
    plain = eng.coarse_obs(pk.reshape(1, -1), snr_min=25.0)[0]
    assert obs["valid"].tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1] and plain["valid"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    for t in range(len(rows)):
        if obs["valid"][t]:
            assert obs["tx_frac"][t] == few["tx_frac"][t] and obs["eph"][t] == t and obs["weight"][t] == 1.0 and obs["tx_ms"][t] == 0
        else:
            assert obs[t].tobytes() == bytes(32), t
    # argument errors return 1, launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out = np.zeros(len(rows), gpsacq.FINE_DTYPE)
    cap = np.ascontiguousarray(capture[:n_bytes])
    n = len(rows)

    def bad_params(**kw):
        r = gpsacq.refine_params()
        for k, v in kw.items():
            r[k] = v
        return r
    assert lib.gpsacq_refine(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(prm), p(out)) == 0 and out.tobytes() == host.tobytes()
    out[:] = 0
    for kw in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(half_spacing_chips=0.01), dict(half_spacing_chips=0.51),
               dict(half_spacing_chips=np.nan), dict(snr_min=np.inf), dict(snr_min=np.nan)):
        assert lib.gpsacq_refine(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(bad_params(**kw)), p(out)) == 1, kw
    assert lib.gpsacq_refine(h, p(cap), n_bytes, 4999, p(tasks), p(pk), n, p(prm), p(out)) == 1 and b"stride" in lib.gpsacq_last_error()
    assert lib.gpsacq_refine(h, None, n_bytes, stride, p(tasks), p(pk), n, p(prm), p(out)) == 1
    assert lib.gpsacq_refine(h, p(cap), n_bytes, stride, p(tasks), None, n, p(prm), p(out)) == 1
    assert lib.gpsacq_refine(h, p(cap), 0, stride, p(tasks), p(pk), n, p(prm), p(out)) == 1
    assert lib.gpsacq_refine(h, p(cap), n_bytes, stride, p(tasks), p(pk), 0, p(prm), p(out)) == 1
    assert lib.gpsacq_refine(h, p(cap), n_bytes, stride, p(tasks), p(pk), n, p(prm), None) == 1
    ob = np.zeros(n, gpsacq.OBS_DTYPE)
    assert lib.gpsacq_coarse_obs_fine(h, p(pk), None, 1, n, 25.0, p(ob)) == 1 and lib.gpsacq_coarse_obs_fine(h, p(pk), p(few), 1, 13, 25.0, p(ob)) == 1
    assert lib.gpsacq_coarse_obs_fine(h, p(pk), p(few), 1, n, float("nan"), p(ob)) == 1
    assert not out.view(np.uint8).any() and not ob.view(np.uint8).any()


# ---- 3. and 4.: the northern receiver's eight satellites, searched, refined, fixed ------------------------------------------------
@pytest.fixture(scope="module")
def scene(eng):
    """test_end_to_end_from_search_peaks's geometry (tests/test_gpu_coarse.py) with its eight satellites at amplitude 0.2 in a
    19-block capture; blocks 0..3 searched"""
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
                prior=prior, rec=to_records(ephs))


def test_chain(eng, scene):
    """gpsacq_coarse_fix_fine_device = gpsacq_refine_device, gpsacq_coarse_obs_fine_device, gpsacq_coarse_fix_batch_device, byte for
    byte, with and without the optional buffers"""
    import gpsacq
    import torch
    n, m = scene["peaks"].shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_bits, d_tasks, d_pk, d_prior = dev(scene["bits"]), dev(scene["tasks"]), dev(scene["peaks"]), dev(scene["prior"])
    nb = scene["bits"].size
    d_fine, d_obs, d_fix, d_info, d_out = fill(n * m * 56), fill(n * m * 32), fill(n * 80), fill(n * 40), fill(n * m * 32)
    torch.cuda.synchronize()
    eng.refine_device(d_bits.data_ptr(), nb, d_pk.data_ptr(), n * m, d_fine.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(), sync=False)
    eng.coarse_obs_fine_device(d_pk.data_ptr(), d_fine.data_ptr(), n, m, d_obs.data_ptr(), sync=False)
    eng.coarse_fix_device(scene["rec"], d_obs.data_ptr(), d_prior.data_ptr(), n, m, d_fix.data_ptr(), d_info.data_ptr(), d_out.data_ptr(), sync=True)
    steps = [t.cpu().numpy().tobytes() for t in (d_fine, d_obs, d_fix, d_info, d_out)]
    fix = np.frombuffer(steps[2], gpsacq.FIX_DTYPE)
    assert (fix["status"] == 0).all() and (fix["n_used"] == m).all()
    e_fine, e_obs, e_fix, e_info, e_out = fill(n * m * 56), fill(n * m * 32), fill(n * 80), fill(n * 40), fill(n * m * 32)
    torch.cuda.synchronize()
    eng.coarse_fix_fine_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), e_fix.data_ptr(),
                               e_info.data_ptr(), d_fine_ptr=e_fine.data_ptr(), d_obs_ptr=e_obs.data_ptr(), d_obs_out_ptr=e_out.data_ptr(), sync=True)
    assert [t.cpu().numpy().tobytes() for t in (e_fine, e_obs, e_fix, e_info, e_out)] == steps
    f_fix, f_info = fill(n * 80), fill(n * 40)
    torch.cuda.synchronize()
    eng.coarse_fix_fine_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), f_fix.data_ptr(),
                               f_info.data_ptr(), sync=True)
    assert f_fix.cpu().numpy().tobytes() == steps[2] and f_info.cpu().numpy().tobytes() == steps[3]
    ms = eng.refine_last_ms()
    print("chain: k_refine %.4f ms, k_coarse_obs_fine %.4f ms for %d tasks of 16 blocks" % (ms[0], ms[1], n * m))
    assert ms[0] > 0 and ms[1] > 0


def test_end_to_end_fine_fixes(eng, scene):
    """Search peaks refined with the defaults (16 blocks, d = 0.25), then fixes from the fine and from the whole-sample phases.

    Measured on an MI355X (printed by this test): code phase against the truth over the 32 hits, whole-sample 22.20 m rms (worst
    54.65), fine 3.22 m rms (worst 6.93); position error of the four rows, whole-sample fixes 18.6 / 10.6 / 29.2 / 38.2 m, fine fixes
    3.2 / 0.5 / 2.5 / 3.0 m, inside the linear bounds 14.8 / 11.3 / 12.9 / 12.5 m of their own range errors."""
    import gpsacq
    geo, ephs, peaks = scene["geo"], scene["ephs"], scene["peaks"]
    n, m = peaks.shape
    assert (peaks["snr"] >= gpsacq.THRESHOLD).all()
    fine = eng.refine(scene["bits"], peaks, tasks=scene["tasks"])
    ref = refine_ref.refine(scene["bits"], 5120, scene["tasks"].tolist(), peaks, SPM, FC, FS)
    worst = refine_ref.same(fine, ref, "end to end")
    assert (fine["flags"] == 0).all() and (fine["segments"] == 16 * 40000 // SPM).all()
    # code phases against the truth, as ranges
    truth = np.stack([nav_ref.truth_tx(e, geo["rx"], scene["blk_ms"], scene["blk_frac"]) for e in ephs], 1)
    want = truth % 1e-3
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    e_whole = nav_ref.C * wrap(peaks["ca_shift"] / FS - want)
    e_fine = nav_ref.C * wrap(fine["tx_frac"] - want)
    rms_whole, rms_fine = np.sqrt((e_whole ** 2).mean()), np.sqrt((e_fine ** 2).mean())
    print("records equal the reference: offset_chips within %.3g, tx_frac within %.3g s" % (worst[0], worst[1]))
    print("code phase against the truth over %d hits: whole-sample rms %.2f m (worst %.2f), fine rms %.2f m (worst %.2f)" %
          (n * m, rms_whole, np.abs(e_whole).max(), rms_fine, np.abs(e_fine).max()))
    # the fixes of both
    rec = scene["rec"]
    fix_w, info_w, _ = eng.coarse_fix(rec, eng.coarse_obs(peaks), scene["prior"])
    obs_f = eng.coarse_obs(peaks, fine=fine)
    assert (obs_f["valid"] == 1).all() and (obs_f["tx_frac"] == fine["tx_frac"]).all()
    fix_f, info_f, _ = eng.coarse_fix(rec, obs_f, scene["prior"])
    assert (fix_w["status"] == 0).all() and (fix_f["status"] == 0).all() and (fix_f["n_used"] == m).all() and (info_f["flags"] == 0).all()
    err_w = np.linalg.norm(np.stack([fix_w["x"], fix_w["y"], fix_w["z"]], 1) - geo["rx"], axis=1)
    err_f = np.linalg.norm(np.stack([fix_f["x"], fix_f["y"], fix_f["z"]], 1) - geo["rx"], axis=1)
    exact, _ = phases(geo, scene["sel"], scene["blk_ms"], scene["blk_frac"])
    rows = coarse_ref.coarse_fix(geo["ephs"], exact, scene["prior"])
    bound = np.zeros(n)
    for i in range(n):
        H = rows[i]["H"]
        G = np.linalg.solve(H.T @ H, H.T)[:3]
        bound[i] = np.linalg.norm(G, 2) * np.linalg.norm(e_fine[i]) * 1.01 + 0.01
    print("position error, whole-sample fixes %s m, fine fixes %s m (linear bound of each row's range errors %s m)" %
          (np.round(err_w, 1), np.round(err_f, 1), np.round(bound, 1)))
    assert rms_fine < 0.5 * rms_whole
    assert (err_f <= bound).all()
    assert err_f.max() < err_w.max()
