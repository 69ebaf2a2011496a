"""Snapshot signal quality on the GPU (gpsacq_snap_quality*, gpsacq_coarse_fix_quality_device) against tests/snapq_ref.py, the
restatement of "Snapshot signal quality: C/N0 and the weight of a code-phase observation" of include/gpsacq.h.

Every field of an info record must equal the reference byte for byte, except cn0_dbhz, which may differ by snapq_ref.CN0_TOL =
1e-9 dB (log10 is the one libm call).  No capture is read before the chain test; the last two tests make theirs with
Engine.generate.  Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases as ac
import aided_ref
import coarse_raim_ref
import coarse_ref
import nav_ref
import raim_ref
import refine_ref
import snapq_ref as sq
from coarse_helpers import block_times, phases, priors, synth_sats
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu

FS, FC, SPM = 5.456e6, 4.092e6, 5456
SIGMA_M = 3.41  # the fine code-phase sigma at the reference level (README, "Coarse-time fix integrity")


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


# ---- 1. exact against the reference on hand-made records ---------------------------------------------------------------------------
def edge_records(spm):
    """FINE_DTYPE records that reach every edge of the text: prompt 0, floor - 1, floor, floor + 1 and the largest there is,
    2 spm^2 segments, at segments 0, 1, 7, 117 and 2251; every combination of the four GPSACQ_FINE_* flags on a record that would
    otherwise read 43.6 dB-Hz; a negative segment count; the rest of each record is filled so that nothing but flags, segments and
    prompt can matter"""
    import gpsacq
    rows = []
    for segments in (0, 1, 7, 117, 2251):
        floor = 2 * spm * segments
        rows += [(0, segments, p) for p in (0, max(floor - 1, 0), floor, floor + 1, 2 * spm * spm * segments)]
    rows += [(flags, 117, 24 * 2 * spm * 117) for flags in range(16)]
    rows += [(0, -1, 12345), (2, 117, 2 * spm * 117 + 2 * spm * 117 // 2), (0, 117, 2 * spm * 117 + 2 * spm * 117 // 2 - 1)]
    out = np.zeros(len(rows), gpsacq.FINE_DTYPE)
    for i, (flags, segments, prompt) in enumerate(rows):
        out[i] = (flags, segments, 0xDEADBEEF, 0x12345678, prompt // 3, prompt, prompt // 5, 0.125, 0.25e-3)
    return out


def shaped(pool, shape, seed):
    """pool cycled into `shape` from a random start, every third record with a random prompt between 0 and 40 floors"""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    out = pool[(np.arange(n) + rng.integers(0, pool.size)) % pool.size].copy()
    k = np.arange(n) % 3 == 2
    seg = rng.integers(1, 2252, n)
    out["segments"][k] = seg[k]
    out["prompt"][k] = (rng.random(n)[k] * 40 * 2 * SPM * seg[k]).astype(np.uint64)
    out["flags"][k] &= 2
    return out.reshape(shape)


@pytest.mark.parametrize("shape", [(1, 1), (3, 12), (257, 1), (43, 6)])
def test_exact_against_the_reference(eng, shape):
    fine = shaped(edge_records(SPM), shape, seed=shape[0])
    if shape == (1, 1):
        fine[0, 0] = edge_records(SPM)[19]  # segments 117, the largest prompt
    _, got = eng.snap_quality(fine)
    ref = sq.quality(fine, SPM, FS)
    worst = sq.same(got, ref, "shape %s" % (shape,))
    print("shape %s: %d records, flags %s, cn0_dbhz within %.3g dB; k_snap_quality %.4f ms" %
          (shape, fine.size, sorted(set(got["flags"].ravel().tolist())), worst, eng.snap_quality_last_ms()))
    assert eng.snap_quality_last_ms() > 0
    if fine.size >= 36:
        assert {0, sq.NO_POWER, sq.NO_RECORD} <= set(got["flags"].ravel().tolist()) and (got["weight"] == 1.0).any() and ((got["weight"] > 0) & (got["weight"] < 1)).any()


def test_every_edge_record(eng):
    """the whole pool in one row-major array, with min_segments = 8 so that SHORT shows, alone and beside NO_POWER"""
    import gpsacq
    pool = edge_records(SPM)
    fine = pool[:pool.size // 4 * 4].reshape(-1, 4)
    prm = gpsacq.snap_quality_params(min_segments=8)
    _, got = eng.snap_quality(fine, params=prm)
    worst = sq.same(got, sq.quality(fine, SPM, FS, prm), "edges")
    flags = got["flags"].ravel()
    print("%d edge records: flags %s, cn0_dbhz within %.3g dB" % (fine.size, flags.tolist(), worst))
    assert set(flags.tolist()) == {0, sq.NO_POWER, sq.SHORT, sq.SHORT | sq.NO_POWER, sq.NO_RECORD}
    # the 16 flag combinations: usable only without NO_HIT, NO_POWER and FEW, that is 0 and SHORT
    combos = got.ravel()[25:41]
    assert [int(f) for f in combos["flags"]] == [0 if c in (0, 2) else sq.NO_RECORD for c in range(16)]
    assert all(c.tobytes() == np.int32(0).tobytes() + np.int32(32).tobytes() + bytes(40) for k, c in enumerate(combos) if k not in (0, 2))
    # the largest prompt of each segment count reads lin = (spm - 1) fs / spm
    top = got.ravel()[[9, 14, 19, 24]]
    assert (top["lin"] == np.float64(SPM - 1) * np.float64(1000.0)).all() and top["weight"].tolist() == [0.0, 0.0, 1.0, 1.0]


def test_gate_and_reference_level_to_the_ulp(eng):
    """lin exactly at cn0_min_lin and at cn0_ref_lin, and one ulp either side"""
    import gpsacq
    floor = 2 * SPM * 117
    fine = edge_records(SPM)[:1].copy().reshape(1, 1)
    fine["flags"], fine["segments"], fine["prompt"] = 0, 117, floor + 123457
    lin = sq.quality(fine, SPM, FS)["lin"][0, 0]
    assert lin == np.float64(123457.0) / np.float64(floor) * np.float64(1000.0) and 96.0 < lin < 97.0
    up, down = np.nextafter(lin, np.inf), np.nextafter(lin, 0.0)
    seen = []
    for kw, want in ((dict(cn0_min_lin=down), None), (dict(cn0_min_lin=lin), None), (dict(cn0_min_lin=up), 0.0),
                     (dict(cn0_min_lin=0.0, cn0_ref_lin=down), 1.0), (dict(cn0_min_lin=0.0, cn0_ref_lin=lin), 1.0),
                     (dict(cn0_min_lin=0.0, cn0_ref_lin=up), lin / up)):
        prm = gpsacq.snap_quality_params(**kw)
        _, got = eng.snap_quality(fine, params=prm)
        sq.same(got, sq.quality(fine, SPM, FS, prm), str(kw))
        w = got["weight"][0, 0]
        seen.append(float(w))
        assert w == (lin / np.float64(10.0 ** 4.35) if want is None else want), kw
    print("lin %.17g: weights at the gate -1, 0, +1 ulp and at the reference level -1, 0, +1 ulp: %s" % (lin, seen))
    assert seen[0] == seen[1] > 0 and seen[2] == 0 and seen[3] == seen[4] == 1.0 and seen[5] < 1.0


def test_a_rate_that_is_no_multiple_of_a_kilohertz():
    """fs / spm is rounded once: an engine of its own at fs = 5.4561 MHz, 5457 samples per millisecond"""
    import gpsacq
    fs = 5.4561e6
    with gpsacq.Engine(FC, fs, 5000.0) as e:
        assert e.num_lags == 5457
        fine = shaped(edge_records(5457), (5, 7), seed=11)
        _, got = e.snap_quality(fine)
        worst = sq.same(got, sq.quality(fine, 5457, fs), "fs 5.4561 MHz")
        print("fs %.1f Hz, %d samples per millisecond: cn0_dbhz within %.3g dB" % (fs, e.num_lags, worst))
        assert (got["lin"] > 0).any()


# ---- 2. observations, device form, argument errors ---------------------------------------------------------------------------------
def test_observation_rules_and_argument_errors(eng):
    import gpsacq
    import torch
    n, m = 43, 6
    fine = shaped(edge_records(SPM), (n, m), seed=7)
    ref = sq.quality(fine, SPM, FS)
    rng = np.random.default_rng(8)
    obs = np.zeros((n, m), gpsacq.OBS_DTYPE)
    obs["eph"], obs["tx_ms"], obs["reserved"] = rng.integers(0, 12, (n, m)), rng.integers(0, 1000, (n, m)), 77
    obs["tx_frac"], obs["weight"] = rng.random((n, m)) * 1e-3, 1.0
    obs["valid"] = rng.integers(0, 3, (n, m))  # 0, 1 and 2: any nonzero value is valid
    raw = obs.view(np.uint8).reshape(n, m, 32)
    raw[obs["valid"] == 0, 8:] = 0xA5  # rows that are not valid hold 0xA5 everywhere else
    raw[obs["valid"] == 0, 4:8] = 0
    before = obs.copy()
    out, info = eng.snap_quality(fine, obs=obs)
    sq.same(info, ref, "with obs")
    assert obs.tobytes() == before.tobytes()
    valid = before["valid"] != 0
    got_raw, was_raw = out.view(np.uint8).reshape(n, m, 32), before.view(np.uint8).reshape(n, m, 32)
    print("%d observations, %d valid: weights written %d, of them 0: %d" % (n * m, valid.sum(), (out["weight"][valid] != 1.0).sum(), (out["weight"][valid] == 0).sum()))
    assert (got_raw[~valid] == was_raw[~valid]).all() and (got_raw[..., :24] == was_raw[..., :24]).all()
    assert (out["weight"][valid] == ref["weight"][valid]).all() and out.tobytes() == sq.apply_weights(before, ref).tobytes()
    assert valid.sum() > 100 and (~valid).sum() > 50
    # obs = NULL
    none, info2 = eng.snap_quality(fine)
    assert none is None and info2.tobytes() == info.tobytes()
    # the device form at odd-sized, sentinel-framed buffers equals the host form
    lead, tail = 56 * 1, 48 * 1
    d_fine = dev(np.concatenate([np.full(lead, 0x5A, np.uint8), fine.view(np.uint8).reshape(-1), np.full(13, 0x5A, np.uint8)]))
    d_obs = dev(np.concatenate([np.full(32, 0x5A, np.uint8), before.view(np.uint8).reshape(-1), np.full(7, 0x5A, np.uint8)]))
    d_info = fill(tail + n * m * 48 + 5)
    torch.cuda.synchronize()
    eng.snap_quality_device(d_fine.data_ptr() + lead, n, m, d_info.data_ptr() + tail, d_obs_ptr=d_obs.data_ptr() + 32, sync=True)
    h_info, h_obs = d_info.cpu().numpy(), d_obs.cpu().numpy()
    assert (h_info[:tail] == 0xA5).all() and (h_info[tail + n * m * 48:] == 0xA5).all() and h_info[tail:tail + n * m * 48].tobytes() == info.tobytes()
    assert (h_obs[:32] == 0x5A).all() and (h_obs[32 + n * m * 32:] == 0x5A).all() and h_obs[32:32 + n * m * 32].tobytes() == out.tobytes()
    e_info = fill(n * m * 48)
    torch.cuda.synchronize()
    eng.snap_quality_device(d_fine.data_ptr() + lead, n, m, e_info.data_ptr(), sync=True)
    assert e_info.cpu().numpy().tobytes() == info.tobytes()
    # argument errors return 1, launch nothing and write nothing
    lib, h = eng._lib, eng._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h_out, h_ob = np.full(n * m * 48, 0xA5, np.uint8), before.copy()
    g_info, g_obs = fill(n * m * 48), dev(before)
    torch.cuda.synchronize()
    f_ptr = d_fine.data_ptr() + lead
    bad = [dict(min_segments=0), dict(min_segments=-4), dict(cn0_min_lin=-1.0), dict(cn0_min_lin=np.inf), dict(cn0_min_lin=np.nan), dict(cn0_ref_lin=0.0),
           dict(cn0_ref_lin=-3.0), dict(cn0_ref_lin=np.inf), dict(cn0_ref_lin=np.nan)]
    for kw in bad:
        prm = gpsacq.snap_quality_params(**kw)
        assert not sq.params_valid(sq.par(prm)), kw
        assert lib.gpsacq_snap_quality(h, p(fine), n, m, p(prm), p(h_ob), p(h_out)) == 1, kw
        assert lib.gpsacq_snap_quality_device(h, f_ptr, n, m, p(prm), g_obs.data_ptr(), g_info.data_ptr(), 1) == 1, kw
    assert b"cn0_ref_lin" in lib.gpsacq_last_error()
    for args in ((None, n, m), (p(fine), 0, m), (p(fine), n, 0), (p(fine), n, 13), (p(fine), n, -1)):
        assert lib.gpsacq_snap_quality(h, *args, None, p(h_ob), p(h_out)) == 1, args[1:]
    assert lib.gpsacq_snap_quality(h, p(fine), n, m, None, p(h_ob), None) == 1
    for args in ((None, n, m), (f_ptr, 0, m), (f_ptr, n, 0), (f_ptr, n, 13)):
        assert lib.gpsacq_snap_quality_device(h, *args, None, g_obs.data_ptr(), g_info.data_ptr(), 1) == 1, args[1:]
    assert lib.gpsacq_snap_quality_device(h, f_ptr, n, m, None, g_obs.data_ptr(), None, 1) == 1
    eng.synchronize()
    assert (h_out == 0xA5).all() and h_ob.tobytes() == before.tobytes()
    assert (g_info.cpu().numpy() == 0xA5).all() and g_obs.cpu().numpy().tobytes() == before.tobytes()
    # the edges of the ranges are accepted
    for kw in (dict(min_segments=2 ** 31 - 1), dict(cn0_min_lin=0.0), dict(cn0_min_lin=1e300), dict(cn0_ref_lin=1e-300), dict(cn0_ref_lin=1e300)):
        prm = gpsacq.snap_quality_params(**kw)
        assert sq.params_valid(sq.par(prm)), kw
        sq.same(eng.snap_quality(fine, params=prm)[1], sq.quality(fine, SPM, FS, prm), str(kw))


# ---- 3. the chain ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(eng):
    """the scene of tests/test_gpu_refine.py, rebuilt: the northern receiver's eight satellites at amplitude 0.2 in a 19-block
    capture, blocks 0..3 searched"""
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, n_search, spb = 19, 4, 5120 * 8
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3
    sats, dops = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.2)
    bits = eng.generate(n_blocks * 5120, sats, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = np.array([(b, s[0] - 1) for b in range(n_search) for s in sats], np.int32)
    _, peaks = eng.search(bits[:n_search * 5120], tasks=tasks, want_cells=False)
    blk_ms, blk_frac = block_times(ref_ms, ref_frac, n_search, spb, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    bits.setflags(write=False)
    return dict(bits=bits, tasks=tasks, peaks=peaks.reshape(n_search, len(sel)), prior=prior, rec=to_records(ephs))


def test_chain(eng, scene):
    """gpsacq_coarse_fix_quality_device = gpsacq_refine_device, gpsacq_coarse_obs_fine_device, gpsacq_snap_quality_device,
    gpsacq_coarse_fix_batch_device, byte for byte, with and without the optional buffers; the reference level is raised to 46 dB-Hz
    so that the weights are not all 1 and the fixes do depend on them"""
    import gpsacq
    import torch
    n, m = scene["peaks"].shape
    qprm = gpsacq.snap_quality_params(cn0_ref_dbhz=46.0)
    d_bits, d_tasks, d_pk, d_prior = dev(scene["bits"]), dev(scene["tasks"]), dev(scene["peaks"]), dev(scene["prior"])
    nb = scene["bits"].size
    sizes = (n * m * 56, n * m * 32, n * m * 48, n * 80, n * 40, n * m * 32)  # fine, obs, qinfo, fix, info, obs_out
    d_fine, d_obs, d_q, d_fix, d_info, d_out = (fill(s) for s in sizes)
    torch.cuda.synchronize()
    eng.refine_device(d_bits.data_ptr(), nb, d_pk.data_ptr(), n * m, d_fine.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(), sync=False)
    eng.coarse_obs_fine_device(d_pk.data_ptr(), d_fine.data_ptr(), n, m, d_obs.data_ptr(), sync=False)
    eng.snap_quality_device(d_fine.data_ptr(), n, m, d_q.data_ptr(), d_obs_ptr=d_obs.data_ptr(), params=qprm, sync=False)
    eng.coarse_fix_device(scene["rec"], d_obs.data_ptr(), d_prior.data_ptr(), n, m, d_fix.data_ptr(), d_info.data_ptr(), d_out.data_ptr(), sync=True)
    steps = [t.cpu().numpy().tobytes() for t in (d_fine, d_obs, d_q, d_fix, d_info, d_out)]
    fix = np.frombuffer(steps[3], gpsacq.FIX_DTYPE)
    obs = np.frombuffer(steps[1], gpsacq.OBS_DTYPE)
    qinfo = np.frombuffer(steps[2], gpsacq.QUALITY_INFO_DTYPE)
    assert (fix["status"] == 0).all() and (fix["n_used"] == m).all() and (obs["valid"] == 1).all()
    assert (obs["weight"] == qinfo["weight"]).all() and ((obs["weight"] > 0) & (obs["weight"] < 1)).all()
    sq.same(qinfo, sq.quality(np.frombuffer(steps[0], gpsacq.FINE_DTYPE), SPM, FS, qprm), "chain")
    # ... and the fixes are the weighted ones: the unweighted chain gives other bytes
    u_fix, u_info = fill(n * 80), fill(n * 40)
    torch.cuda.synchronize()
    eng.coarse_fix_fine_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), u_fix.data_ptr(),
                               u_info.data_ptr(), sync=True)
    assert u_fix.cpu().numpy().tobytes() != steps[3]
    e = [fill(s) for s in sizes]
    torch.cuda.synchronize()
    eng.coarse_fix_quality_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), e[3].data_ptr(),
                                  e[4].data_ptr(), d_fine_ptr=e[0].data_ptr(), d_obs_ptr=e[1].data_ptr(), d_qinfo_ptr=e[2].data_ptr(),
                                  d_obs_out_ptr=e[5].data_ptr(), quality_params=qprm, sync=True)
    assert [t.cpu().numpy().tobytes() for t in e] == steps
    f_fix, f_info = fill(n * 80), fill(n * 40)
    torch.cuda.synchronize()
    eng.coarse_fix_quality_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), f_fix.data_ptr(),
                                  f_info.data_ptr(), quality_params=qprm, sync=True)
    assert f_fix.cpu().numpy().tobytes() == steps[3] and f_info.cpu().numpy().tobytes() == steps[4]
    # the defaults (quality_params NULL) are the defaults of the separate call
    g_q, g_fix, g_info, h_q = fill(sizes[2]), fill(n * 80), fill(n * 40), fill(sizes[2])
    torch.cuda.synchronize()
    eng.coarse_fix_quality_device(scene["rec"], d_bits.data_ptr(), nb, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, d_prior.data_ptr(), g_fix.data_ptr(),
                                  g_info.data_ptr(), d_qinfo_ptr=g_q.data_ptr(), sync=True)
    eng.snap_quality_device(d_fine.data_ptr(), n, m, h_q.data_ptr(), sync=True)
    assert g_q.cpu().numpy().tobytes() == h_q.cpu().numpy().tobytes()
    ms = eng.refine_last_ms() + (eng.snap_quality_last_ms(),)
    db = qinfo["cn0_dbhz"]
    print("chain: k_refine %.4f ms, k_coarse_obs_fine %.4f ms, k_snap_quality %.4f ms for %d tasks; C/N0 %.2f .. %.2f dB-Hz (median %.2f), weights at a "
          "reference level of 46 dB-Hz %.3f .. %.3f" % (ms[0], ms[1], ms[2], n * m, db.min(), db.max(), np.median(db), obs["weight"].min(), obs["weight"].max()))
    assert ms[2] > 0
    # a bad quality parameter: GPSACQ_ERR_ARG, nothing launched, nothing written
    lib, h = eng._lib, eng._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    z = [fill(s) for s in sizes]
    torch.cuda.synchronize()
    for kw in (dict(min_segments=0), dict(cn0_ref_lin=0.0), dict(cn0_min_lin=np.nan)):
        prm = gpsacq.snap_quality_params(**kw)
        assert lib.gpsacq_coarse_fix_quality_device(h, p(scene["rec"]), m, d_bits.data_ptr(), nb, 5120, d_tasks.data_ptr(), d_pk.data_ptr(), n, m, None, p(prm),
                                                    d_prior.data_ptr(), None, z[0].data_ptr(), z[1].data_ptr(), z[2].data_ptr(), z[3].data_ptr(),
                                                    z[4].data_ptr(), z[5].data_ptr(), 1) == 1, kw
    assert lib.gpsacq_coarse_fix_quality_device(h, p(scene["rec"]), m, d_bits.data_ptr(), nb, 5120, d_tasks.data_ptr(), d_pk.data_ptr(), n, 13, None, None,
                                                d_prior.data_ptr(), None, z[0].data_ptr(), z[1].data_ptr(), z[2].data_ptr(), z[3].data_ptr(), z[4].data_ptr(),
                                                z[5].data_ptr(), 1) == 1
    eng.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in z)


# ---- 4. end to end: five strong satellites and one that only the aided search finds ---------------------------------------------------
# (seed of the capture, the least weight of a strong satellite, the weak satellite's weight) read on the CPU: tests/gen_ref.py makes
# the capture of tests/aided_cases.py's scene with that seed, the strong peaks sit at the sample and bin nearest to the generator's
# law, tests/aided_ref.py finds the weak one, tests/refine_ref.py and tests/snapq_ref.py give the records.  The bands of the test are
# these widened by the factor 1.25 the aided test uses: a peak one sample further from the truth than the CPU's costs up to 0.9 dB.
E2E = [(2024, 0.974, 0.0649), (4, 1.0, 0.0490)]


@pytest.mark.parametrize("seed,strong_w,weak_w", E2E)
def test_end_to_end_weighted_fix(eng, seed, strong_w, weak_w):
    """Search, a fix from the strong five, its receive instant, aided search, all six refined, quality, the weighted fix and its
    integrity.

    On the CPU (tests/gen_ref.py, aided_ref, refine_ref, snapq_ref, coarse_raim_ref with sigma_m = 3.41 m, one degree of freedom,
    threshold 10.83), before any GPU run:
      seed 2024: C/N0 44.11 43.96 43.71 43.39 43.80 and 31.62 dB-Hz, weights 1 1 1 0.974 1 and 0.0649; range errors -4.50 -0.33 -2.54
        0.10 5.45 and 5.91 m; statistic 0.0047 weighted (PASS) against 0.0391 at unit weight; position error 11.61 m weighted,
        11.98 m at unit weight, 11.56 m from the strong five.
      seed 4: C/N0 44.24 43.94 43.53 43.54 43.98 and 30.40 dB-Hz, weights 1 1 1 1 1 and 0.0490; the weak range is 32.7 m off;
        statistic 4.77 weighted (PASS) against 51.47 at unit weight (FAILED, a false alarm by the rule of weight 1); position
        error 2.21 m weighted, 17.89 m at unit weight, 3.23 m from the strong five.
    Of the seeds 2024 and 0 .. 9 every one reads PASS weighted, and the unit-weight statistic is the larger one in all of them.
    Measured on an MI355X (printed by this test): the search puts the fourth strong peak one sample further from the truth than the
    CPU's nearest sample (range error -6.31 / -4.54 m for 0.10 / -0.16 m), so it reads 43.21 / 43.18 dB-Hz and weight 0.935 / 0.930;
    every other C/N0 and the weak weights 0.0649 / 0.0490 are the CPU's to the digit.  Seed 2024: statistic 0.0012 weighted and 0.0097
    at unit weight, both PASS; position error 11.80 m weighted (linear bound 29.34 m), 11.55 m at unit weight, 11.83 m from the strong
    five.  Seed 4: statistic 5.05 weighted (PASS) against 54.45 at unit weight (FAILED); position error 4.90 m weighted (bound
    85.27 m), 16.66 m at unit weight, 6.20 m from the strong five.  The reference's verdicts on the same observations are equal."""
    import gpsacq
    geo, sel, present, absent, dops = ac.scene_sats()
    m = 6
    ephs = [geo["ephs"][k] for k in sel[:m]]
    rec = to_records(ephs)
    bits = eng.generate(16 * 5120, present, noise_sigma=1.0, seed=seed)
    tasks = np.array([(0, s[0] - 1) for s in present], np.int32)
    _, peaks = eng.search(bits[:5120], tasks=tasks, want_cells=False)
    assert (peaks["snr"][:5] >= gpsacq.THRESHOLD).all() and peaks["snr"][5] < gpsacq.THRESHOLD
    blk_ms, blk_frac = block_times(geo["ref_ms"] + 4321, ac.REF_FRAC, 1, 40960, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    # the first fix: the strong five, fine code phases at unit weight (the sixth column is no hit)
    pk1 = peaks.reshape(1, m)
    fine1 = eng.refine(bits, pk1, tasks=tasks)
    fix1, info1, _ = eng.coarse_fix(rec, eng.coarse_obs(pk1, fine=fine1), prior)
    assert fix1["status"][0] == 0 and fix1["n_used"][0] == 5
    # the aided search around the predictions of that fix at its receive instant (gpsacq_aid_instant: good below a sample)
    aid = eng.aid_predict(rec, eng.aid_instant(fix1, info1, prior), m)
    aided, pk = eng.aided_search(bits, aid, tasks=tasks.reshape(1, m, 2), peaks_in=pk1)
    assert (aided["flags"][0, :5] == gpsacq.AIDED_KEPT).all() and aided["flags"][0, 5] == 0 and aided["ratio"][0, 5] >= aided_ref.RATIO_MIN
    # all six refined, the quality of each, the weights
    rprm = gpsacq.refine_params(snr_min=aided_ref.RATIO_MIN)
    fine = eng.refine(bits, pk, tasks=tasks, params=rprm)
    ref_fine = refine_ref.refine(bits, 5120, tasks.tolist(), pk.ravel(), SPM, FC, FS, snr_min=aided_ref.RATIO_MIN)
    refine_ref.same(fine, ref_fine, "fine records")
    obs = eng.coarse_obs(pk, snr_min=aided_ref.RATIO_MIN, fine=fine)
    obs_w, info = eng.snap_quality(fine, obs=obs)
    worst = sq.same(info, sq.quality(ref_fine, SPM, FS).reshape(1, m), "records of the reference on the same bits")
    w = info["weight"][0]
    truth = np.stack([nav_ref.truth_tx(e, geo["rx"], blk_ms, blk_frac) for e in ephs], 1) % 1e-3
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    err = nav_ref.C * wrap(fine["tx_frac"] - truth)
    print("seed %d: search snr %s, aided ratio of the weak PRN %.3f" % (seed, np.round(peaks["snr"], 1), aided["ratio"][0, 5]))
    print("C/N0 %s dB-Hz (equal to the reference's within %.3g dB), weights %s, range errors %s m" %
          (np.round(info["cn0_dbhz"][0], 2), worst, np.round(w, 4), np.round(err[0], 2)))
    assert (info["flags"] == 0).all() and (obs["valid"] == 1).all() and (obs_w["weight"] == info["weight"]).all()
    # the fixes three ways and their integrity
    rp = gpsacq.raim_params(SIGMA_M)
    obs_s = obs.copy()
    obs_s["valid"][0, 5] = 0
    res = {name: eng.coarse_fix_raim(rec, o, prior, rp) for name, o in (("strong five", obs_s), ("unit weight", obs), ("weighted", obs_w))}
    perr = {}
    for name, (fx, _, _, rm) in res.items():
        assert fx["status"][0] == 0, name
        perr[name] = float(np.linalg.norm(np.array([fx["x"][0], fx["y"][0], fx["z"][0]]) - geo["rx"]))
        print("%-12s position error %6.2f m, n_used %d; integrity status %d, statistic %.4f (threshold %.2f)" %
              (name, perr[name], fx["n_used"][0], rm["status"][0], rm["stat_full"][0], rm["threshold"][0]))
    # the linear bound of the weighted fix's own weighted range errors
    exact, _ = phases(geo, sel[:m], blk_ms, blk_frac)
    H = coarse_ref.coarse_fix(geo["ephs"], exact, prior)[0]["H"]
    G = np.linalg.solve(H.T @ (w[:, None] * H), H.T * w)[:3]
    bound = np.linalg.norm(G, 2) * np.linalg.norm(err[0]) * 1.01 + 0.01
    print("linear bound of the weighted fix %.2f m" % bound)
    # the CPU's integrity verdicts of these very observations
    cpu = {name: coarse_raim_ref.coarse_fix_raim(ephs, o, prior, raim_ref.params(SIGMA_M))[0]["raim"] for name, o in (("unit weight", obs), ("weighted", obs_w))}
    print("reference integrity: weighted status %d statistic %.4f, unit weight status %d statistic %.4f" %
          (cpu["weighted"]["status"], cpu["weighted"]["stat_full"], cpu["unit weight"]["status"], cpu["unit weight"]["stat_full"]))
    assert (w[:5] >= strong_w / 1.25).all() and (w[:5] <= 1.0).all()
    assert weak_w / 1.25 <= w[5] <= weak_w * 1.25
    assert perr["weighted"] <= bound
    rm_w, rm_u = res["weighted"][3], res["unit weight"][3]
    assert cpu["weighted"]["status"] == coarse_raim_ref.PASS and cpu["unit weight"]["stat_full"] > cpu["weighted"]["stat_full"]
    assert rm_w["status"][0] == gpsacq.RAIM_PASS and rm_w["dof"][0] == 1
    assert rm_u["stat_full"][0] > rm_w["stat_full"][0]
