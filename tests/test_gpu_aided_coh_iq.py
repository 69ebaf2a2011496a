"""Coherent aided acquisition on an 8-bit IQ capture on the GPU (gpsacq_aided_coh_search_iq8*, gpsacq_aided_coh_peaks_iq8_device)
against tests/aided_coh_iq_ref.py, the numpy / Python-integer restatement of "Coherent aided acquisition on an 8-bit IQ capture" of
include/gpsacq.h.

Every integer field of a record and every entry of powers_out must equal the reference, peaks byte for byte; ratio may differ by
1e-12 relative (one fp64 division of two integers) and doppler_hz by 1e-9 Hz.  fs = 5.456 MHz, fc = 4.092 MHz; the bytes come from
Engine.generate_iq8 at a residual IF of 2 kHz, so that the hypotheses at -kmax sit at a NEGATIVE carrier.  The reference's segment
sums are its quick spelling (Law.segment_sums_stream), which tests/test_aided_coh_iq.py holds against the sample-by-sample one on the
CPU; its coherent sums are the Python integers except in the two 16-block cases.  Sign mode is held against
gpsacq_iq8_to_bits_device followed by gpsacq_aided_coh_search_device, byte for byte.  At most eight tasks per call.
Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases
import aided_coh_iq_ref as qr
import aided_coh_ref
import aided_iq_cases as ic
from coarse_helpers import block_times, priors
from nav_helpers import to_records

pytestmark = pytest.mark.gpu

FS, FC, SPM, IF_HZ = ic.FS, ic.FC, ic.SPM, 2000.0
REAL, COMPLEX = ic.REAL, ic.COMPLEX


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def capture(eng):
    """seventeen blocks of three satellites at amplitude 0.3 (PRN 1 and 32 among them) with navigation bits, int8, 1.4 MB, made once"""
    sats = [(1, 0.3, 1234.0, 100.25, 0.1), (32, 0.3, -2900.0, 4000.7, 0.4), (17, 0.3, 310.0, 2727.4, 0.7)]
    nav = (1 - 2 * np.random.default_rng(11).integers(0, 2, (3, 16))).astype(np.int8)
    iq = eng.generate_iq8(17 * 40960, sats, if_hz=IF_HZ, scale=16.0, signed=True, noise_sigma=1.0, seed=5, nav=nav)
    iq.setflags(write=False)
    return iq


def inp_of(eng, signed, dc, multibit, if_hz=IF_HZ, fc=FC):
    return eng.iq8_input(signed=signed, remove_dc=dc, mean=ic.MEAN if dc else (0.0, 0.0), mix_hz=ic.mix_of(multibit, if_hz, fc), multibit=multibit)


def aid8(kmax, spm, step_hz, max_block=1):
    """eight hand-made predictions that reach the edges: ca_center 0, 1, spm / 2 - 1 and spm - 1 (base + h crosses spm on both
    sides), lo_center -kmax, 0 and +kmax (invalid d rows at the grid's ends, a negative carrier at -kmax), PRN 1 and 32, blocks 0 ..
    max_block.  Returns (tasks int32 [8][2], aid)"""
    import gpsacq
    combos = [(0, -kmax, 0), (1, 0, 31), (spm // 2 - 1, kmax, 0), (spm - 1, -kmax, 31), (0, kmax, 31), (spm - 1, 0, 0), (1, -kmax, 0), (spm // 2 - 1, 0, 31)]
    aid = np.zeros(8, gpsacq.AID_DTYPE)
    tasks = np.zeros((8, 2), np.int32)
    for t, (ca, lo, prn) in enumerate(combos):
        aid[t] = (0, ca, lo, 0, ca / (spm * 1e3), lo * step_hz, 45.0)
        tasks[t] = (t % (max_block + 1), prn)
    return tasks, aid


def reference(eng, iq, stride, tasks, aid, spm=SPM, fc=FC, fs=FS, **kw):
    step = 0.0 if eng.doppler_sub == 1 and eng.doppler_stride == 1 else eng.doppler_step_hz
    return qr.aided_coh_search(iq, stride, None if tasks is None else tasks.tolist(), aid, spm, fc, fs, eng.kmax, step_hz=step, stream=True, **kw)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


def n_pow(prm):
    r = prm[0]
    return (2 * int(r["dop_half"]) + 1) * (2 * int(r["fine_half"]) + 1) * int(r["coh_ms"]) * (2 * int(r["code_half"]) + 1)


# ---- 1. exact against the reference --------------------------------------------------------------------------------------------
# blocks 3 is 21 segments: one whole 20 ms period and a one-segment tail.  M in {1, 4, 5, 20}, F in {0, 3}, u in {25, 512}, W in
# {0, 2, 16, 31}, K in {0, 1}, three strides, U8 and S8 with and without the mean, REAL and COMPLEX
CASES = [(3, 1, 0, 25, 0, 0, 80000, True, False, REAL), (3, 4, 3, 25, 2, 1, 80016, False, True, COMPLEX), (3, 5, 0, 512, 16, 1, 80000, True, True, REAL),
         (3, 20, 3, 512, 31, 0, 80016, False, False, REAL), (3, 20, 3, 25, 2, 1, 81920, True, False, COMPLEX), (3, 5, 3, 25, 31, 1, 80016, False, True, REAL)]


@pytest.mark.parametrize("blocks,M,F,u,W,K,stride,signed,dc,multibit", CASES)
def test_exact_against_the_reference(eng, capture, blocks, M, F, u, W, K, stride, signed, dc, multibit):
    import gpsacq
    tasks, aid = aid8(eng.kmax, SPM, eng.doppler_step_hz)
    iq = capture if signed else ic.as_u8(capture)
    inp, kw = inp_of(eng, signed, dc, multibit), ic.ref_kw(signed, dc, multibit, IF_HZ)
    pk_ = dict(blocks=blocks, min_segments=20, code_half=W, dop_half=K, coh_ms=M, fine_half=F, fine_step=u, ratio_min=3.0)
    prm = gpsacq.aided_coh_params(**pk_)
    got, pk, pw = eng.aided_coh_search_iq8(iq, inp, aid, tasks=tasks, stride=stride, params=prm, powers=True)
    ref = reference(eng, iq, stride, tasks, aid, **pk_, **kw)
    label = "blocks %d M %d F %d u %d W %d K %d stride %d %s dc %d multibit %d" % (blocks, M, F, u, W, K, stride, "S8" if signed else "U8", dc, multibit)
    worst = qr.same(got, ref, pk, pw, label)
    rows = sum(int(not r["powers"][d].any()) for r in ref for d in range(2 * K + 1))
    wraps = sum(int((int(a["ca_center"]) - W) % SPM + 2 * W >= SPM) for a in aid)
    print("%s: 8 records, %d powers and the peaks equal the reference (%d rows of invalid d, %d tasks across the wrap); ratio within %.3g; flags %s; "
          "best_e %s best_f %s" % (label, pw.size, rows, wraps, worst, sorted(set(got["flags"].tolist())), got["best_e"].tolist(), got["best_f"].tolist()))
    assert pw.shape == (8, 2 * K + 1, 2 * F + 1, M, 2 * W + 1)
    assert (got["segments"] == blocks * 40000 // SPM).all() and (got["n_code"] == 2 * W + 1).all() and (got["n_edge"] == M).all()
    assert not (got["flags"] & ~gpsacq.AIDED_BELOW).any() and (got["best"] > 0).all() and (got["floor"] > 0).all() and (got["noncoh"] > 0).all()
    assert (rows > 0) == (K > 0) and (wraps > 0) == (W > 0)


@pytest.mark.parametrize("dc", [False, True])
def test_the_defaults_on_sixteen_blocks(eng, capture, dc):
    """the default window: 117 segments of 33 code phases, 3 x 7 x 20 hypotheses each; three tasks, one on a satellite in the
    capture at its own code phase and Doppler (detected at the measured default), two elsewhere"""
    import gpsacq
    ca, lo = ic.law_center((17, 0.3, 310.0, 2727.4, 0.7), 0)
    aid = np.zeros(3, gpsacq.AID_DTYPE)
    aid[0] = (0, int(round(ca)) % SPM, int(round(lo)), 0, 0.0, 0.0, 45.0)
    aid[1] = (0, SPM - 3, -eng.kmax, 0, 0.0, 0.0, 45.0)
    aid[2] = (0, 9, eng.kmax, 0, 0.0, 0.0, 45.0)  # PRN 9 is not in the capture
    tasks = np.array([(0, 16), (0, 4), (0, 8)], np.int32)
    iq = capture if not dc else ic.as_u8(capture)
    inp, kw = inp_of(eng, not dc, dc, REAL), ic.ref_kw(not dc, dc, REAL, IF_HZ)
    got, pk, pw = eng.aided_coh_search_iq8(iq, inp, aid, tasks=tasks, powers=True)  # params None: the iq8 defaults
    ref = reference(eng, iq, 81920, tasks, aid, quick=True, **kw)
    worst = qr.same(got, ref, pk, pw, "defaults dc %d" % dc)
    print("defaults, dc %d: ratios %s (ratio_min %.2f), flags %s, best_e %s, doppler_hz %s; ratio within %.3g" % (
        dc, np.round(got["ratio"], 3).tolist(), qr.RATIO_MIN, got["flags"].tolist(), got["best_e"].tolist(), np.round(got["doppler_hz"], 1).tolist(), worst))
    assert pw.shape == (3, 3, 7, 20, 33) and (got["segments"] == 117).all()
    assert got["flags"][0] == 0 and got["ratio"][0] >= qr.RATIO_MIN and pk["snr"][0] > 0 and (got["flags"][1:] == gpsacq.AIDED_BELOW).all()
    assert float(gpsacq.aided_coh_params_iq8()["ratio_min"][0]) == qr.RATIO_MIN


def test_a_second_rate_whose_segment_is_no_multiple_of_the_chunk():
    """fs = 8.184 MHz, fc = 2.046 MHz: spm 8184 = 15 * 512 + 504, the kernel's last chunk of a segment is a short one and no segment
    starts where a chunk does; an engine and a capture of its own"""
    import gpsacq
    fs, fc, spm, if_hz = 8.184e6, 2.046e6, 8184, -1500.0
    with gpsacq.Engine(fc, fs, 5000.0) as e:
        iq = e.generate_iq8(4 * 40960, [(1, 0.3, 800.0, 100.25, 0.1), (32, 0.3, -2100.0, 1500.7, 0.4)], if_hz=if_hz, scale=16.0, signed=False,
                            noise_sigma=1.0, seed=6)
        tasks, aid = aid8(e.kmax, spm, e.doppler_step_hz)
        inp = e.iq8_input(signed=False, remove_dc=True, mean=ic.MEAN, mix_hz=fc - if_hz, multibit=REAL)
        pk_ = dict(blocks=2, min_segments=5, code_half=16, dop_half=1, coh_ms=4, fine_half=1, fine_step=100, ratio_min=2.0)
        got, pk, pw = e.aided_coh_search_iq8(iq, inp, aid, tasks=tasks, stride=80016, params=gpsacq.aided_coh_params(**pk_), powers=True)
        ref = reference(e, iq, 80016, tasks, aid, spm, fc, fs, signed=False, mean=ic.MEAN, mix_hz=fc - if_hz, multibit=REAL, **pk_)
        worst = qr.same(got, ref, pk, pw, "fs 8.184 MHz")
        print("fs 8.184 MHz, spm %d, kmax %d: 8 records and %d powers equal the reference; ratio within %.3g" % (spm, e.kmax, pw.size, worst))
        assert (got["segments"] == 2 * 40000 // spm).all() and spm % 512 != 0 and (got["best"] > 0).all()


# ---- 2. M = 1, F = 0 is the non-coherent search; noncoh for every M ------------------------------------------------------------
def test_against_the_aided_search_iq8_on_the_device(eng, capture):
    import gpsacq
    import torch
    W, K, stride, n = 5, 1, 80016, 8
    tasks, aid = aid8(eng.kmax, SPM, eng.doppler_step_hz)
    inp = inp_of(eng, True, True, REAL)
    d_iq, d_tasks, d_aid = dev(capture), dev(tasks), dev(aid)
    ns = capture.size // 2
    d_non, d_npk, d_npw = fill(n * 64), fill(n * 16), fill(n * 3 * 11 * 8)
    torch.cuda.synchronize()
    eng.aided_search_iq8_device(inp, d_iq.data_ptr(), ns, d_aid.data_ptr(), n, d_non.data_ptr(), d_npk.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                                d_powers_ptr=d_npw.data_ptr(), params=gpsacq.aided_params(blocks=3, code_half=W, dop_half=K, ratio_min=0.0), sync=True)
    non, npw = d_non.cpu().numpy().view(gpsacq.AIDED_DTYPE), d_npw.cpu().numpy().view(np.uint64).reshape(n, 3, 11)
    for M in aided_coh_ref.COH_MS:
        F = 0 if M == 1 else 2
        prm = gpsacq.aided_coh_params(blocks=3, min_segments=1, code_half=W, dop_half=K, coh_ms=M, fine_half=F, fine_step=40, ratio_min=0.0)
        d_out, d_pk, d_pw = fill(n * 96), fill(n * 16), fill(n * n_pow(prm) * 8)
        torch.cuda.synchronize()
        eng.aided_coh_search_iq8_device(inp, d_iq.data_ptr(), ns, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), stride=stride,
                                        d_tasks_ptr=d_tasks.data_ptr(), d_powers_ptr=d_pw.data_ptr(), params=prm, sync=True)
        got = d_out.cpu().numpy().view(gpsacq.AIDED_COH_DTYPE)
        pw = d_pw.cpu().numpy().view(np.uint64).reshape(n, 3, 2 * F + 1, M, 11)
        at = np.array([npw[t, got["best_d"][t], got["best_h"][t]] for t in range(n)], np.uint64)
        print("M %2d F %d: noncoh equals k_aided_iq's power at (best_h, best_d) in %d of %d tasks; floors equal: %s" % (
            M, F, int((got["noncoh"] == at).sum()), n, bool((got["floor"] == non["floor"]).all())))
        assert (got["noncoh"] == at).all() and (got["floor"] == non["floor"]).all() and (got["segments"] == non["segments"]).all()
        if M == 1:
            assert np.array_equal(pw[:, :, 0, 0, :], npw) and (got["best"] == non["best"]).all() and (got["best_h"] == non["best_h"]).all()
            assert (got["best_d"] == non["best_d"]).all() and (got["ratio"] == non["ratio"]).all() and (got["noncoh"] == got["best"]).all()
            assert d_pk.cpu().numpy().tobytes() == d_npk.cpu().numpy().tobytes()


# ---- 3. the rails ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc", [(True, False), (True, True), (False, True)])
def test_the_rails(eng, signed, dc):
    """a noise-free satellite at a scale that drives every byte onto a rail, searched at its own code phase and Doppler, with a mean of
    (128, -128) taken off or none: |v| reaches 256 and the replica lines every sample up, the largest sums the format can carry --
    |I_s| 2^14 is past 32 bits and the power past the 44 bits of the 1-bit kernel's key; all fields against Python integers"""
    import gpsacq
    sat = (5, 1.0, 310.0, 100.25, 0.1)
    nav = (1 - 2 * np.random.default_rng(3).integers(0, 2, (1, 16))).astype(np.int8)
    raw = eng.generate_iq8(3 * 40960, [sat], if_hz=IF_HZ, scale=1e6, signed=True, noise_sigma=0.0, seed=1, nav=nav)
    assert (np.abs(raw.view(np.int8).astype(np.int16)) >= 127).mean() > 0.999
    iq = raw if signed else ic.as_u8(raw)
    ca, lo = ic.law_center(sat, 0)
    aid = np.zeros(2, gpsacq.AID_DTYPE)
    aid[0] = (0, int(round(ca)) % SPM, int(round(lo)), 0, 0.0, 0.0, 45.0)
    aid[1] = (0, (int(round(ca)) + 700) % SPM, int(round(lo)) + 9, 0, 0.0, 0.0, 45.0)  # off the signal: the rails alone
    tasks = np.array([(0, 4), (0, 4)], np.int32)
    mean = (128.0, -128.0) if dc else (0.0, 0.0)
    inp = eng.iq8_input(signed=signed, remove_dc=dc, mean=mean, mix_hz=FC - IF_HZ, multibit=REAL)
    pk_ = dict(blocks=3, min_segments=20, code_half=2, dop_half=1, coh_ms=20, fine_half=1, fine_step=25, ratio_min=0.5)
    got, pk, pw = eng.aided_coh_search_iq8(iq, inp, aid, tasks=tasks, stride=80000, params=gpsacq.aided_coh_params(**pk_), powers=True)
    ref = reference(eng, iq, 80000, tasks, aid, signed=signed, mean=mean if dc else None, mix_hz=FC - IF_HZ, multibit=REAL, **pk_)
    qr.same(got, ref, pk, pw, "rails %s dc %d" % ("S8" if signed else "U8", dc))
    z_top = np.sqrt(float(got["noncoh"][0]) / 21.0)
    print("rails %s dc %d: best 2^%.1f (ratio %.1f), |z| about 2^%.1f per segment, floor %d; off the signal best 2^%.1f" % (
        "S8" if signed else "U8", dc, np.log2(float(got["best"][0])), got["ratio"][0], np.log2(z_top), got["floor"][0], np.log2(float(got["best"][1]))))
    assert got["best"][0] >= 2 ** 44 and z_top * 2 ** 14 >= 2 ** 31 and got["best_h"][0] == 2 and got["flags"][0] == 0
    if dc:
        assert got["floor"][0] > 2 * 21 * SPM * 128 * 128 * 2  # both arms carry more than the format's own 128^2


def test_a_zero_capture(eng):
    import gpsacq
    tasks, aid = aid8(eng.kmax, SPM, eng.doppler_step_hz, max_block=0)
    iq = np.zeros(2 * 40960, np.int8)
    prm = gpsacq.aided_coh_params(blocks=1, min_segments=1, code_half=3, coh_ms=5, fine_half=1)
    got, pk, pw = eng.aided_coh_search_iq8(iq, inp_of(eng, True, False, REAL), aid[:3], tasks=tasks[:3], params=prm, powers=True)
    print("all-zero S8 capture: flags %s floor %s ratio %s" % (got["flags"].tolist(), got["floor"].tolist(), got["ratio"].tolist()))
    assert (got["floor"] == 0).all() and (got["ratio"] == 0.0).all() and (got["flags"] == gpsacq.AIDED_NO_POWER | gpsacq.AIDED_BELOW).all()
    assert (got["segments"] == 7).all() and not pw.any() and pk.tobytes() == bytes(48)
    assert (got["best_h"] == 0).all() and (got["best_f"] == 0).all() and (got["best_e"] == 0).all() and (got["noncoh"] == 0).all()


# ---- 4. flags and edges ----------------------------------------------------------------------------------------------------------
def test_flags_and_edges(eng, capture):
    import gpsacq
    import torch
    stride = 80000
    n_samples = 3 * 40000 + 7 * SPM + 2733  # the window of a task of block 3 ends with the capture, inside a group and a segment
    assert n_samples % 8 == 5 and (n_samples - 3 * 40000) % SPM != 0
    kmax = eng.kmax
    rows = [(1, 0, 0, 100, 3),        # 0: the whole window of 21 segments
            (3, 0, 0, 0, -kmax),      # 1: SHORT and FEW, 7 segments and a tail that ends inside a 16-byte group; one invalid d row; e >= S from 7 on
            (2, 31, 0, 5455, kmax),   # 2: SHORT, 14 segments and a tail: every e beyond 13 leaves one period
            (5, 0, 0, 7, 0),          # 3: the block starts beyond the capture
            (0, 0, 4, 7, 0),          # 4: a flagged prediction
            (0, 5, 0, 1, kmax + 2),   # 5: no Doppler hypothesis on the grid
            (0, 31, 0, 4000, -21),    # 6: kept
            (4, 0, 0, 7, 0)]          # 7: the block starts 925 samples before the end: searched, no segment
    n = len(rows)
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    aid = np.zeros(n, gpsacq.AID_DTYPE)
    for t, r in enumerate(rows):
        aid[t] = (r[2], r[3], r[4], 0, 0.0, 0.0, 45.0)
    pin = np.zeros(n, gpsacq.PEAK_DTYPE)
    pin["snr"], pin["lo_shift"], pin["ca_shift"], pin["max_pwr"] = 24.99, 5, 6, 7.0
    pin[6] = (25.0, -21, 4001, 1234.5)
    kw = dict(blocks=3, min_segments=8, code_half=5, dop_half=1, coh_ms=20, fine_half=1, fine_step=25)
    inp, rkw = inp_of(eng, True, True, REAL), ic.ref_kw(True, True, REAL, IF_HZ)
    first = reference(eng, capture, stride, tasks, aid, peaks_in=pin, n_samples=n_samples, ratio_min=0.0, **kw, **rkw)
    ratio_min = 0.5 * (first[0]["ratio"] + first[2]["ratio"])  # between the two: one of them is BELOW
    ref = reference(eng, capture, stride, tasks, aid, peaks_in=pin, n_samples=n_samples, ratio_min=ratio_min, **kw, **rkw)
    prm = gpsacq.aided_coh_params(ratio_min=ratio_min, **kw)
    assert [r["flags"] & 15 for r in ref] == [0, 4 | 8, 4, 2, 2, 2, 1, 4 | 8] and sorted(r["flags"] & 32 for r in (ref[0], ref[2])) == [0, 32]
    assert [r["segments"] for r in ref][:3] == [21, 7, 14] and ref[7]["flags"] == 4 | 8 | 16 | 32 and ref[7]["floor"] == 0
    cut = np.ascontiguousarray(capture[:2 * n_samples])
    host, hpk, hpw = eng.aided_coh_search_iq8(cut, inp, aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True)
    worst = qr.same(host, ref, hpk, hpw, "host form")
    for t in (3, 4, 5):
        assert host[t].tobytes() == np.int32(2).tobytes() + bytes(92) and hpk[t].tobytes() == bytes(16) and not hpw[t].any(), t
    assert host[6].tobytes() == np.int32(1).tobytes() + bytes(92) and hpk[6].tobytes() == pin[6].tobytes() and not hpw[6].any()
    assert not hpw[1][0].any() and hpw[1][1].any()  # the row of the invalid d is zero
    assert (hpw[1][1][:, 7:, :] == hpw[1][1][:, :1, :]).all() and (hpw[2][1][:, 14:, :] == hpw[2][1][:, :1, :]).all()  # e at or beyond S: the one period [0, S)
    assert hpk[1].tobytes() == bytes(16)  # FEW: measured, and no peak
    assert host["ratio"][7] == 0.0 and host["n_code"][7] == 11 and not hpw[7].any()
    below = 0 if ref[0]["flags"] & 32 else 2
    assert hpk[below].tobytes() == bytes(16) and hpk[2 - below]["snr"] > 0
    # the device form: the capture at the very end of its allocation, then with sentinel bytes of either kind behind it; poisoned outputs
    d_tasks, d_aid, d_pin = dev(tasks), dev(aid), dev(pin)
    front = 2 * 1024 * 1024 - 2 * n_samples
    front -= front % 16  # the device pointer stays 16-byte aligned
    for sentinel in (None, 0x00, 0xFF):
        if sentinel is None:
            buf = np.zeros(front + 2 * n_samples, np.uint8)  # the tensor ends with the capture's last byte
            buf[front:] = cut.view(np.uint8)
            d_all = dev(buf)
            iq_ptr = d_all.data_ptr() + front
        else:
            buf = np.full(2 * n_samples + 150, sentinel, np.uint8)
            buf[:2 * n_samples] = cut.view(np.uint8)
            d_all = dev(buf)
            iq_ptr = d_all.data_ptr()
        assert iq_ptr % 16 == 0
        d_out, d_pk, d_pw = fill((n + 1) * 96), fill((n + 1) * 16), fill((n + 1) * n_pow(prm) * 8)
        torch.cuda.synchronize()
        eng.aided_coh_search_iq8_device(inp, iq_ptr, n_samples, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), stride=stride,
                                        d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=d_pw.data_ptr(), params=prm, sync=True)
        o = [x.cpu().numpy().tobytes() for x in (d_out, d_pk, d_pw)]
        assert o[0] == host.tobytes() + b"\xa5" * 96 and o[1] == hpk.tobytes() + b"\xa5" * 16 and o[2] == hpw.tobytes() + b"\xa5" * (n_pow(prm) * 8), sentinel
    ms = eng.aided_coh_iq8_last_ms()
    print("edges: ratio within %.3g; ratio_min %.3f; host and device forms agree byte for byte, nothing written beyond the records; k_aided_coh_iq %.4f ms "
          "for %d tasks" % (worst, ratio_min, ms[3], n))
    assert ms[0] == 0 and ms[1] == 0 and ms[2] == 0 and ms[3] > 0
    # the reference schedule (tasks == NULL is (block t, PRN t % 32)), and no input peaks: nothing is kept
    sched, spk = eng.aided_coh_search_iq8(cut, inp, aid[:3], stride=stride, params=prm)
    qr.same(sched, reference(eng, capture, stride, None, aid[:3], n_samples=n_samples, ratio_min=ratio_min, **kw, **rkw), spk, None, "schedule")


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(eng, capture):
    import gpsacq
    import torch
    stride, n_samples, n = 80000, 3 * 40960, 6
    tasks, aid = aid8(eng.kmax, SPM, eng.doppler_step_hz)
    tasks, aid = tasks[:n], aid[:n]
    pin = np.zeros(n, gpsacq.PEAK_DTYPE)
    prm = gpsacq.aided_coh_params(blocks=1, min_segments=5, code_half=5, dop_half=1, coh_ms=4, fine_half=1)
    inp = inp_of(eng, True, True, REAL)
    cut = np.ascontiguousarray(capture[:2 * n_samples])
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    ip = ctypes.byref(inp)
    out, opk, opw = np.zeros(n, gpsacq.AIDED_COH_DTYPE), np.zeros(n, gpsacq.PEAK_DTYPE), np.zeros(n * n_pow(prm), np.uint64)
    call = lambda **kv: lib.gpsacq_aided_coh_search_iq8(*[dict(dict(h=h, ip=ip, iq=p(cut), ns=n_samples, stride=stride, tasks=p(tasks), aid=p(aid), pin=p(pin),
                                                                    n=n, prm=p(prm), out=p(out), opk=p(opk), opw=p(opw)), **kv)[k]
                                                          for k in ("h", "ip", "iq", "ns", "stride", "tasks", "aid", "pin", "n", "prm", "out", "opk", "opw")])
    assert call() == 0 and out["n_code"].tolist() == [11] * n and out["n_edge"].tolist() == [4] * n
    out[:], opk[:], opw[:] = 0, 0, 0

    def bad_params(**kv):
        r = gpsacq.aided_coh_params()
        for k, v in kv.items():
            r[k] = v
        return r
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(code_half=-1), dict(code_half=32), dict(dop_half=-1), dict(dop_half=9),
               dict(coh_ms=0), dict(coh_ms=3), dict(coh_ms=8), dict(coh_ms=40), dict(fine_half=-1), dict(fine_half=8), dict(fine_step=0), dict(fine_step=513),
               dict(keep_snr=np.nan), dict(ratio_min=np.inf)):
        keep = bad_params(**kv)
        assert call(prm=p(keep)) == 1, kv
    for bad_stride in (79984, 80008, 2 ** 31 + 16):
        assert call(stride=bad_stride) == 1 and b"stride" in lib.gpsacq_last_error()
    for kv in (dict(h=None), dict(ip=None), dict(iq=None), dict(aid=None), dict(ns=0), dict(n=0), dict(out=None), dict(opk=None), dict(pin=p(opk))):
        assert call(**kv) == 1, kv
    fmt = eng.iq8_input(signed=True, multibit=REAL)
    fmt.format = 2
    for bad in (eng.iq8_input(signed=True, multibit=3), eng.iq8_input(signed=True, multibit=-1), fmt,
                eng.iq8_input(signed=True, remove_dc=True, mean=(200.0, 0.0), multibit=REAL),
                eng.iq8_input(signed=True, remove_dc=True, mean=(0.0, -128.6), multibit=REAL)):
        assert call(ip=ctypes.byref(bad)) == 1
    # GPSACQ_ERR_UNSUPPORTED: the z matrix (469 segments of 63 code phases), in either mode
    big = bad_params(blocks=64, code_half=31)
    assert call(prm=p(big)) == 3 and b"z matrix" in lib.gpsacq_last_error()
    assert call(prm=p(big), ip=ctypes.byref(inp_of(eng, True, False, 0))) == 3
    assert not out.view(np.uint8).any() and not opk.view(np.uint8).any() and not opw.any()
    # the device forms, a misaligned pointer among them, and the chain
    d_iq, d_tasks, d_aid = dev(np.concatenate([cut.view(np.uint8), np.zeros(32, np.uint8)])), dev(tasks), dev(aid)
    d_out, d_pk, d_fix = fill(n * 96), fill(n * 16), dev(np.zeros(1, gpsacq.FIX_DTYPE))
    d_info = dev(np.zeros(1, gpsacq.COARSE_INFO_DTYPE))
    torch.cuda.synchronize()
    args = lambda **kv: dict(dict(inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=n_samples, d_aid_ptr=d_aid.data_ptr(), n_tasks=n, d_aided_ptr=d_out.data_ptr(),
                                  d_peaks_out_ptr=d_pk.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(), params=prm), **kv)
    for kv in (dict(d_iq_ptr=d_iq.data_ptr() + 8), dict(d_iq_ptr=d_iq.data_ptr() + 2), dict(d_iq_ptr=None), dict(stride=80008), dict(n_samples=0),
               dict(n_tasks=0), dict(d_aid_ptr=None), dict(d_aided_ptr=None), dict(d_peaks_out_ptr=None), dict(d_peaks_in_ptr=d_pk.data_ptr()),
               dict(inp=eng.iq8_input(signed=True, multibit=7)), dict(params=bad_params(coh_ms=3))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.aided_coh_search_iq8_device(**args(**kv))
        assert ei.value.code == 1, kv
    with pytest.raises(gpsacq.GpsAcqError) as ei:
        eng.aided_coh_search_iq8_device(**args(params=big))
    assert ei.value.code == 3
    rec = to_records([aided_cases.scene_sats()[0]["ephs"][0]])
    for kv in (dict(d_iq_ptr=d_iq.data_ptr() + 4), dict(d_fix_ptr=None), dict(n_chans=13), dict(stride=80008), dict(inp=eng.iq8_input(signed=True, multibit=7)),
               dict(d_info_ptr=d_info.data_ptr()), dict(params=bad_params(fine_step=0))):  # coarse-time records without their priors
        a = dict(dict(eph=rec, d_fix_ptr=d_fix.data_ptr(), inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=n_samples, d_tasks_ptr=None, n_fix=1, n_chans=1,
                      d_aided_ptr=d_out.data_ptr(), d_peaks_out_ptr=d_pk.data_ptr(), stride=stride), **kv)
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.aided_coh_peaks_iq8_device(**a)
        assert ei.value.code == 1, kv
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_pk.cpu().numpy() == 0xA5).all()
    # an engine that accumulates blocks is refused as gpsacq_aided_search refuses it
    with gpsacq.Engine(FC, FS, 5000.0) as e2:
        e2.set_noncoherent(2)
        with pytest.raises(gpsacq.GpsAcqError) as err:
            e2.aided_coh_search_iq8(cut, inp, aid, tasks=tasks, stride=stride, params=prm)
        assert err.value.code == 3  # GPSACQ_ERR_UNSUPPORTED
        with pytest.raises(gpsacq.GpsAcqError) as err:
            e2.aided_coh_iq8_last_ms()
        assert err.value.code == 1


# ---- 6. sign mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc", [(True, False), (False, True)])
def test_sign_mode_is_the_one_bit_path(eng, capture, signed, dc):
    """GPSACQ_SAMPLES_SIGN = gpsacq_iq8_to_bits_device, then gpsacq_aided_coh_search_device with stride / 16, byte for byte; remove_dc
    with the mean gpsacq_iq8_to_bits_device itself finds; and the reference's sign mode agrees"""
    import gpsacq
    import torch
    iq = np.ascontiguousarray((capture if signed else ic.as_u8(capture))[:2 * 5 * 40960])
    n_samples = iq.size // 2 - 3  # the last byte of the 1-bit stream is not full
    n_bytes = (n_samples + 7) // 8
    n = 8
    tasks, aid = aid8(eng.kmax, SPM, eng.doppler_step_hz)
    pin = np.zeros(n, gpsacq.PEAK_DTYPE)
    pin[5] = (31.0, 4, 77, 9.0)
    stride = 80016
    raw = iq.view(np.int8).astype(np.int64)[:2 * n_samples].reshape(-1, 2) if signed else iq.view(np.uint8).astype(np.int64)[:2 * n_samples].reshape(-1, 2) - 128
    mean = (raw[:, 0].sum() / n_samples, raw[:, 1].sum() / n_samples) if dc else (0.0, 0.0)
    inp = eng.iq8_input(signed=signed, remove_dc=dc, mean=mean, mix_hz=FC - IF_HZ, multibit=0)
    d_iq, d_tasks, d_aid, d_pin = dev(iq), dev(tasks), dev(aid), dev(pin)
    pk_ = dict(blocks=3, min_segments=20, code_half=16, dop_half=1, coh_ms=5, fine_half=1, fine_step=25, ratio_min=4.0)
    prm = gpsacq.aided_coh_params(**pk_)
    n_pw = n * n_pow(prm) * 8
    d_bits, a1, p1, w1, a2, p2, w2 = fill(n_bytes + 16), fill(n * 96), fill(n * 16), fill(n_pw), fill(n * 96), fill(n * 16), fill(n_pw)
    torch.cuda.synchronize()
    rc = eng._lib.gpsacq_iq8_to_bits_device(eng._h, d_iq.data_ptr(), n_samples, 1 if signed else 0, 1 if dc else 0, FC - IF_HZ, 0.0, d_bits.data_ptr(), 1)
    assert rc == 0
    eng.aided_coh_search_device(d_bits.data_ptr(), n_bytes, d_aid.data_ptr(), n, a1.data_ptr(), p1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(),
                                d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=w1.data_ptr(), params=prm)
    eng.aided_coh_search_iq8_device(inp, d_iq.data_ptr(), n_samples, d_aid.data_ptr(), n, a2.data_ptr(), p2.data_ptr(), stride=stride,
                                    d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=w2.data_ptr(), params=prm)
    ms = eng.aided_coh_iq8_last_ms()
    one = [x.cpu().numpy().tobytes() for x in (a1, p1, w1)]
    rec = np.frombuffer(one[0], gpsacq.AIDED_COH_DTYPE)
    print("sign mode %s dc %d: conversion %.4f ms, k_aided_coh %.4f ms; %d records, flags %s" %
          ("S8" if signed else "U8", dc, ms[0], ms[3], rec.size, sorted(set(rec["flags"].tolist()))))
    assert [x.cpu().numpy().tobytes() for x in (a2, p2, w2)] == one
    assert ms[0] > 0 and ms[1] == 0 and ms[2] == 0 and ms[3] > 0 and rec["flags"][5] == gpsacq.AIDED_KEPT and (rec["floor"][rec["flags"] != 1] == 2 * SPM * 21).all()
    host, hpk, hpw = eng.aided_coh_search_iq8(iq, inp, aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True, n_samples=n_samples)
    assert [host.tobytes(), hpk.tobytes(), hpw.tobytes()] == one
    ref = reference(eng, iq, stride, tasks, aid, peaks_in=pin, n_samples=n_samples, signed=signed, mean=mean if dc else None, mix_hz=FC - IF_HZ, multibit=0, **pk_)
    qr.same(host, ref, hpk, hpw, "sign mode")
    # params == NULL in sign mode are gpsacq_aided_coh_default_params (ratio_min 10.73), not the multi-bit path's; three tasks of 16 blocks
    b1, q1, b2, q2 = fill(3 * 96), fill(3 * 16), fill(3 * 96), fill(3 * 16)
    torch.cuda.synchronize()
    eng.aided_coh_search_device(d_bits.data_ptr(), n_bytes, d_aid.data_ptr(), 3, b1.data_ptr(), q1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(),
                                d_peaks_in_ptr=d_pin.data_ptr())
    eng.aided_coh_search_iq8_device(inp, d_iq.data_ptr(), n_samples, d_aid.data_ptr(), 3, b2.data_ptr(), q2.data_ptr(), stride=stride,
                                    d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr())
    assert b2.cpu().numpy().tobytes() == b1.cpu().numpy().tobytes() and q2.cpu().numpy().tobytes() == q1.cpu().numpy().tobytes()


# ---- 7. the chain, end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weak_scene(eng):
    """tests/test_aided_coh.py's scene as a 16-block IQ capture by Engine.generate_iq8 (IF 0.4 MHz, scale 16, sigma 1, int8): five
    satellites at 0.2 and one at aided_iq_cases.WEAK_AMPLITUDE with random navigation bits, two absent; block 0 searched for all
    eight in multi-bit mode.  The fix is a coarse-time fix's: its own rx_frac is milliseconds off, its coarse_info and prior carry the
    receive instant"""
    import gpsacq
    geo, sel, present, absent, dops = aided_cases.scene_sats(weak=ic.WEAK_AMPLITUDE)
    nav = (1 - 2 * np.random.default_rng(5).integers(0, 2, (len(present), 16))).astype(np.int8)
    iq = eng.generate_iq8(16 * 40960, present, if_hz=ic.IF_HZ, scale=ic.SCALE, signed=True, noise_sigma=1.0, seed=2024, nav=nav)
    chans = present + absent
    tasks = np.array([(0, s[0] - 1) for s in chans], np.int32)
    inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=FC - ic.IF_HZ, multibit=REAL)
    _, peaks = eng.search_iq8(iq[:2 * 40960], inp, tasks=tasks, want_cells=False)
    iq.setflags(write=False)
    blk_ms, blk_frac = block_times(geo["ref_ms"] + 4321, aided_cases.REF_FRAC, 1, 40960, FS)
    fix = np.zeros(1, gpsacq.FIX_DTYPE)
    fix["n_used"], fix["rx_ms"], fix["rx_frac"] = 8, (int(blk_ms[0]) + 3) % aided_coh_ref.WEEK_MS, 0.4e-3  # the coarse-time fix's own time: 2.8 ms off
    fix["x"], fix["y"], fix["z"] = geo["rx"]
    prior = np.zeros(1, gpsacq.COARSE_PRIOR_DTYPE)  # the receive instant is prior.rx_ms + coarse_s - bias_m / c: put the true one there
    prior["rx_ms"] = (int(blk_ms[0]) - 17000) % aided_coh_ref.WEEK_MS
    info = np.zeros(1, gpsacq.COARSE_INFO_DTYPE)
    info["coarse_s"], info["bias_m"] = 17.0003, -float(blk_frac[0]) * aided_coh_ref.C_MPS
    return dict(geo=geo, rec=to_records([geo["ephs"][k] for k in sel]), iq=iq, inp=inp, chans=chans, tasks=tasks, peaks=peaks, fix=fix, info=info, prior=prior,
                blk=(int(blk_ms[0]), float(blk_frac[0])))


def test_chain_and_end_to_end(eng, weak_scene):
    """gpsacq_aided_coh_peaks_iq8_device = gpsacq_aid_instant_device + gpsacq_aid_predict_device + gpsacq_aided_coh_search_iq8_device byte
    for byte, in the caller's buffers, in engine scratch and with d_info NULL; host form = device form; the records equal the
    reference.  Then the scene: the weak satellite, below the search threshold in block 0, is found with the defaults at its true
    code phase, the absent PRNs are not, and the merged peaks go through gpsacq_coarse_fix_fine_iq8_device to a fix within
    pdop * sqrt(n) * half a sample of range.

    Measured on an MI355X (printed by this test): the search of block 0 gives the five strong satellites snr 166 to 249, the weak one
    (amplitude 0.04) 13.73 and the absent ones 15.24 and 12.92.  The coherent multi-bit search keeps the five, finds the weak one at
    ratio 40.7864 (ratio_min 28.56), ca_shift 4627 against the law's 4626.77, 384.8 Hz against the generator's 389.8, best_e 7, and
    reads the absent ones at 3.344 and 7.349 -- the CPU's figures for tests/gen_ref.py's capture.  k_aid_instant 0.007 ms,
    k_aid_predict 0.027 ms, k_aided_coh_iq 4.41 ms for the 8 tasks, 3 of them searched; the fix from six satellites lies 2.73 m from
    the truth (pdop 2.84, bound 190.9 m)."""
    import gpsacq
    import torch
    w = weak_scene
    n = len(w["chans"])
    ns = w["iq"].size // 2
    d_iq, d_tasks, d_pin = dev(w["iq"]), dev(w["tasks"]), dev(w["peaks"])
    d_fix, d_info, d_prior = dev(w["fix"]), dev(w["info"]), dev(w["prior"])
    d_fi, d_aid, d_out, d_pk = fill(80), fill(n * 40), fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aid_instant_device(d_fix.data_ptr(), d_info.data_ptr(), d_prior.data_ptr(), 1, d_fi.data_ptr(), sync=False)
    eng.aid_predict_device(w["rec"], d_fi.data_ptr(), 1, n, d_aid.data_ptr(), sync=False)
    eng.aided_coh_search_iq8_device(w["inp"], d_iq.data_ptr(), ns, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(),
                                    d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    steps = [x.cpu().numpy().tobytes() for x in (d_fi, d_aid, d_out, d_pk)]
    fi = np.frombuffer(steps[0], gpsacq.FIX_DTYPE)
    assert fi["rx_ms"][0] == w["blk"][0] and abs(fi["rx_frac"][0] - w["blk"][1]) < 1e-12 and fi["status"][0] == 0
    e_fi, e_aid, e_out, e_pk = fill(80), fill(n * 40), fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_coh_peaks_iq8_device(w["rec"], d_fix.data_ptr(), w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), 1, n, e_out.data_ptr(), e_pk.data_ptr(),
                                   d_info_ptr=d_info.data_ptr(), d_prior_ptr=d_prior.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(),
                                   d_fix_instant_ptr=e_fi.data_ptr(), d_aid_ptr=e_aid.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (e_fi, e_aid, e_out, e_pk)] == steps
    ms = eng.aided_coh_iq8_last_ms()
    f_out, f_pk = fill(n * 96), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_coh_peaks_iq8_device(w["rec"], d_fix.data_ptr(), w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), 1, n, f_out.data_ptr(), f_pk.data_ptr(),
                                   d_info_ptr=d_info.data_ptr(), d_prior_ptr=d_prior.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (f_out, f_pk)] == steps[2:]
    g_out, g_pk = fill(n * 96), fill(n * 16)  # d_info NULL: the fixes as they are -- here the instants made above
    torch.cuda.synchronize()
    eng.aided_coh_peaks_iq8_device(w["rec"], d_fi.data_ptr(), w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), 1, n, g_out.data_ptr(), g_pk.data_ptr(),
                                   d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (g_out, g_pk)] == steps[2:] and eng.aided_coh_iq8_last_ms()[1] == 0.0
    aid = np.frombuffer(steps[1], gpsacq.AID_DTYPE)
    got = np.frombuffer(steps[2], gpsacq.AIDED_COH_DTYPE)
    pk = np.frombuffer(steps[3], gpsacq.PEAK_DTYPE)
    host, hpk = eng.aided_coh_search_iq8(w["iq"], w["inp"], aid, tasks=w["tasks"], peaks_in=w["peaks"])  # params None: the iq8 defaults
    assert host.tobytes() == steps[2] and hpk.tobytes() == steps[3]
    ref = reference(eng, w["iq"], 81920, w["tasks"], aid, peaks_in=w["peaks"], signed=True, mix_hz=FC - ic.IF_HZ, multibit=REAL, quick=True)
    qr.same(got, ref, pk, None, "end to end")
    snr = w["peaks"]["snr"]
    ca_law, lo_law = aided_cases.law_center(w["chans"][5], 0)
    print("search snr of block 0: strong %s, weak %.2f, absent %.2f %.2f" % (np.round(snr[:5], 1), snr[5], snr[6], snr[7]))
    print("coherent, multi-bit: flags %s, ratios %s (ratio_min %.2f); weak PRN (amplitude %g) at ca_shift %d (law %.2f), doppler_hz %.1f (generator %.1f), "
          "best_e %d; k_aid_instant %.4f, k_aid_predict %.4f, k_aided_coh_iq %.4f ms for %d tasks, 3 of them searched" % (
              got["flags"].tolist(), np.round(got["ratio"], 4).tolist(), qr.RATIO_MIN, ic.WEAK_AMPLITUDE, got["ca_shift"][5], ca_law, got["doppler_hz"][5],
              w["chans"][5][2], got["best_e"][5], ms[1], ms[2], ms[3], n))
    assert ms[0] == 0 and min(ms[1:]) > 0
    assert (snr[:5] >= gpsacq.THRESHOLD).all() and snr[5] < gpsacq.THRESHOLD
    assert (got["flags"][:5] == gpsacq.AIDED_KEPT).all() and pk[:5].tobytes() == w["peaks"][:5].tobytes()
    assert got["flags"][5] == 0 and got["ratio"][5] >= qr.RATIO_MIN
    assert abs((got["ca_shift"][5] - ca_law + SPM / 2) % SPM - SPM / 2) <= 1.0
    assert abs(got["doppler_hz"][5] - w["chans"][5][2]) <= 25 / 1024.0 * (FS / SPM)  # within a fine step of the generator's Doppler
    assert (got["flags"][6:] == gpsacq.AIDED_BELOW).all() and pk[6:].tobytes() == bytes(32)
    # downstream: gpsacq_coarse_fix_fine_iq8_device (k_refine_iq, k_coarse_obs_fine, k_coarse_fix) on the merged peaks, from a prior 30 km
    # and 30 s off.  THE BOUND is tests/test_gpu_aided_coh.py's: every peak is the whole sample nearest its true code phase, so every
    # range going in is within half a sample, c / (2 fs) = 27.5 m; the position rows of the least-squares inverse have Frobenius norm
    # pdop, so |error| <= pdop * sqrt(n_used) * 27.5 m whatever the signs of the range errors
    prior30 = priors(w["geo"], np.array([w["blk"][0]]), seed=3, km=30.0, secs=30.0)
    d_prior30, d_mpk = dev(prior30), dev(pk)
    d_fx, d_nf = fill(gpsacq.FIX_DTYPE.itemsize), fill(gpsacq.COARSE_INFO_DTYPE.itemsize)
    torch.cuda.synchronize()
    eng.coarse_fix_fine_iq8_device(w["rec"], w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), d_mpk.data_ptr(), 1, n, d_prior30.data_ptr(), d_fx.data_ptr(),
                                   d_nf.data_ptr(), refine_params=gpsacq.refine_params(snr_min=qr.RATIO_MIN), sync=True)
    fx, nf = d_fx.cpu().numpy().view(gpsacq.FIX_DTYPE)[0], d_nf.cpu().numpy().view(gpsacq.COARSE_INFO_DTYPE)[0]
    off = float(np.linalg.norm(np.array([fx["x"], fx["y"], fx["z"]]) - w["geo"]["rx"]))
    bound = float(nf["pdop"]) * np.sqrt(6.0) * aided_coh_ref.C_MPS / (2.0 * FS)
    print("coarse-time fix from the merged peaks: status %d, n_used %d, flags %d, rms %.2f m, pdop %.2f, %.2f m from the truth (bound %.1f m)" % (
        fx["status"], fx["n_used"], nf["flags"], fx["rms"], nf["pdop"], off, bound))
    assert fx["status"] == gpsacq.FIX_OK and fx["n_used"] == 6 and nf["flags"] == 0
    assert np.isfinite(nf["pdop"]) and nf["pdop"] > 0 and off <= bound
