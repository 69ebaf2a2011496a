"""The snapshot chain on an 8-bit IQ capture on the GPU (gpsacq_refine_iq8*, gpsacq_fine_doppler_iq8*, gpsacq_coarse_fix_fine_iq8_device,
gpsacq_cold_fix_iq8_device) against tests/refine_iq_ref.py and tests/dop_iq_ref.py, the numpy restatements of "Snapshot chain on an
8-bit IQ capture" of include/gpsacq.h.

Every integer field of a record must equal the reference; offset_chips, tx_frac, coherence, df_hz and doppler_hz lie within the
tolerances tests/refine_ref.py and tests/dop_ref.py already carry (OFFSET_TOL, TX_FRAC_TOL, COHERENCE_TOL, DF_TOL).  fs = 5.456 MHz,
fc = 4.092 MHz; the bytes come from Engine.generate_iq8 at a residual IF of 2 kHz, so that the hits at -dmax sit at a NEGATIVE
carrier.  Sign mode is held against gpsacq_iq8_to_bits_device followed by the 1-bit kernels, byte for byte.
Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_ref
import dop_iq_ref
import dop_ref
import nav_ref
import refine_iq_ref
import refine_ref
from coarse_helpers import block_times, phases, priors, synth_sats
from nav_helpers import geometry, to_records

pytestmark = pytest.mark.gpu

FS, FC, SPM, IF_HZ = 5.456e6, 4.092e6, 5456, 2000.0
REAL, COMPLEX = 1, 2
MEAN = (3.4, -2.6)


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(FC, FS, 5000.0) as e:
        yield e


@pytest.fixture(scope="module")
def capture(eng):
    """four blocks of three satellites at amplitude 0.3 (PRN 1 and 32 among them), int8, about 330 KB, made once"""
    sats = [(1, 0.3, 1234.0, 100.25, 0.1), (32, 0.3, -2900.0, 4000.7, 0.4), (17, 0.3, 310.0, 2727.4, 0.7)]
    iq = eng.generate_iq8(4 * 40960 + 1000, sats, if_hz=IF_HZ, scale=16.0, signed=True, noise_sigma=1.0, seed=5)
    iq.setflags(write=False)
    return iq


def as_u8(iq):
    return (iq.astype(np.int16) + 128).astype(np.uint8)


def mix_of(multibit, if_hz=IF_HZ, fc=FC):
    """the mix_hz with which a search of the capture reports lo_shift = round(doppler * 40000 / fs)"""
    return -if_hz if multibit == COMPLEX else fc - if_hz


def inp_of(eng, signed, dc, multibit, if_hz=IF_HZ, fc=FC):
    return eng.iq8_input(signed=signed, remove_dc=dc, mean=MEAN if dc else (0.0, 0.0), mix_hz=mix_of(multibit, if_hz, fc), multibit=multibit)


def ref_kw(signed, dc, multibit, if_hz=IF_HZ, fc=FC):
    return dict(signed=signed, mean=MEAN if dc else None, mix_hz=mix_of(multibit, if_hz, fc), multibit=multibit)


def hand_peaks(dmax, spm, n, seed, max_block=1):
    """n hand-made hits that reach the edges whatever a search would find: ca_shift in {0, 1, 2727, spm - 1} x lo_shift in {-dmax, 0,
    +dmax} x PRN 1 and 32 (24 combinations, cycled), blocks 0 .. max_block"""
    import gpsacq
    combos = [(ca, lo, prn) for ca in (0, 1, 2727, spm - 1) for lo in (-dmax, 0, dmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    pk = np.zeros(n, gpsacq.PEAK_DTYPE)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        pk[t] = (30.0 + t, lo, ca, 1.0)
        tasks[t] = (t % (max_block + 1), prn)
    return tasks, pk


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


# ---- 1. exact against the references -------------------------------------------------------------------------------------------
# blocks x d x stride, all 27; format, remove_dc and REAL / COMPLEX go through their eight combinations along the list, three times and
# more each; then one task and five tasks (fewer tasks than waves' worth of work)
_MODES = [(signed, dc, mb) for signed in (True, False) for dc in (False, True) for mb in (REAL, COMPLEX)]
CASES = [(b, d, s, 24) + _MODES[(9 * i + 3 * j + k) % 8] for i, b in enumerate((1, 2, 3)) for j, d in enumerate((1.0 / 64, 0.25, 0.5))
         for k, s in enumerate((80000, 80016, 81920))] + [(2, 0.25, 80016, 1, False, True, REAL), (2, 0.25, 81920, 5, True, True, COMPLEX)]


@pytest.mark.parametrize("blocks,d,stride,n_tasks,signed,dc,multibit", CASES)
def test_exact_against_the_references(eng, capture, blocks, d, stride, n_tasks, signed, dc, multibit):
    import gpsacq
    tasks, pk = hand_peaks(eng.dmax, SPM, n_tasks, seed=blocks * 100 + stride)
    iq = capture if signed else as_u8(capture)
    inp, kw = inp_of(eng, signed, dc, multibit), ref_kw(signed, dc, multibit)
    got = eng.refine_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=blocks, half_spacing_chips=d))
    ref = refine_iq_ref.refine(iq, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=blocks, half_spacing_chips=d, **kw)
    label = "blocks %d d %g stride %d %s dc %d multibit %d" % (blocks, d, stride, "S8" if signed else "U8", dc, multibit)
    worst = refine_ref.same(got, ref, label)
    dgot = eng.fine_doppler_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=gpsacq.dopfine_params(blocks=blocks))
    dref = dop_iq_ref.fine_doppler(iq, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=blocks, **kw)
    dworst = dop_ref.same(dgot, dref, label)
    print("%s, %d tasks: offset_chips within %.3g, tx_frac within %.3g s, coherence within %.3g, df_hz within %.3g, doppler_hz within %.3g Hz; k %s" %
          (label, n_tasks, worst[0], worst[1], dworst[0], dworst[1], dworst[2], sorted({r["k"] for r in dref})))
    assert (got["flags"] == 0).all() and (got["segments"] == blocks * 40000 // SPM).all() and (dgot["flags"] == 0).all()
    if n_tasks == 24:
        assert set(pk["ca_shift"].tolist()) == {0, 1, 2727, SPM - 1} and set(pk["lo_shift"].tolist()) == {-eng.dmax, 0, eng.dmax}
        assert (got["lo_rate"] >= 2 ** 31).any() and (got["lo_rate"] < 2 ** 31).any()  # a negative f is among them
        assert (np.abs(got["offset_chips"]) <= 1.0 - d).all() and got["early"].min() > 0


def test_a_second_rate():
    """fs = 2.8 MHz, fc = 0.7 MHz (spm 2800): one case, an engine and a capture of its own"""
    import gpsacq
    fs, fc, spm, if_hz = 2.8e6, 0.7e6, 2800, -1500.0
    with gpsacq.Engine(fc, fs, 5000.0) as e:
        iq = e.generate_iq8(3 * 40960, [(1, 0.3, 800.0, 100.25, 0.1), (32, 0.3, -2100.0, 1500.7, 0.4)], if_hz=if_hz, scale=16.0, signed=False,
                            noise_sigma=1.0, seed=6)
        combos = [(ca, lo, prn) for ca in (0, 1, 2727, spm - 1) for lo in (-e.dmax, 0, e.dmax) for prn in (0, 31)]
        pk = np.zeros(len(combos), gpsacq.PEAK_DTYPE)
        tasks = np.zeros((len(combos), 2), np.int32)
        for t, (ca, lo, prn) in enumerate(combos):
            pk[t], tasks[t] = (40.0, lo, ca, 1.0), (t % 2, prn)
        inp = e.iq8_input(signed=False, remove_dc=True, mean=MEAN, mix_hz=fc - if_hz, multibit=REAL)
        kw = dict(signed=False, mean=MEAN, mix_hz=fc - if_hz, multibit=REAL)
        got = e.refine_iq8(iq, inp, pk, tasks=tasks, stride=80016, params=gpsacq.refine_params(blocks=2, half_spacing_chips=0.25))
        worst = refine_ref.same(got, refine_iq_ref.refine(iq, 80016, tasks.tolist(), pk, spm, fc, fs, blocks=2, **kw), "fs 2.8 MHz")
        dgot = e.fine_doppler_iq8(iq, inp, pk, tasks=tasks, stride=80016, params=gpsacq.dopfine_params(blocks=2))
        dworst = dop_ref.same(dgot, dop_iq_ref.fine_doppler(iq, 80016, tasks.tolist(), pk, spm, fc, fs, blocks=2, **kw), "fs 2.8 MHz")
        print("fs 2.8 MHz, %d tasks: offset_chips within %.3g, tx_frac within %.3g s, df_hz within %.3g Hz" % (len(combos), worst[0], worst[1], dworst[1]))
        assert (got["flags"] == 0).all() and (got["segments"] == 2 * 40000 // spm).all() and (dgot["flags"] == 0).all()


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------
def test_edges(eng, capture):
    import gpsacq
    import torch
    stride = 80000
    # the window of a task of block 3 ends with the capture: in the middle of a 16-byte group (n_samples % 8 = 5) and of a segment
    n_samples = 3 * 40000 + 7 * SPM + 2733
    assert n_samples % 8 == 5 and (n_samples - 3 * 40000) % SPM != 0
    dmax = eng.dmax
    rows = [(1, 0, 40.0, 3, 100),       # 0: the whole window of 21 segments
            (3, 0, 40.0, -dmax, 0),     # 1: SHORT, 7 segments and a tail that ends inside a group
            (2, 31, 40.0, dmax, 5455),  # 2: SHORT, 14 segments and a tail
            (3, 31, 40.0, 0, 2727),     # 3: SHORT
            (5, 0, 40.0, 0, 7),         # 4: the block starts beyond the capture
            (0, 0, 24.5, 0, 7),         # 5: below snr_min
            (0, 0, 40.0, 0, -1),        # 6
            (0, 0, 40.0, 0, SPM),       # 7
            (0, 32, 40.0, 0, 7),        # 8: a task list with prn = 32
            (-1, 0, 40.0, 0, 7),        # 9
            (0, 5, 40.0, 1, 1),         # 10: a PRN that is not in the capture: still a record
            (0, 0, 40.0, 20000, 7),     # 11: |f| >= fs / 2
            (0, 0, 40.0, -20030, 7),    # 12: |f| >= fs / 2 on the other side
            (4, 0, 40.0, 0, 7)]         # 13: the block starts 925 samples before the end: a hit with no segment, SHORT | NO_POWER | FEW
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    pk = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    for t, r in enumerate(rows):
        pk[t] = (r[2], r[3], r[4], 1.0)
    n = len(rows)
    prm, dprm = gpsacq.refine_params(blocks=3, min_segments=3), gpsacq.dopfine_params(blocks=3, min_segments=3)
    inp, kw = inp_of(eng, True, True, REAL), ref_kw(True, True, REAL)
    ref = refine_iq_ref.refine(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=3, min_segments=3, n_samples=n_samples, **kw)
    dref = dop_iq_ref.fine_doppler(capture, stride, tasks.tolist(), pk, SPM, FC, FS, blocks=3, min_segments=3, n_samples=n_samples, **kw)
    fit = 3 * 40000 // SPM
    assert [r["flags"] for r in ref] == [0, 2, 2, 2, 1, 1, 1, 1, 1, 1, 0, 1, 1, 14] and [r["segments"] for r in ref][:4] == [fit, 7, 14, 7]
    assert [r["flags"] for r in dref] == [r["flags"] for r in ref]
    cut = np.ascontiguousarray(capture[:2 * n_samples])
    host = eng.refine_iq8(cut, inp, pk, tasks=tasks, stride=stride, params=prm)
    dhost = eng.fine_doppler_iq8(cut, inp, pk, tasks=tasks, stride=stride, params=dprm)
    worst, dworst = refine_ref.same(host, ref, "host form"), dop_ref.same(dhost, dref, "host form")
    for t in (4, 5, 6, 7, 8, 9, 11, 12):
        assert host[t].tobytes() == np.int32(1).tobytes() + bytes(52) and dhost[t].tobytes() == np.int32(1).tobytes() + bytes(68), t
    # the device form with sentinel bytes of either kind behind the capture gives the host form's bytes
    d_tasks, d_pk = dev(tasks), dev(pk)
    for sentinel in (0x00, 0xFF):
        buf = np.full(2 * n_samples + 150, sentinel, np.uint8)
        buf[:2 * n_samples] = cut.view(np.uint8)
        d_iq = dev(buf)
        assert d_iq.data_ptr() % 16 == 0
        d_fine, d_dop = fill(n * 56), fill(n * 72)
        torch.cuda.synchronize()
        eng.refine_iq8_device(inp, d_iq.data_ptr(), n_samples, d_pk.data_ptr(), n, d_fine.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                              params=prm, sync=True)
        ms = eng.snapshot_iq8_last_ms()
        assert ms[0] == 0 and ms[1] > 0 and ms[2] == 0
        eng.fine_doppler_iq8_device(inp, d_iq.data_ptr(), n_samples, d_pk.data_ptr(), n, d_dop.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                                    params=dprm, sync=True)
        ms2 = eng.snapshot_iq8_last_ms()
        assert ms2[0] == 0 and ms2[1] == 0 and ms2[2] > 0
        assert d_fine.cpu().numpy().tobytes() == host.tobytes() and d_dop.cpu().numpy().tobytes() == dhost.tobytes(), sentinel
    print("edges: offset_chips within %.3g, tx_frac within %.3g s, df_hz within %.3g Hz; k_refine_iq %.4f ms, k_fine_dop_iq %.4f ms for %d tasks" %
          (worst[0], worst[1], dworst[1], ms[1], ms2[2], n))
    # the reference schedule: tasks == NULL is (block t, PRN t % 32)
    sched = eng.refine_iq8(cut, inp, pk[:4], stride=stride, params=prm)
    refine_ref.same(sched, refine_iq_ref.refine(capture, stride, None, pk[:4], SPM, FC, FS, blocks=3, min_segments=3, n_samples=n_samples, **kw), "schedule")
    # min_segments above what fits: FEW
    few = eng.refine_iq8(cut, inp, pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=3, min_segments=8))
    assert few["flags"].tolist() == [0, 2 | 8, 2, 2 | 8, 1, 1, 1, 1, 1, 1, 0, 1, 1, 14] and (few["segments"] == host["segments"]).all()
    dfew = eng.fine_doppler_iq8(cut, inp, pk, tasks=tasks, stride=stride, params=gpsacq.dopfine_params(blocks=3, min_segments=8))
    assert dfew["flags"].tolist() == few["flags"].tolist()
    # argument errors return 1, launch nothing and write nothing
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out, dout = np.zeros(n, gpsacq.FINE_DTYPE), np.zeros(n, gpsacq.DOPFINE_DTYPE)
    ip = ctypes.byref(inp)
    assert lib.gpsacq_refine_iq8(h, ip, p(cut), n_samples, stride, p(tasks), p(pk), n, p(prm), p(out)) == 0 and out.tobytes() == host.tobytes()
    out[:] = 0

    def bad_params(**kv):
        r = gpsacq.refine_params()
        for k, v in kv.items():
            r[k] = v
        return r

    def bad_dop(**kv):
        r = gpsacq.dopfine_params()
        for k, v in kv.items():
            r[k] = v
        return r
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(half_spacing_chips=0.01), dict(half_spacing_chips=0.51),
               dict(half_spacing_chips=np.nan), dict(snr_min=np.inf), dict(snr_min=np.nan)):
        assert lib.gpsacq_refine_iq8(h, ip, p(cut), n_samples, stride, p(tasks), p(pk), n, p(bad_params(**kv)), p(out)) == 1, kv
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=1), dict(snr_min=np.nan), dict(coherence_min=-1.0), dict(coherence_min=np.nan)):
        assert lib.gpsacq_fine_doppler_iq8(h, ip, p(cut), n_samples, stride, p(tasks), p(pk), n, p(bad_dop(**kv)), p(dout)) == 1, kv
    for fn, par, o in ((lib.gpsacq_refine_iq8, prm, out), (lib.gpsacq_fine_doppler_iq8, dprm, dout)):
        for bad_stride in (79984, 80008, 2 ** 31 + 16):
            assert fn(h, ip, p(cut), n_samples, bad_stride, p(tasks), p(pk), n, p(par), p(o)) == 1 and b"stride" in lib.gpsacq_last_error()
        assert fn(h, None, p(cut), n_samples, stride, p(tasks), p(pk), n, p(par), p(o)) == 1
        assert fn(h, ip, None, n_samples, stride, p(tasks), p(pk), n, p(par), p(o)) == 1
        assert fn(h, ip, p(cut), n_samples, stride, p(tasks), None, n, p(par), p(o)) == 1
        assert fn(h, ip, p(cut), 0, stride, p(tasks), p(pk), n, p(par), p(o)) == 1
        assert fn(h, ip, p(cut), n_samples, stride, p(tasks), p(pk), 0, p(par), p(o)) == 1
        assert fn(h, ip, p(cut), n_samples, stride, p(tasks), p(pk), n, p(par), None) == 1
        for bad in (eng.iq8_input(signed=True, multibit=3), eng.iq8_input(signed=True, multibit=-1),
                    eng.iq8_input(signed=True, remove_dc=True, mean=(200.0, 0.0), multibit=REAL)):
            assert fn(h, ctypes.byref(bad), p(cut), n_samples, stride, p(tasks), p(pk), n, p(par), p(o)) == 1
        fmt = eng.iq8_input(signed=True, multibit=REAL)
        fmt.format = 2
        assert fn(h, ctypes.byref(fmt), p(cut), n_samples, stride, p(tasks), p(pk), n, p(par), p(o)) == 1
    assert not out.view(np.uint8).any() and not dout.view(np.uint8).any()
    # ... and the device forms, a misaligned pointer among them
    d_iq, d_fine, d_dop = dev(np.concatenate([cut.view(np.uint8), np.zeros(32, np.uint8)])), fill(n * 56), fill(n * 72)
    torch.cuda.synchronize()
    for call, d_out, par in ((eng.refine_iq8_device, d_fine, prm), (eng.fine_doppler_iq8_device, d_dop, dprm)):
        for kv in (dict(d_iq_ptr=d_iq.data_ptr() + 8), dict(d_iq_ptr=d_iq.data_ptr() + 2), dict(d_iq_ptr=None), dict(stride=80008), dict(n_samples=0),
                   dict(n_tasks=0), dict(d_peaks_ptr=None), dict(d_out=None)):
            a = dict(dict(inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=n_samples, d_peaks_ptr=d_pk.data_ptr(), n_tasks=n, d_out=d_out.data_ptr(),
                          stride=stride), **kv)
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                call(a["inp"], a["d_iq_ptr"], a["n_samples"], a["d_peaks_ptr"], a["n_tasks"], a["d_out"], stride=a["stride"],
                     d_tasks_ptr=d_tasks.data_ptr(), params=par, sync=True)
            assert ei.value.code == 1, kv
    torch.cuda.synchronize()
    assert (d_fine.cpu().numpy() == 0xA5).all() and (d_dop.cpu().numpy() == 0xA5).all()


def test_the_rails(eng):
    """scale 100, no noise, one satellite of amplitude 1: the largest sums the format can carry, k = 8 in the fine Doppler; U8"""
    import gpsacq
    lo_shift, prn, cp = 7, 9, 1234.0
    dop = lo_shift * FS / 40000 + 21.0
    iq = eng.generate_iq8(2 * 40960 + 64, [(prn, 1.0, dop, cp, 0.3)], if_hz=IF_HZ, scale=100.0, signed=False, noise_sigma=0.0, seed=1)
    assert int(iq.max()) >= 228 and int(iq.min()) <= 28
    ca_rate = refine_iq_ref.nco_words(lo_shift, FC, FS, FC - IF_HZ, REAL)[2]
    pos = (cp * 1.023e6 * (1.0 + dop / 1575.42e6) / FS) % 1023.0
    pk = np.zeros(3, gpsacq.PEAK_DTYPE)
    for t, off in enumerate((-1, 0, 1)):
        pk[t] = (99.0, lo_shift, (int(round(pos / (ca_rate / 2 ** 32))) + off) % SPM, 1.0)
    tasks = np.array([(0, prn - 1)] * 3, np.int32)
    inp, kw = inp_of(eng, False, False, REAL), ref_kw(False, False, REAL)
    got = eng.refine_iq8(iq, inp, pk, tasks=tasks, params=gpsacq.refine_params(blocks=2))
    dgot = eng.fine_doppler_iq8(iq, inp, pk, tasks=tasks, params=gpsacq.dopfine_params(blocks=2))
    ref = refine_iq_ref.refine(iq, 81920, tasks.tolist(), pk, SPM, FC, FS, blocks=2, **kw)
    dref = dop_iq_ref.fine_doppler(iq, 81920, tasks.tolist(), pk, SPM, FC, FS, blocks=2, **kw)
    refine_ref.same(got, ref, "rails")
    dworst = dop_ref.same(dgot, dref, "rails")
    print("rails: k %s, prompt %s, doppler_hz %s (given %.3f), df_hz within %.3g Hz" %
          ([r["k"] for r in dref], got["prompt"].tolist(), np.round(dgot["doppler_hz"], 3).tolist(), dop, dworst[1]))
    assert max(r["k"] for r in dref) >= 8 and (dgot["flags"] == 0).all() and (np.abs(dgot["doppler_hz"] - dop) < 3.0).all()


# ---- 3. sign mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc", [(True, False), (False, True)])
def test_sign_mode_is_the_one_bit_path(eng, capture, signed, dc):
    """GPSACQ_SAMPLES_SIGN = gpsacq_iq8_to_bits_device, then gpsacq_refine_device / gpsacq_fine_doppler_device with stride / 16, byte
    for byte; remove_dc with the mean gpsacq_iq8_to_bits_device itself finds"""
    import gpsacq
    import torch
    iq = np.ascontiguousarray(capture if signed else as_u8(capture))
    n_samples = iq.size // 2 - 3  # the last byte of the 1-bit stream is not full
    n_bytes = (n_samples + 7) // 8
    tasks, pk = hand_peaks(eng.dmax, SPM, 24, seed=7, max_block=1)
    stride = 80016
    raw = iq.view(np.uint8).astype(np.int64)[:2 * n_samples].reshape(-1, 2) - (0 if signed else 128)
    if signed:
        raw = np.where(raw >= 128, raw - 256, raw)
    mean = (raw[:, 0].sum() / n_samples, raw[:, 1].sum() / n_samples) if dc else (0.0, 0.0)
    inp = eng.iq8_input(signed=signed, remove_dc=dc, mean=mean, mix_hz=FC - IF_HZ, multibit=0)
    d_iq, d_tasks, d_pk = dev(iq), dev(tasks), dev(pk)
    d_bits, d_f1, d_d1, d_f2, d_d2 = fill(n_bytes + 16), fill(24 * 56), fill(24 * 72), fill(24 * 56), fill(24 * 72)
    torch.cuda.synchronize()
    rc = eng._lib.gpsacq_iq8_to_bits_device(eng._h, d_iq.data_ptr(), n_samples, 1 if signed else 0, 1 if dc else 0, FC - IF_HZ, 0.0, d_bits.data_ptr(), 1)
    assert rc == 0
    prm, dprm = gpsacq.refine_params(blocks=3), gpsacq.dopfine_params(blocks=3)
    eng.refine_device(d_bits.data_ptr(), n_bytes, d_pk.data_ptr(), 24, d_f1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(), params=prm)
    eng.fine_doppler_device(d_bits.data_ptr(), n_bytes, d_pk.data_ptr(), 24, d_d1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(),
                            params=dprm)
    eng.refine_iq8_device(inp, d_iq.data_ptr(), n_samples, d_pk.data_ptr(), 24, d_f2.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(), params=prm)
    ms = eng.snapshot_iq8_last_ms()
    eng.fine_doppler_iq8_device(inp, d_iq.data_ptr(), n_samples, d_pk.data_ptr(), 24, d_d2.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(),
                                params=dprm)
    ms2 = eng.snapshot_iq8_last_ms()
    f1 = np.frombuffer(d_f1.cpu().numpy().tobytes(), gpsacq.FINE_DTYPE)
    print("sign mode %s dc %d: conversion %.4f ms, k_refine %.4f ms, k_fine_dop %.4f ms; %d records, prompt %d .. %d" %
          ("S8" if signed else "U8", dc, ms[0], ms[1], ms2[2], f1.size, f1["prompt"].min(), f1["prompt"].max()))
    assert (f1["flags"] == 0).all() and f1["prompt"].min() > 0
    assert d_f2.cpu().numpy().tobytes() == d_f1.cpu().numpy().tobytes()
    assert d_d2.cpu().numpy().tobytes() == d_d1.cpu().numpy().tobytes()
    assert ms[0] > 0 and ms[1] > 0 and ms[2] == 0 and ms2[0] > 0 and ms2[1] == 0 and ms2[2] > 0
    # the host forms agree with the device forms
    host = eng.refine_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=prm, n_samples=n_samples)
    dhost = eng.fine_doppler_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=dprm, n_samples=n_samples)
    assert host.tobytes() == f1.tobytes() and dhost.tobytes() == d_d1.cpu().numpy().tobytes()


# ---- 4. and 5.: the northern receiver's eight satellites in an IQ capture, searched, refined, fixed --------------------------------
@pytest.fixture(scope="module")
def scene(eng):
    """tests/test_gpu_refine.py's scene as a 19-block IQ capture: eight satellites at amplitude 0.1, sigma 1, scale 16; blocks 0..3
    searched with search_iq8 in multi-bit mode; the time prior of every block is 20 s off, early and late in turn"""
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, n_search, spb = 19, 4, 40960
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3  # the receive time of the first sample of block 0
    sats, dops = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.1)
    iq = eng.generate_iq8(n_blocks * spb, sats, if_hz=IF_HZ, scale=16.0, signed=True, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = np.array([(b, s[0] - 1) for b in range(n_search) for s in sats], np.int32)
    inp = inp_of(eng, True, False, REAL)
    _, peaks = eng.search_iq8(iq[:2 * n_search * spb], inp, tasks=tasks, want_cells=False)
    blk_ms, blk_frac = block_times(ref_ms, ref_frac, n_search, spb, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    iq.setflags(write=False)
    return dict(geo=geo, sel=sel, ephs=ephs, iq=iq, inp=inp, tasks=tasks, peaks=peaks.reshape(n_search, len(sel)), blk_ms=blk_ms, blk_frac=blk_frac,
                prior=prior, rx_ms=np.ascontiguousarray(prior["rx_ms"].astype(np.int32)), rec=to_records(ephs), dops=dops)


SIZES = lambda n, m: dict(dopfine=n * m * 72, rate=n * m * 32, dfix=n * 88, prior=n * 32, fine=n * m * 56, obs=n * m * 32, fix=n * 80, info=n * 40,
                          out=n * m * 32)


@pytest.mark.parametrize("multibit", [REAL, 0])
def test_chains(eng, scene, multibit):
    """gpsacq_coarse_fix_fine_iq8_device and gpsacq_cold_fix_iq8_device = their kernels run one by one through the single entry
    points, byte for byte, with and without the optional buffers; multi-bit and sign mode"""
    import gpsacq
    import torch
    n, m = scene["peaks"].shape
    inp = inp_of(eng, True, False, multibit)
    ns = scene["iq"].size // 2
    d_iq, d_tasks, d_pk, d_rx, d_prior = dev(scene["iq"]), dev(scene["tasks"]), dev(scene["peaks"]), dev(scene["rx_ms"]), dev(scene["prior"])
    ptr = lambda t: t.data_ptr()
    sizes = SIZES(n, m)
    # the warm chain, step by step
    a = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.refine_iq8_device(inp, ptr(d_iq), ns, ptr(d_pk), n * m, ptr(a["fine"]), d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_obs_fine_device(ptr(d_pk), ptr(a["fine"]), n, m, ptr(a["obs"]), sync=False)
    eng.coarse_fix_device(scene["rec"], ptr(a["obs"]), ptr(d_prior), n, m, ptr(a["fix"]), ptr(a["info"]), ptr(a["out"]), sync=True)
    warm = {k: a[k].cpu().numpy().tobytes() for k in ("fine", "obs", "fix", "info", "out")}
    fix = np.frombuffer(warm["fix"], gpsacq.FIX_DTYPE)
    assert multibit == 0 or ((fix["status"] == 0).all() and (fix["n_used"] == m).all())  # (the sign path promises nothing at this amplitude)
    b = {k: fill(sizes[k]) for k in warm}
    torch.cuda.synchronize()
    eng.coarse_fix_fine_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_prior), ptr(b["fix"]), ptr(b["info"]),
                                   d_fine_ptr=ptr(b["fine"]), d_obs_ptr=ptr(b["obs"]), d_obs_out_ptr=ptr(b["out"]), sync=True)
    ms_w = eng.snapshot_iq8_last_ms()
    for k, t in b.items():
        assert t.cpu().numpy().tobytes() == warm[k], k
    c = {k: fill(sizes[k]) for k in ("fix", "info")}
    torch.cuda.synchronize()
    eng.coarse_fix_fine_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_prior), ptr(c["fix"]), ptr(c["info"]), sync=True)
    assert all(t.cpu().numpy().tobytes() == warm[k] for k, t in c.items())
    # the cold chain, step by step
    a = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.fine_doppler_iq8_device(inp, ptr(d_iq), ns, ptr(d_pk), n * m, ptr(a["dopfine"]), d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_obs_device(ptr(d_pk), n, m, ptr(a["obs"]), sync=False)
    eng.rate_obs_fine_device(ptr(d_pk), ptr(a["dopfine"]), n, m, ptr(a["rate"]), sync=False)
    eng.doppler_fix_device(scene["rec"], ptr(a["obs"]), ptr(a["rate"]), ptr(d_rx), n, m, ptr(a["dfix"]), ptr(a["prior"]), sync=False)
    eng.refine_iq8_device(inp, ptr(d_iq), ns, ptr(d_pk), n * m, ptr(a["fine"]), d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_obs_fine_device(ptr(d_pk), ptr(a["fine"]), n, m, ptr(a["obs"]), sync=False)
    eng.coarse_fix_device(scene["rec"], ptr(a["obs"]), ptr(a["prior"]), n, m, ptr(a["fix"]), ptr(a["info"]), ptr(a["out"]), sync=True)
    steps = {k: t.cpu().numpy().tobytes() for k, t in a.items()}
    fix = np.frombuffer(steps["fix"], gpsacq.FIX_DTYPE)
    assert multibit == 0 or ((fix["status"] == 0).all() and (fix["n_used"] == m).all())
    b = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.cold_fix_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), ptr(d_rx), n, m, ptr(b["fix"]), ptr(b["info"]), ptr(b["dfix"]),
                            d_dopfine_ptr=ptr(b["dopfine"]), d_rate_obs_ptr=ptr(b["rate"]), d_prior_ptr=ptr(b["prior"]), d_fine_ptr=ptr(b["fine"]),
                            d_obs_ptr=ptr(b["obs"]), d_obs_out_ptr=ptr(b["out"]), sync=True)
    ms_c = eng.snapshot_iq8_last_ms()
    for k, t in b.items():
        assert t.cpu().numpy().tobytes() == steps[k], k
    c = {k: fill(sizes[k]) for k in ("fix", "info", "dfix")}
    torch.cuda.synchronize()
    eng.cold_fix_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), ptr(d_rx), n, m, ptr(c["fix"]), ptr(c["info"]), ptr(c["dfix"]),
                            sync=True)
    for k, t in c.items():
        assert t.cpu().numpy().tobytes() == steps[k], k
    print("chains, multibit %d: warm: conversion %.4f ms, fine records %.4f ms; cold: conversion %.4f ms, fine records %.4f ms, fine Dopplers %.4f ms "
          "for %d tasks of 16 blocks" % (multibit, ms_w[0], ms_w[1], ms_c[0], ms_c[1], ms_c[2], n * m))
    assert ms_w[1] > 0 and ms_w[2] == 0 and ms_c[1] > 0 and ms_c[2] > 0
    assert (ms_w[0] > 0 and ms_c[0] > 0) if multibit == 0 else (ms_w[0] == 0 and ms_c[0] == 0)
    # argument errors: nothing launched, nothing written
    d = {k: fill(sizes[k]) for k in ("fix", "info", "dfix")}
    torch.cuda.synchronize()
    cold = lambda **kw: dict(dict(eph=scene["rec"], inp=inp, d_iq_ptr=ptr(d_iq), n_samples=ns, d_tasks_ptr=ptr(d_tasks), d_peaks_ptr=ptr(d_pk),
                                  d_rx_ms_ptr=ptr(d_rx), n_fix=n, n_chans=m, d_fix_ptr=ptr(d["fix"]), d_info_ptr=ptr(d["info"]),
                                  d_doppler_fix_ptr=ptr(d["dfix"])), **kw)
    bad_inp = eng.iq8_input(signed=True, multibit=7)
    for kw in (dict(d_iq_ptr=None), dict(d_iq_ptr=ptr(d_iq) + 4), dict(inp=bad_inp), dict(d_peaks_ptr=None), dict(d_rx_ms_ptr=None), dict(d_fix_ptr=None),
               dict(d_info_ptr=None), dict(d_doppler_fix_ptr=None), dict(n_fix=0), dict(n_chans=0), dict(n_chans=13), dict(n_samples=0),
               dict(stride=79984), dict(stride=80008), dict(dopfine_params=np.array([(0, 2, 25.0, 0.0)], gpsacq.DOPFINE_PARAMS_DTYPE)),
               dict(doppler_params=gpsacq.doppler_fix_params(-1.0)), dict(refine_params=np.array([(16, 0, 0.25, 25.0)], gpsacq.REFINE_PARAMS_DTYPE)),
               dict(params=gpsacq.coarse_params(0.0)), dict(d_obs_ptr=ptr(a["obs"]), d_obs_out_ptr=ptr(a["obs"]))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.cold_fix_iq8_device(**cold(**kw))
        assert ei.value.code == 1, kw
    warm_args = lambda **kw: dict(dict(eph=scene["rec"], inp=inp, d_iq_ptr=ptr(d_iq), n_samples=ns, d_tasks_ptr=ptr(d_tasks), d_peaks_ptr=ptr(d_pk),
                                       n_fix=n, n_chans=m, d_prior_ptr=ptr(d_prior), d_fix_ptr=ptr(d["fix"]), d_info_ptr=ptr(d["info"])), **kw)
    for kw in (dict(d_iq_ptr=None), dict(d_iq_ptr=ptr(d_iq) + 4), dict(inp=bad_inp), dict(d_peaks_ptr=None), dict(d_prior_ptr=None), dict(d_fix_ptr=None),
               dict(d_info_ptr=None), dict(n_fix=0), dict(n_chans=13), dict(n_samples=0), dict(stride=80008),
               dict(refine_params=np.array([(16, 0, 0.25, 25.0)], gpsacq.REFINE_PARAMS_DTYPE)), dict(params=gpsacq.coarse_params(0.0))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.coarse_fix_fine_iq8_device(**warm_args(**kw))
        assert ei.value.code == 1, kw
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in d.values())


def test_end_to_end_fine_fixes(eng, scene):
    """Search peaks of an IQ capture at amplitude 0.1 refined with the defaults (16 blocks, d = 0.25) both ways, then fixes from the
    multi-bit fine phases.

    Measured on an MI355X (printed by this test): code phase against the truth over the 32 hits, whole-sample 20.91 m rms, sign path
    5.93 m rms (worst 15.61), multi-bit 3.80 m rms (worst 8.69); position error of the four rows, sign-path fixes 3.2 / 9.0 / 7.0 /
    11.5 m, multi-bit fixes 3.7 / 5.2 / 7.7 / 7.8 m, inside the linear bounds 15.6 / 14.7 / 14.4 / 16.3 m of their own range errors."""
    import gpsacq
    geo, ephs, peaks, iq = scene["geo"], scene["ephs"], scene["peaks"], scene["iq"]
    n, m = peaks.shape
    assert (peaks["snr"] >= gpsacq.THRESHOLD).all()
    fine = eng.refine_iq8(iq, scene["inp"], peaks, tasks=scene["tasks"])
    ref = refine_iq_ref.refine(iq, 81920, scene["tasks"].tolist(), peaks, SPM, FC, FS, **ref_kw(True, False, REAL))
    worst = refine_ref.same(fine, ref, "end to end")
    assert (fine["flags"] == 0).all() and (fine["segments"] == 16 * 40000 // SPM).all()
    sign = eng.refine_iq8(iq, inp_of(eng, True, False, 0), peaks, tasks=scene["tasks"])
    assert (sign["flags"] == 0).all()
    # code phases against the truth, as ranges
    truth = np.stack([nav_ref.truth_tx(e, geo["rx"], scene["blk_ms"], scene["blk_frac"]) for e in ephs], 1)
    want = truth % 1e-3
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    e_whole = nav_ref.C * wrap(peaks["ca_shift"] / FS - want)
    e_fine = nav_ref.C * wrap(fine["tx_frac"] - want)
    e_sign = nav_ref.C * wrap(sign["tx_frac"] - want)
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    print("records equal the reference: offset_chips within %.3g, tx_frac within %.3g s" % (worst[0], worst[1]))
    print("code phase against the truth over %d hits: whole-sample rms %.2f m, sign path rms %.2f m (worst %.2f), multi-bit rms %.2f m (worst %.2f)" %
          (n * m, rms(e_whole), rms(e_sign), np.abs(e_sign).max(), rms(e_fine), np.abs(e_fine).max()))
    rec = scene["rec"]
    obs_f = eng.coarse_obs(peaks, fine=fine)
    assert (obs_f["valid"] == 1).all() and (obs_f["tx_frac"] == fine["tx_frac"]).all()
    fix_f, info_f, _ = eng.coarse_fix(rec, obs_f, scene["prior"])
    fix_s, _, _ = eng.coarse_fix(rec, eng.coarse_obs(peaks, fine=sign), scene["prior"])
    err_f = np.linalg.norm(np.stack([fix_f["x"], fix_f["y"], fix_f["z"]], 1) - geo["rx"], axis=1)
    err_s = np.linalg.norm(np.stack([fix_s["x"], fix_s["y"], fix_s["z"]], 1) - geo["rx"], axis=1)
    exact, _ = phases(geo, scene["sel"], scene["blk_ms"], scene["blk_frac"])
    rows = coarse_ref.coarse_fix(geo["ephs"], exact, scene["prior"])
    bound = np.zeros(n)
    for i in range(n):
        H = rows[i]["H"]
        G = np.linalg.solve(H.T @ H, H.T)[:3]
        bound[i] = np.linalg.norm(G, 2) * np.linalg.norm(e_fine[i]) * 1.01 + 0.01
    print("position error, sign-path fixes %s m, multi-bit fixes %s m (linear bound of each row's range errors %s m)" %
          (np.round(err_s, 1), np.round(err_f, 1), np.round(bound, 1)))
    assert (fix_f["status"] == 0).all() and (fix_f["n_used"] == m).all() and (info_f["flags"] == 0).all()
    assert rms(e_fine) < rms(e_sign)
    assert (err_f <= bound).all()
