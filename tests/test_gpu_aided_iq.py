"""Aided acquisition on an 8-bit IQ capture on the GPU (gpsacq_aided_search_iq8*, gpsacq_aided_peaks_iq8_device) against
tests/aided_iq_ref.py, the numpy restatement of "Aided acquisition on an 8-bit IQ capture" of include/gpsacq.h.

Every integer field of a record and every entry of powers_out must equal the reference, peaks byte for byte; ratio may differ by
1e-12 relative (one fp64 division of two integers).  fs = 5.456 MHz, fc = 4.092 MHz; the bytes come from Engine.generate_iq8 at a
residual IF of 2 kHz, so that the hypotheses at -kmax sit at a NEGATIVE carrier.  The reference's sums are its quick spelling
(Law.powers_stream), which tests/test_aided_iq.py holds against the sample-by-sample one on the CPU.  Sign mode is held against
gpsacq_iq8_to_bits_device followed by gpsacq_aided_search_device, byte for byte.
Each test prints what it measured before it asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import aided_cases
import aided_iq_cases as ic
import aided_iq_ref
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
    """four blocks of three satellites at amplitude 0.3 (PRN 1 and 32 among them), int8, about 330 KB, made once"""
    sats = [(1, 0.3, 1234.0, 100.25, 0.1), (32, 0.3, -2900.0, 4000.7, 0.4), (17, 0.3, 310.0, 2727.4, 0.7)]
    iq = eng.generate_iq8(4 * 40960 + 1000, sats, if_hz=IF_HZ, scale=16.0, signed=True, noise_sigma=1.0, seed=5)
    iq.setflags(write=False)
    return iq


def inp_of(eng, signed, dc, multibit, if_hz=IF_HZ, fc=FC):
    return eng.iq8_input(signed=signed, remove_dc=dc, mean=ic.MEAN if dc else (0.0, 0.0), mix_hz=ic.mix_of(multibit, if_hz, fc), multibit=multibit)


def hand_aid(eng, n, seed, max_block=1):
    import gpsacq
    return ic.hand_aid(gpsacq.AID_DTYPE, eng.kmax, SPM, eng.doppler_step_hz, n, seed, max_block)


def reference(eng, iq, stride, tasks, aid, spm=SPM, fc=FC, fs=FS, **kw):
    step = 0.0 if eng.doppler_sub == 1 and eng.doppler_stride == 1 else eng.doppler_step_hz
    return aided_iq_ref.aided_search(iq, stride, None if tasks is None else tasks.tolist(), aid, spm, fc, fs, eng.kmax, step_hz=step, stream=True, **kw)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


# ---- 1. exact against the reference --------------------------------------------------------------------------------------------
# (blocks, W, K) out of {1, 2, 3} x {0, 5, 40, 100, 127} x {0, 1, 2}, the large W with the small windows (the reference's time); the
# three strides and the eight (format, mean, REAL / COMPLEX) modes go round along the list.  ca_center 0, 1 and spm - 1 put base + h
# across spm on both sides (ca_center < W and ca_center > spm - W) wherever W > 1
_BWK = [(1, 0, 0), (1, 127, 0), (1, 100, 1), (2, 40, 2), (3, 5, 2), (2, 5, 0), (3, 40, 0), (2, 100, 0), (1, 40, 1), (3, 0, 1), (1, 127, 1), (3, 5, 1)]
CASES = [bwk + ((80000, 80016, 81920)[i % 3],) + ic.MODES[(3 * i + 1) % 8] for i, bwk in enumerate(_BWK)]


@pytest.mark.parametrize("blocks,W,K,stride,signed,dc,multibit", CASES)
def test_exact_against_the_reference(eng, capture, blocks, W, K, stride, signed, dc, multibit):
    import gpsacq
    tasks, aid = hand_aid(eng, 24, seed=blocks * 1000 + W * 10 + K)
    iq = capture if signed else ic.as_u8(capture)
    inp, kw = inp_of(eng, signed, dc, multibit), ic.ref_kw(signed, dc, multibit, IF_HZ)
    prm = gpsacq.aided_params(blocks=blocks, code_half=W, dop_half=K, ratio_min=1.2)
    got, pk, pw = eng.aided_search_iq8(iq, inp, aid, tasks=tasks, stride=stride, params=prm, powers=True)
    ref = reference(eng, iq, stride, tasks, aid, blocks=blocks, code_half=W, dop_half=K, ratio_min=1.2, **kw)
    label = "blocks %d W %d K %d stride %d %s dc %d multibit %d" % (blocks, W, K, stride, "S8" if signed else "U8", dc, multibit)
    worst = aided_iq_ref.same(got, ref, pk, pw, label)
    rows = sum(int(not r["powers"][d].any()) for r in ref for d in range(2 * K + 1))
    wraps = sum(int((int(a["ca_center"]) - W) % SPM + 2 * W >= SPM) for a in aid)
    print("%s: 24 records, %d powers and the peaks equal the reference (%d rows of invalid d, %d tasks across the wrap); ratio within %.3g; flags %s" %
          (label, pw.size, rows, wraps, worst, sorted(set(got["flags"].tolist()))))
    assert (got["segments"] == blocks * 40000 // SPM).all() and (got["n_code"] == 2 * W + 1).all() and (got["n_dop"] == 2 * K + 1).all()
    assert not (got["flags"] & ~gpsacq.AIDED_BELOW).any() and (got["best"] > 0).all() and (got["floor"] > 0).all()
    assert (rows > 0) == (K > 0) and (wraps > 0) == (W > 0)
    assert set(aid["lo_center"].tolist()) == {-eng.kmax, 0, eng.kmax}  # -kmax: f = lo_dop + 2 kHz < 0, a word above 2^31


def test_a_second_rate_whose_segment_is_no_multiple_of_the_chunk():
    """fs = 8.184 MHz, fc = 2.046 MHz: spm 8184 = 7 * 1024 + 1016, the kernel's last chunk of a segment is a short one and no
    segment starts where a chunk does; an engine and a capture of its own"""
    import gpsacq
    fs, fc, spm, if_hz = 8.184e6, 2.046e6, 8184, -1500.0
    with gpsacq.Engine(fc, fs, 5000.0) as e:
        iq = e.generate_iq8(3 * 40960, [(1, 0.3, 800.0, 100.25, 0.1), (32, 0.3, -2100.0, 1500.7, 0.4)], if_hz=if_hz, scale=16.0, signed=False,
                            noise_sigma=1.0, seed=6)
        tasks, aid = ic.hand_aid(gpsacq.AID_DTYPE, e.kmax, spm, e.doppler_step_hz, 12, seed=4)
        inp = e.iq8_input(signed=False, remove_dc=True, mean=ic.MEAN, mix_hz=fc - if_hz, multibit=REAL)
        prm = gpsacq.aided_params(blocks=2, code_half=40, dop_half=1, ratio_min=1.2)
        got, pk, pw = e.aided_search_iq8(iq, inp, aid, tasks=tasks, stride=80016, params=prm, powers=True)
        ref = reference(e, iq, 80016, tasks, aid, spm, fc, fs, blocks=2, code_half=40, dop_half=1, ratio_min=1.2, signed=False, mean=ic.MEAN,
                        mix_hz=fc - if_hz, multibit=REAL)
        worst = aided_iq_ref.same(got, ref, pk, pw, "fs 8.184 MHz")
        print("fs 8.184 MHz, spm %d, kmax %d: 12 records and %d powers equal the reference; ratio within %.3g" % (spm, e.kmax, pw.size, worst))
        assert (got["segments"] == 2 * 40000 // spm).all() and spm % 1024 != 0 and (got["best"] > 0).all()


def test_powers_are_refine_iq8s_prompt_sums(eng, capture):
    """against a kernel already merged, whatever the new reference says: for base + h < spm, power(h, d) is the `prompt` k_refine_iq
    returns for the peak (ca_shift_h, lo_shift_d) with the same input"""
    import gpsacq
    W, K, blocks = 5, 1, 2
    tasks, aid = ic.hand_aid(gpsacq.AID_DTYPE, eng.kmax - 1, SPM, eng.doppler_step_hz, 8, seed=77)  # every d on the grid
    total = 0
    for signed, dc, multibit in ((False, True, REAL), (True, False, COMPLEX)):
        iq = capture if signed else ic.as_u8(capture)
        inp = inp_of(eng, signed, dc, multibit)
        _, _, pw = eng.aided_search_iq8(iq, inp, aid, tasks=tasks, stride=80016, params=gpsacq.aided_params(blocks=blocks, code_half=W, dop_half=K), powers=True)
        peaks, ptasks, where = [], [], []
        for t in range(len(aid)):
            base = (int(aid["ca_center"][t]) - W) % SPM
            for d in range(2 * K + 1):
                for h in range(2 * W + 1):
                    if base + h < SPM:
                        peaks.append((30.0, int(aid["lo_center"][t]) - K + d, base + h, 0.0))
                        ptasks.append(tuple(tasks[t]))
                        where.append((t, d, h))
        fine = eng.refine_iq8(iq, inp, np.array(peaks, gpsacq.PEAK_DTYPE), tasks=np.array(ptasks, np.int32), stride=80016,
                              params=gpsacq.refine_params(blocks=blocks))
        mine = np.array([pw[w] for w in where], np.uint64)
        print("%s dc %d multibit %d: %d of %d powers have a refine peak; all equal its prompt: %s" %
              ("S8" if signed else "U8", dc, multibit, len(where), pw.size, bool((fine["prompt"] == mine).all())))
        assert (fine["flags"] == 0).all() and (fine["prompt"] == mine).all() and 0 < len(where) < pw.size
        total += len(where)
    assert total >= 300


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------
def edge_rows(kmax):
    rows = [(1, 0, 0, 100, 3),          # 0: the whole window of 21 segments
            (3, 0, 0, 0, -kmax),        # 1: SHORT, 7 segments and a tail that ends inside a 16-byte group; one invalid d row
            (2, 31, 0, 5455, kmax),     # 2: SHORT, 14 segments and a tail
            (3, 31, 0, 2727, 0),        # 3: SHORT
            (5, 0, 0, 7, 0),            # 4: the block starts beyond the capture
            (0, 0, 4, 7, 0),            # 5: a flagged prediction
            (0, 0, 0, -1, 0),           # 6
            (0, 0, 0, SPM, 0),          # 7
            (0, 32, 0, 7, 0),           # 8: a task list with prn = 32
            (-1, 0, 0, 7, 0),           # 9
            (0, 5, 0, 1, kmax + 2),     # 10: no Doppler hypothesis on the grid
            (0, 5, 0, 1, -kmax - 3),    # 11
            (0, 5, 0, 1, 2 ** 31 - 1),  # 12
            (0, 5, 0, 1, kmax + 1),     # 13: one of three on the grid
            (0, 31, 0, 4000, -21),      # 14: kept
            (4, 0, 0, 7, 0)]            # 15: the block starts 925 samples before the end: searched, no segment
    return rows


def test_edges(eng, capture):
    import gpsacq
    import torch
    stride = 80000
    n_samples = 3 * 40000 + 7 * SPM + 2733  # the window of a task of block 3 ends with the capture, inside a group and a segment
    assert n_samples % 8 == 5 and (n_samples - 3 * 40000) % SPM != 0
    kmax = eng.kmax
    rows = edge_rows(kmax)
    tasks = np.array([(r[0], r[1]) for r in rows], np.int32)
    aid = np.zeros(len(rows), gpsacq.AID_DTYPE)
    for t, r in enumerate(rows):
        aid[t] = (r[2], r[3], r[4], 0, 0.0, 0.0, 45.0)
    pin = np.zeros(len(rows), gpsacq.PEAK_DTYPE)
    pin["snr"], pin["lo_shift"], pin["ca_shift"], pin["max_pwr"] = 24.99, 5, 6, 7.0
    pin[14] = (25.0, -21, 4001, 1234.5)
    n = len(rows)
    kw = dict(blocks=3, min_segments=8, code_half=40, dop_half=1, ratio_min=1.0)
    prm = gpsacq.aided_params(**kw)
    inp, rkw = inp_of(eng, True, True, REAL), ic.ref_kw(True, True, REAL, IF_HZ)
    ref = reference(eng, capture, stride, tasks, aid, peaks_in=pin, n_samples=n_samples, **kw, **rkw)
    fit = 3 * 40000 // SPM
    assert [r["flags"] & 15 for r in ref] == [0, 4 | 8, 4, 4 | 8, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 4 | 8]
    assert [r["segments"] for r in ref][:4] == [fit, 7, 14, 7] and ref[15]["flags"] == 4 | 8 | 16 | 32 and ref[15]["floor"] == 0
    cut = np.ascontiguousarray(capture[:2 * n_samples])
    host, hpk, hpw = eng.aided_search_iq8(cut, inp, aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True)
    worst = aided_iq_ref.same(host, ref, hpk, hpw, "host form")
    for t in range(4, 13):
        assert host[t].tobytes() == np.int32(2).tobytes() + bytes(60) and hpk[t].tobytes() == bytes(16) and not hpw[t].any(), t
    assert host[14].tobytes() == np.int32(1).tobytes() + bytes(60) and hpk[14].tobytes() == pin[14].tobytes() and not hpw[14].any()
    assert not hpw[1][0].any() and hpw[1][1].any() and not hpw[13][1:].any() and hpw[13][0].any()
    assert hpk[1].tobytes() == bytes(16) and hpk[3].tobytes() == bytes(16)  # FEW: measured, and no peak
    assert host["ratio"][15] == 0.0 and host["n_code"][15] == 81 and not hpw[15].any()
    # the device form, sentinel bytes of either kind behind the capture, poisoned outputs
    d_tasks, d_aid, d_pin = dev(tasks), dev(aid), dev(pin)
    for sentinel in (0x00, 0xFF):
        buf = np.full(2 * n_samples + 150, sentinel, np.uint8)
        buf[:2 * n_samples] = cut.view(np.uint8)
        d_iq = dev(buf)
        assert d_iq.data_ptr() % 16 == 0
        d_out, d_pk, d_pw = fill((n + 1) * 64), fill((n + 1) * 16), fill((n + 1) * 3 * 81 * 8)
        torch.cuda.synchronize()
        eng.aided_search_iq8_device(inp, d_iq.data_ptr(), n_samples, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), stride=stride,
                                    d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=d_pw.data_ptr(), params=prm, sync=True)
        o = [x.cpu().numpy().tobytes() for x in (d_out, d_pk, d_pw)]
        assert o[0] == host.tobytes() + b"\xa5" * 64 and o[1] == hpk.tobytes() + b"\xa5" * 16 and o[2] == hpw.tobytes() + b"\xa5" * (3 * 81 * 8), sentinel
    ms = eng.aided_iq8_last_ms()
    print("edges: ratio within %.3g; host and device forms agree byte for byte, nothing written beyond the records; k_aided_iq %.4f ms for %d tasks" %
          (worst, ms[2], n))
    assert ms[0] == 0 and ms[1] == 0 and ms[2] > 0
    # a block AT n_samples is NO_AID, one sample before it a search without a segment
    at = np.ascontiguousarray(capture[:2 * 160008])
    for ns, want in ((160000, 2), (160001, 4 | 8 | 16 | 32)):
        r, _ = eng.aided_search_iq8(at, inp, aid[:1], tasks=np.array([(4, 0)], np.int32), stride=stride, params=prm, n_samples=ns)
        assert r["flags"][0] == want and r["segments"][0] == 0, (ns, r)
    # the reference schedule (tasks == NULL is (block t, PRN t % 32)), and no input peaks: nothing is kept
    sched, spk = eng.aided_search_iq8(cut, inp, aid[:4], stride=stride, params=prm)
    aided_iq_ref.same(sched, reference(eng, capture, stride, None, aid[:4], n_samples=n_samples, **kw, **rkw), spk, None, "schedule")


@pytest.mark.parametrize("signed", [True, False])
def test_the_rails(eng, signed):
    """every byte 0x00 / 0xFF / 0x7F / 0x80, with and without a mean of (128, -128) taken off: |v_i| reaches 256 (the byte -128 less a
    mean of +128; v_q is then 0) and every sample adds alike, the largest sums the format can carry on one arm; all fields against
    the reference's Python integers"""
    import gpsacq
    tasks, aid = hand_aid(eng, 2, seed=1, max_block=0)
    aid["lo_center"] = (0, 3)
    prm = gpsacq.aided_params(blocks=3, code_half=2, dop_half=1, ratio_min=0.5)
    top = 0
    for byte in (0x00, 0xFF, 0x7F, 0x80):
        iq = np.full(2 * (3 * 40000 + 16), byte, np.uint8)
        for dc in (False, True):
            mean = (128.0, -128.0) if dc else (0.0, 0.0)
            inp = eng.iq8_input(signed=signed, remove_dc=dc, mean=mean, mix_hz=FC - IF_HZ, multibit=REAL)
            got, pk, pw = eng.aided_search_iq8(iq, inp, aid, tasks=tasks, stride=80000, params=prm, powers=True)
            ref = reference(eng, iq, 80000, tasks, aid, blocks=3, code_half=2, dop_half=1, ratio_min=0.5, signed=signed, mean=mean if dc else None,
                            mix_hz=FC - IF_HZ, multibit=REAL)
            aided_iq_ref.same(got, ref, pk, pw, "rails %02x %s dc %d" % (byte, "S8" if signed else "U8", dc))
            top = max(top, int(got["floor"].max()))
            assert (got["floor"] > 0).all() == any(r["floor"] > 0 for r in ref)
    print("rails %s: every field equals the reference; the largest floor %d = 2^%.1f" % ("S8" if signed else "U8", top, np.log2(max(top, 1))))
    assert top == 2 * 21 * SPM * 256 * 256  # |v_i| = 256, v_q = 0 on every sample of 21 segments


def test_a_zero_capture(eng):
    import gpsacq
    tasks, aid = hand_aid(eng, 3, seed=2, max_block=0)
    iq = np.zeros(2 * 40960, np.int8)
    got, pk, pw = eng.aided_search_iq8(iq, inp_of(eng, True, False, REAL), aid, tasks=tasks, params=gpsacq.aided_params(blocks=1, code_half=3), powers=True)
    print("all-zero S8 capture: flags %s floor %s ratio %s" % (got["flags"].tolist(), got["floor"].tolist(), got["ratio"].tolist()))
    assert (got["floor"] == 0).all() and (got["ratio"] == 0.0).all() and (got["flags"] == gpsacq.AIDED_NO_POWER | gpsacq.AIDED_BELOW).all()
    assert (got["segments"] == 7).all() and not pw.any() and pk.tobytes() == bytes(48) and (got["best_h"] == 0).all()


def test_argument_errors(eng, capture):
    import gpsacq
    import torch
    stride, n_samples, n = 80000, 3 * 40960, 6
    tasks, aid = hand_aid(eng, n, seed=3)
    pin = np.zeros(n, gpsacq.PEAK_DTYPE)
    prm = gpsacq.aided_params(blocks=1, code_half=5, dop_half=1)
    inp = inp_of(eng, True, True, REAL)
    cut = np.ascontiguousarray(capture[:2 * n_samples])
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    ip = ctypes.byref(inp)
    out, opk, opw = np.zeros(n, gpsacq.AIDED_DTYPE), np.zeros(n, gpsacq.PEAK_DTYPE), np.zeros(n * 33, np.uint64)
    call = lambda **kv: lib.gpsacq_aided_search_iq8(*[dict(dict(h=h, ip=ip, iq=p(cut), ns=n_samples, stride=stride, tasks=p(tasks), aid=p(aid), pin=p(pin), n=n,
                                                                prm=p(prm), out=p(out), opk=p(opk), opw=p(opw)), **kv)[k]
                                                      for k in ("h", "ip", "iq", "ns", "stride", "tasks", "aid", "pin", "n", "prm", "out", "opk", "opw")])
    assert call() == 0 and out["n_code"].tolist() == [11] * n
    out[:], opk[:], opw[:] = 0, 0, 0

    def bad_params(**kv):
        r = gpsacq.aided_params()
        for k, v in kv.items():
            r[k] = v
        return p(r)
    for kv in (dict(blocks=0), dict(blocks=65), dict(min_segments=0), dict(code_half=-1), dict(code_half=128), dict(dop_half=-1), dict(dop_half=9),
               dict(keep_snr=np.nan), dict(ratio_min=np.inf)):
        keep = bad_params(**kv)
        assert call(prm=keep) == 1, kv
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
    assert not out.view(np.uint8).any() and not opk.view(np.uint8).any() and not opw.any()
    # the device forms, a misaligned pointer among them, and the chain
    d_iq, d_tasks, d_aid = dev(np.concatenate([cut.view(np.uint8), np.zeros(32, np.uint8)])), dev(tasks), dev(aid)
    d_out, d_pk, d_fix = fill(n * 64), fill(n * 16), dev(np.zeros(1, gpsacq.FIX_DTYPE))
    torch.cuda.synchronize()
    args = lambda **kv: dict(dict(inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=n_samples, d_aid_ptr=d_aid.data_ptr(), n_tasks=n, d_aided_ptr=d_out.data_ptr(),
                                  d_peaks_out_ptr=d_pk.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr(), params=prm), **kv)
    for kv in (dict(d_iq_ptr=d_iq.data_ptr() + 8), dict(d_iq_ptr=d_iq.data_ptr() + 2), dict(d_iq_ptr=None), dict(stride=80008), dict(n_samples=0),
               dict(n_tasks=0), dict(d_aid_ptr=None), dict(d_aided_ptr=None), dict(d_peaks_out_ptr=None), dict(d_peaks_in_ptr=d_pk.data_ptr()),
               dict(inp=eng.iq8_input(signed=True, multibit=7))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.aided_search_iq8_device(**args(**kv))
        assert ei.value.code == 1, kv
    rec = to_records([aided_cases.scene_sats()[0]["ephs"][0]])
    for kv in (dict(d_iq_ptr=d_iq.data_ptr() + 4), dict(d_fix_ptr=None), dict(n_chans=13), dict(stride=80008), dict(inp=eng.iq8_input(signed=True, multibit=7))):
        a = dict(dict(eph=rec, d_fix_ptr=d_fix.data_ptr(), inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=n_samples, d_tasks_ptr=None, n_fix=1, n_chans=1,
                      d_aided_ptr=d_out.data_ptr(), d_peaks_out_ptr=d_pk.data_ptr(), stride=stride), **kv)
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.aided_peaks_iq8_device(**a)
        assert ei.value.code == 1, kv
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_pk.cpu().numpy() == 0xA5).all()
    # an engine that accumulates blocks is refused as gpsacq_aided_search refuses it
    with gpsacq.Engine(FC, FS, 5000.0) as e2:
        e2.set_noncoherent(2)
        with pytest.raises(gpsacq.GpsAcqError) as err:
            e2.aided_search_iq8(cut, inp, aid, tasks=tasks, stride=stride, params=prm)
        assert err.value.code == 3  # GPSACQ_ERR_UNSUPPORTED


# ---- 3. sign mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed,dc", [(True, False), (False, True)])
def test_sign_mode_is_the_one_bit_path(eng, capture, signed, dc):
    """GPSACQ_SAMPLES_SIGN = gpsacq_iq8_to_bits_device, then gpsacq_aided_search_device with stride / 16, byte for byte; remove_dc with
    the mean gpsacq_iq8_to_bits_device itself finds; and the reference's sign mode agrees"""
    import gpsacq
    import torch
    iq = np.ascontiguousarray(capture if signed else ic.as_u8(capture))
    n_samples = iq.size // 2 - 3  # the last byte of the 1-bit stream is not full
    n_bytes = (n_samples + 7) // 8
    tasks, aid = hand_aid(eng, 24, seed=7)
    pin = np.zeros(24, gpsacq.PEAK_DTYPE)
    pin[5] = (31.0, 4, 77, 9.0)
    stride = 80016
    raw = iq.view(np.int8).astype(np.int64)[:2 * n_samples].reshape(-1, 2) if signed else iq.view(np.uint8).astype(np.int64)[:2 * n_samples].reshape(-1, 2) - 128
    mean = (raw[:, 0].sum() / n_samples, raw[:, 1].sum() / n_samples) if dc else (0.0, 0.0)
    inp = eng.iq8_input(signed=signed, remove_dc=dc, mean=mean, mix_hz=FC - IF_HZ, multibit=0)
    d_iq, d_tasks, d_aid, d_pin = dev(iq), dev(tasks), dev(aid), dev(pin)
    n_pw = 24 * 3 * 81 * 8
    d_bits, a1, p1, w1, a2, p2, w2 = fill(n_bytes + 16), fill(24 * 64), fill(24 * 16), fill(n_pw), fill(24 * 64), fill(24 * 16), fill(n_pw)
    torch.cuda.synchronize()
    rc = eng._lib.gpsacq_iq8_to_bits_device(eng._h, d_iq.data_ptr(), n_samples, 1 if signed else 0, 1 if dc else 0, FC - IF_HZ, 0.0, d_bits.data_ptr(), 1)
    assert rc == 0
    prm = gpsacq.aided_params(blocks=3, code_half=40, dop_half=1, ratio_min=1.2)
    eng.aided_search_device(d_bits.data_ptr(), n_bytes, d_aid.data_ptr(), 24, a1.data_ptr(), p1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(),
                            d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=w1.data_ptr(), params=prm)
    eng.aided_search_iq8_device(inp, d_iq.data_ptr(), n_samples, d_aid.data_ptr(), 24, a2.data_ptr(), p2.data_ptr(), stride=stride,
                                d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr(), d_powers_ptr=w2.data_ptr(), params=prm)
    ms = eng.aided_iq8_last_ms()
    one = [x.cpu().numpy().tobytes() for x in (a1, p1, w1)]
    rec = np.frombuffer(one[0], gpsacq.AIDED_DTYPE)
    print("sign mode %s dc %d: conversion %.4f ms, k_aided %.4f ms; %d records, flags %s" %
          ("S8" if signed else "U8", dc, ms[0], ms[2], rec.size, sorted(set(rec["flags"].tolist()))))
    assert [x.cpu().numpy().tobytes() for x in (a2, p2, w2)] == one
    assert ms[0] > 0 and ms[1] == 0 and ms[2] > 0 and rec["flags"][5] == gpsacq.AIDED_KEPT and (rec["floor"][rec["flags"] != 1] == 2 * SPM * 21).all()
    host, hpk, hpw = eng.aided_search_iq8(iq, inp, aid, tasks=tasks, peaks_in=pin, stride=stride, params=prm, powers=True, n_samples=n_samples)
    assert [host.tobytes(), hpk.tobytes(), hpw.tobytes()] == one
    ref = reference(eng, iq, stride, tasks, aid, peaks_in=pin, n_samples=n_samples, blocks=3, code_half=40, dop_half=1, ratio_min=1.2, signed=signed,
                    mean=mean if dc else None, mix_hz=FC - IF_HZ, multibit=0)
    aided_iq_ref.same(host, ref, hpk, hpw, "sign mode")
    # params == NULL in sign mode are gpsacq_aided_default_params (ratio_min 1.922), not the multi-bit path's
    b1, q1, b2, q2 = fill(24 * 64), fill(24 * 16), fill(24 * 64), fill(24 * 16)
    torch.cuda.synchronize()
    eng.aided_search_device(d_bits.data_ptr(), n_bytes, d_aid.data_ptr(), 24, b1.data_ptr(), q1.data_ptr(), stride=stride // 16, d_tasks_ptr=d_tasks.data_ptr(),
                            d_peaks_in_ptr=d_pin.data_ptr())
    eng.aided_search_iq8_device(inp, d_iq.data_ptr(), n_samples, d_aid.data_ptr(), 24, b2.data_ptr(), q2.data_ptr(), stride=stride,
                                d_tasks_ptr=d_tasks.data_ptr(), d_peaks_in_ptr=d_pin.data_ptr())
    assert b2.cpu().numpy().tobytes() == b1.cpu().numpy().tobytes() and q2.cpu().numpy().tobytes() == q1.cpu().numpy().tobytes()


# ---- 4. the chain, end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weak_scene(eng):
    """tests/aided_cases.py's scene as a 16-block IQ capture by Engine.generate_iq8 (IF 0.4 MHz, scale 16, sigma 1, int8): five satellites
    at 0.2, one at aided_iq_cases.WEAK_AMPLITUDE, two absent; block 0 searched for all eight in multi-bit mode"""
    import gpsacq
    geo, sel, present, absent, dops = aided_cases.scene_sats(weak=ic.WEAK_AMPLITUDE)
    iq = eng.generate_iq8(16 * 40960, present, if_hz=ic.IF_HZ, scale=ic.SCALE, signed=True, noise_sigma=1.0, seed=2024)
    chans = present + absent
    tasks = np.array([(0, s[0] - 1) for s in chans], np.int32)
    inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=FC - ic.IF_HZ, multibit=REAL)
    _, peaks = eng.search_iq8(iq[:2 * 40960], inp, tasks=tasks, want_cells=False)
    iq.setflags(write=False)
    blk_ms, blk_frac = block_times(geo["ref_ms"] + 4321, aided_cases.REF_FRAC, 1, 40960, FS)
    fix = np.zeros(1, gpsacq.FIX_DTYPE)
    fix["status"], fix["n_used"], fix["rx_ms"], fix["rx_frac"] = 0, 8, blk_ms, blk_frac
    fix["x"], fix["y"], fix["z"] = geo["rx"]
    return dict(geo=geo, rec=to_records([geo["ephs"][k] for k in sel]), iq=iq, inp=inp, chans=chans, tasks=tasks, peaks=peaks, fix=fix,
                prior=priors(geo, blk_ms, seed=3, km=30.0, secs=20.0))


def test_chain_and_end_to_end(eng, weak_scene):
    """gpsacq_aided_peaks_iq8_device = gpsacq_aid_predict_device + gpsacq_aided_search_iq8_device byte for byte, with and without the
    optional buffer; host form = device form; and the records equal the reference.  Then the scene: the weak satellite, below the
    search threshold in block 0, is found by the multi-bit search with the defaults at its true code phase; the absent PRNs are not;
    the merged peaks go into gpsacq_refine_iq8 and the coarse-time fix unchanged.

    Measured on an MI355X (printed by this test): the search of block 0 gives the five strong satellites snr 170 to 213, the weak one
    (amplitude 0.04) 14.52 and the absent ones 13.49 and 14.61.  The multi-bit aided search keeps the five, finds the weak one at ratio
    3.9197 (ratio_min 3.44), ca_shift 4627 against the law's 4626.77, and reads the absent ones at 1.4374 and 1.4404 -- the CPU's
    figures for tests/gen_ref.py's capture to the digit.  k_aid_predict 0.028 ms, k_aided_iq 4.07 ms for the 8 tasks, 3 of them
    searched; the fix from six satellites lies 5.4 m from the truth."""
    import gpsacq
    import torch
    w = weak_scene
    n = len(w["chans"])
    ns = w["iq"].size // 2
    d_iq, d_tasks, d_pin, d_fix = dev(w["iq"]), dev(w["tasks"]), dev(w["peaks"]), dev(w["fix"])
    d_aid, d_out, d_pk = fill(n * 40), fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aid_predict_device(w["rec"], d_fix.data_ptr(), 1, n, d_aid.data_ptr(), sync=False)
    eng.aided_search_iq8_device(w["inp"], d_iq.data_ptr(), ns, d_aid.data_ptr(), n, d_out.data_ptr(), d_pk.data_ptr(), d_tasks_ptr=d_tasks.data_ptr(),
                                d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    steps = [x.cpu().numpy().tobytes() for x in (d_aid, d_out, d_pk)]
    e_aid, e_out, e_pk = fill(n * 40), fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_peaks_iq8_device(w["rec"], d_fix.data_ptr(), w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), 1, n, e_out.data_ptr(), e_pk.data_ptr(),
                               d_peaks_in_ptr=d_pin.data_ptr(), d_aid_ptr=e_aid.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (e_aid, e_out, e_pk)] == steps
    ms = eng.aided_iq8_last_ms()
    f_out, f_pk = fill(n * 64), fill(n * 16)
    torch.cuda.synchronize()
    eng.aided_peaks_iq8_device(w["rec"], d_fix.data_ptr(), w["inp"], d_iq.data_ptr(), ns, d_tasks.data_ptr(), 1, n, f_out.data_ptr(), f_pk.data_ptr(),
                               d_peaks_in_ptr=d_pin.data_ptr(), sync=True)
    assert [x.cpu().numpy().tobytes() for x in (f_out, f_pk)] == steps[1:]
    aid = np.frombuffer(steps[0], gpsacq.AID_DTYPE)
    got = np.frombuffer(steps[1], gpsacq.AIDED_DTYPE)
    pk = np.frombuffer(steps[2], gpsacq.PEAK_DTYPE)
    host, hpk = eng.aided_search_iq8(w["iq"], w["inp"], aid, tasks=w["tasks"], peaks_in=w["peaks"])  # params None: the iq8 defaults
    assert host.tobytes() == steps[1] and hpk.tobytes() == steps[2]
    ref = reference(eng, w["iq"], 81920, w["tasks"], aid, peaks_in=w["peaks"], signed=True, mix_hz=FC - ic.IF_HZ, multibit=REAL)
    aided_iq_ref.same(got, ref, pk, None, "end to end")
    snr = w["peaks"]["snr"]
    ca_law, lo_law = aided_cases.law_center(w["chans"][5], 0)
    print("search snr of block 0: strong %s, weak %.2f, absent %.2f %.2f" % (np.round(snr[:5], 1), snr[5], snr[6], snr[7]))
    print("aided, multi-bit: flags %s, ratios %s (ratio_min %.3f); weak PRN (amplitude %g) at ca_shift %d (law %.2f), lo_shift %d (law %.2f); "
          "k_aid_predict %.4f ms, k_aided_iq %.4f ms for %d tasks" % (got["flags"].tolist(), np.round(got["ratio"], 4), aided_iq_ref.RATIO_MIN,
                                                                       ic.WEAK_AMPLITUDE, got["ca_shift"][5], ca_law, got["lo_shift"][5], lo_law, ms[1], ms[2], n))
    assert ms[0] == 0 and ms[1] > 0 and ms[2] > 0
    assert float(gpsacq.aided_params_iq8()["ratio_min"][0]) == aided_iq_ref.RATIO_MIN
    assert (snr[:5] >= gpsacq.THRESHOLD).all() and snr[5] < gpsacq.THRESHOLD
    assert (got["flags"][:5] == gpsacq.AIDED_KEPT).all() and pk[:5].tobytes() == w["peaks"][:5].tobytes()
    assert got["flags"][5] == 0 and got["ratio"][5] >= aided_iq_ref.RATIO_MIN
    assert abs((got["ca_shift"][5] - ca_law + SPM / 2) % SPM - SPM / 2) <= 1.0 and abs(got["lo_shift"][5] - lo_law) <= 1.5
    assert (got["flags"][6:] == gpsacq.AIDED_BELOW).all() and pk[6:].tobytes() == bytes(32)
    # downstream, unchanged: refine_iq8 accepts the merged peaks at snr_min = ratio_min, and the coarse-time fix takes all six
    fine = eng.refine_iq8(w["iq"], w["inp"], pk.copy(), tasks=w["tasks"], params=gpsacq.refine_params(snr_min=aided_iq_ref.RATIO_MIN))
    assert (fine["flags"][:6] == 0).all() and (fine["flags"][6:] == gpsacq.FINE_NO_HIT).all() and fine["prompt"][5] == got["best"][5]
    obs = eng.coarse_obs(pk.copy().reshape(1, n), fine=fine.reshape(1, n), snr_min=aided_iq_ref.RATIO_MIN)
    fixes, info, _ = eng.coarse_fix(w["rec"], obs, w["prior"])
    err = float(np.linalg.norm(np.array([fixes["x"][0], fixes["y"][0], fixes["z"][0]]) - w["geo"]["rx"]))
    print("refine_iq8 at snr_min = ratio_min: flags %s, offset of the weak PRN %.3f chips; coarse-time fix from %d satellites, %.1f m from the truth" %
          (fine["flags"].tolist(), fine["offset_chips"][5], fixes["n_used"][0], err))
    # half a chip of range is 147 m; six fine code phases good to metres at a PDOP of a few stay well inside it
    assert fixes["status"][0] == 0 and fixes["n_used"][0] == 6 and info["flags"][0] == 0 and err <= 147.0
