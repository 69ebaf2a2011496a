"""Snapshot signal quality on an 8-bit IQ capture on the GPU (gpsacq_snap_floor_iq8*, gpsacq_snap_quality_iq8*,
gpsacq_coarse_fix_quality_iq8_device) against tests/snapq_iq_ref.py, the restatement of "Snapshot signal quality on an 8-bit IQ
capture" of include/gpsacq.h.

Every floor must equal the reference's integer, every field of an info record its bytes, except cn0_dbhz, which may differ by
snapq_ref.CN0_TOL = 1e-9 dB (log10 is the one libm call).  The captures are those of tests/test_gpu_snapshot_iq.py: four blocks plus
1000 samples, three satellites, about 330 KB, made once with Engine.generate_iq8.  k_iq_energy's chunk is 1024 samples: a block of
stride 80000 or 80016 bytes starts off a chunk boundary, one of 81920 bytes on it.  Each test prints what it measured before it
asserts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import coarse_ref
import snapq_iq_ref as sqi
import snapq_ref as sq
from coarse_helpers import block_times, priors, synth_sats
from nav_helpers import geometry, to_records
from test_coarse import POS_TOL

pytestmark = pytest.mark.gpu

FS, FC, SPM, IF_HZ = 5.456e6, 4.092e6, 5456, 2000.0
REAL, COMPLEX = 1, 2
MEAN = (3.4, -2.6)
CHUNK = 1024


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


def inp_of(eng, signed, dc, multibit):
    return eng.iq8_input(signed=signed, remove_dc=dc, mean=MEAN if dc else (0.0, 0.0), mix_hz=-IF_HZ if multibit == COMPLEX else FC - IF_HZ,
                         multibit=multibit)


def hand_peaks(dmax, n, seed, max_block=1):
    """tests/test_gpu_snapshot_iq.py's hand-made hits: ca_shift x lo_shift x PRN 1 and 32 cycled, blocks 0 .. max_block"""
    import gpsacq
    combos = [(ca, lo, prn) for ca in (0, 1, 2727, SPM - 1) for lo in (-dmax, 0, dmax) for prn in (0, 31)]
    order = np.random.default_rng(seed).permutation(len(combos))
    pk = np.zeros(n, gpsacq.PEAK_DTYPE)
    tasks = np.zeros((n, 2), np.int32)
    for t in range(n):
        ca, lo, prn = combos[order[t % len(combos)]]
        pk[t] = (30.0 + t, lo, ca, 1.0)
        tasks[t] = (t % (max_block + 1), prn)
    return tasks, pk


def hand_fine(rows):
    """FINE_DTYPE records of (flags, segments, prompt); the other fields are filled so that nothing else can matter"""
    import gpsacq
    out = np.zeros(len(rows), gpsacq.FINE_DTYPE)
    for i, (flags, segments, prompt) in enumerate(rows):
        out[i] = (flags, segments, 0xDEADBEEF, 0x12345678, prompt // 3, prompt, prompt // 5, 0.125, 0.25e-3)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def fill(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")


def shapes(tasks, fine, stride):
    """which head / tail shapes the windows of these records have: (start on a chunk boundary, end on one) per usable record"""
    out = set()
    for (block, _), r in zip(np.asarray(tasks).reshape(-1, 2).tolist(), fine.ravel()):
        if r["segments"] > 0 and not r["flags"] & sq.FINE_UNUSABLE:
            o = block * (stride // 2)
            out.add((o % CHUNK == 0, (o + int(r["segments"]) * SPM) % CHUNK == 0))
    return out


# ---- 1. exact against the reference ------------------------------------------------------------------------------------------------
# blocks x stride, all 9; format, remove_dc and REAL / COMPLEX go through their eight combinations along the list; then one task and
# five tasks
_MODES = [(signed, dc, mb) for signed in (True, False) for dc in (False, True) for mb in (REAL, COMPLEX)]
CASES = [(b, s, 24) + _MODES[(3 * i + k) % 8] for i, b in enumerate((1, 2, 3)) for k, s in enumerate((80000, 80016, 81920))] + [
    (2, 80016, 1, False, True, REAL), (2, 81920, 5, True, True, COMPLEX)]


@pytest.mark.parametrize("blocks,stride,n_tasks,signed,dc,multibit", CASES)
def test_exact_against_the_reference(eng, capture, blocks, stride, n_tasks, signed, dc, multibit):
    import gpsacq
    tasks, pk = hand_peaks(eng.dmax, n_tasks, seed=blocks * 100 + stride)
    iq = capture if signed else as_u8(capture)
    inp, mean = inp_of(eng, signed, dc, multibit), MEAN if dc else None
    fine = eng.refine_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=blocks)).reshape(-1, 6 if n_tasks == 24 else n_tasks)
    prm = gpsacq.snap_quality_params_iq8()
    floors = eng.snap_floor_iq8(iq, inp, fine, tasks=tasks, stride=stride)
    _, info = eng.snap_quality_iq8(iq, inp, fine, tasks=tasks, stride=stride)
    rfl, rinfo = sqi.quality(iq, stride, tasks.tolist(), fine, SPM, FS, signed=signed, mean=mean, params=prm)
    label = "blocks %d stride %d %s dc %d multibit %d" % (blocks, stride, "S8" if signed else "U8", dc, multibit)
    print("%s, %d tasks: floors %d .. %d, C/N0 %.2f .. %.2f dB-Hz, shapes (start on a boundary, end on one) %s; floors %.4f ms, quality %.4f ms" %
          ((label, n_tasks, floors.min(), floors.max(), info["cn0_dbhz"].min(), info["cn0_dbhz"].max(), sorted(shapes(tasks, fine, stride))) +
           eng.snap_quality_iq8_last_ms()))
    assert (fine["flags"] == 0).all() and (fine["segments"] == blocks * 40000 // SPM).all()
    assert floors.dtype == np.uint64 and floors.tolist() == rfl.tolist() and floors.min() > 0
    worst = sq.same(info, rinfo, label)
    assert worst <= sq.CN0_TOL and (info["noise"] == floors).all() and (info["flags"] & ~sq.NO_POWER == 0).all()  # (most hits are no satellite's)
    ms = eng.snap_quality_iq8_last_ms()
    assert ms[0] > 0 and ms[1] > 0
    if n_tasks == 24:
        assert shapes(tasks, fine, stride) == ({(True, False)} if stride == 81920 else {(True, False), (False, False)})


def test_head_whole_chunks_and_tail(eng, capture):
    """hand-made records whose windows start on a chunk boundary and off it and end on one and off it: at 5456 samples per
    millisecond and stride 80000, block 1 starts 64 samples past a boundary and 12 segments from there end on one; a window start on
    a boundary with its end on one too needs 64 segments, more than this capture holds, so the end on a boundary has its start off"""
    stride = 80000
    rows = [(0, 0, 7), (1, 0, 7), (1, 0, 12), (0, 0, 1), (2, 0, 15), (3, 2, 8), (0, 0, 30)]
    tasks = np.array([(r[0], 0) for r in rows], np.int32)
    fine = hand_fine([(r[1], r[2], 10 ** 10) for r in rows]).reshape(1, -1)
    assert shapes(tasks, fine, stride) == {(True, False), (False, False), (False, True)} and (40000 + 12 * SPM) % CHUNK == 0
    for signed, dc in ((False, True), (True, False)):
        iq = capture if signed else as_u8(capture)
        inp = inp_of(eng, signed, dc, REAL)
        floors = eng.snap_floor_iq8(iq, inp, fine, tasks=tasks, stride=stride)
        rfl, rinfo = sqi.quality(iq, stride, tasks.tolist(), fine, SPM, FS, signed=signed, mean=MEAN if dc else None)
        _, info = eng.snap_quality_iq8(iq, inp, fine, tasks=tasks, stride=stride)
        print("%s dc %d: floors %s" % ("S8" if signed else "U8", dc, floors.ravel().tolist()))
        assert floors.tolist() == rfl.tolist() and floors.min() > 0
        sq.same(info, rinfo, "shapes")


# ---- 2. an engine whose spm is odd -------------------------------------------------------------------------------------------------
def test_an_odd_number_of_samples_per_millisecond():
    """fs = 2.047 MHz, fc = 0.4 MHz, 2047 samples per millisecond, U8, mean removed: windows of 1, 2, 3 and 39 segments end in the
    middle of a 16-byte group and, where segments is odd, of a dword; the last one ends with the capture.  The bytes are random and
    reach both rails (the floor needs no satellite)."""
    import gpsacq
    fs, fc, spm, stride = 2.047e6, 0.4e6, 2047, 80000
    n_samples = 40000 + 39 * spm
    assert n_samples % 8 == 1
    rng = np.random.default_rng(21)
    iq = rng.integers(0, 256, 2 * n_samples, dtype=np.uint8)
    iq[:64], iq[64:128] = 0, 255
    rows = [(0, 1), (0, 2), (0, 3), (0, 39), (1, 1), (1, 2), (1, 3), (1, 39), (3, 1), (1, 40)]  # the last two are not of this capture
    tasks = np.array([(b, 0) for b, _ in rows], np.int32)
    fine = hand_fine([(0, s, 2 * spm * s * 3) for _, s in rows]).reshape(2, 5)
    mean = (3.5, -128.0)  # nearbyint: 4 (ties to even) and -128
    with gpsacq.Engine(fc, fs, 5000.0) as e:
        assert e.num_lags == spm
        inp = e.iq8_input(signed=False, remove_dc=True, mean=mean, mix_hz=fc, multibit=REAL)
        floors = e.snap_floor_iq8(iq, inp, fine, tasks=tasks, stride=stride)
        _, info = e.snap_quality_iq8(iq, inp, fine, tasks=tasks, stride=stride)
    rfl, rinfo = sqi.quality(iq, stride, tasks.tolist(), fine, spm, fs, signed=False, mean=mean, params=gpsacq.snap_quality_params_iq8())
    ends = [(b * 40000 + s * spm) % 8 for b, s in rows[:8]]
    print("spm %d: floors %s, window ends modulo 8 %s" % (spm, floors.ravel().tolist(), ends))
    assert any(x % 2 for x in ends) and all(ends)  # mid-dword and mid-group
    assert floors.ravel().tolist() == rfl.ravel().tolist() and (floors.ravel()[:8] > 0).all() and floors.ravel()[8:].tolist() == [0, 0]
    sq.same(info, rinfo, "spm 2047")
    # 2047 >= 2 * 1024 - 1: at this rate every window holds a whole chunk.  A window with none needs fewer than 2047 samples per
    # millisecond: fs = 1.2 MHz (1200), where one segment of block 1 (sample 40000, 64 past a boundary) is a head of 960 samples and
    # a tail of 240.  A window that lies INSIDE one chunk cannot exist at a chunk of 1024 (no engine has fewer than 1138 samples per
    # millisecond); the kernel's branch for it serves other chunk sizes.
    fs2, fc2, spm2 = 1.2e6, 0.3e6, 1200
    rows2 = [(1, 1), (0, 1), (1, 2), (2, 1)]
    n2 = 80000 + spm2
    iq2 = rng.integers(0, 256, 2 * n2, dtype=np.uint8).view(np.int8)
    tasks2 = np.array([(b, 0) for b, _ in rows2], np.int32)
    fine2 = hand_fine([(0, s, 7 * spm2 * s) for _, s in rows2]).reshape(1, 4)
    with gpsacq.Engine(fc2, fs2, 5000.0) as e:
        assert e.num_lags == spm2
        inp2 = e.iq8_input(signed=True, remove_dc=True, mean=(-2.5, 7.0), mix_hz=fc2, multibit=REAL)
        floors2 = e.snap_floor_iq8(iq2, inp2, fine2, tasks=tasks2, stride=stride)
    rfl2 = [f for _, f in sqi.floors(iq2, stride, tasks2.tolist(), fine2, spm2, signed=True, mean=(-2.5, 7.0))]
    print("spm %d: floors %s" % (spm2, floors2.ravel().tolist()))
    assert -(-40000 // CHUNK) == (40000 + spm2) // CHUNK  # no whole chunk between the start and the end of row 0
    assert floors2.ravel().tolist() == rfl2 and min(rfl2) > 0


# ---- 3. records that are not of this capture ---------------------------------------------------------------------------------------
def test_records_that_are_not_of_this_capture(eng, capture):
    """segments = 2251 on the four-block capture, a block past its end, a negative block, unusable flags: NO_RECORD with floor 0; the
    device form with 0xA5 behind the capture's last byte (which is not the buffer's) and behind every output gives the host form's
    bytes and leaves the guards alone"""
    import gpsacq
    import torch
    stride = 80000
    n_samples = 3 * 40000 + 7 * SPM + 2733  # ends in the middle of a 16-byte group
    assert n_samples % 8 == 5
    rows = [(0, 0, 21), (0, 0, 2251), (5, 0, 7), (-1, 0, 7), (3, 0, 7), (3, 0, 8), (1, 1, 7), (1, 4, 7), (1, 8, 7), (1, 2, 7), (1, 0, 0), (1, 0, -2)]
    tasks = np.array([(r[0], 0) for r in rows], np.int32)
    fine = hand_fine([(r[1], r[2], 10 ** 9) for r in rows]).reshape(2, 6)
    want = [True, False, False, False, True, False, False, False, False, True, False, False]
    n = len(rows)
    u8 = as_u8(capture)
    inp = inp_of(eng, False, True, COMPLEX)
    cut = np.ascontiguousarray(u8[:2 * n_samples])
    rfl, rinfo = sqi.quality(cut, stride, tasks.tolist(), fine, SPM, FS, signed=False, mean=MEAN, params=gpsacq.snap_quality_params_iq8())
    floors = eng.snap_floor_iq8(cut, inp, fine, tasks=tasks, stride=stride)
    _, info = eng.snap_quality_iq8(cut, inp, fine, tasks=tasks, stride=stride)
    print("floors %s, flags %s" % (floors.ravel().tolist(), info["flags"].ravel().tolist()))
    assert [bool(f) for f in floors.ravel()] == want and floors.tolist() == rfl.tolist()
    sq.same(info, rinfo, "not of this capture")
    blank = np.int32(0).tobytes() + np.int32(sq.NO_RECORD).tobytes() + bytes(40)
    assert all(info.ravel()[k].tobytes() == blank for k in range(n) if not want[k])
    buf = np.full(2 * n_samples + 150, 0xA5, np.uint8)
    buf[:2 * n_samples] = cut
    d_iq, d_tasks, d_fine = dev(buf), dev(tasks), dev(fine)
    d_floor, d_info, d_floor2 = fill(n * 8 + 64), fill(n * 48 + 64), fill(n * 8 + 64)
    torch.cuda.synchronize()
    eng.snap_floor_iq8_device(inp, d_iq.data_ptr(), n_samples, d_fine.data_ptr(), n, d_floor2.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr())
    eng.snap_quality_iq8_device(inp, d_iq.data_ptr(), n_samples, d_fine.data_ptr(), 2, 6, d_info.data_ptr(), d_floor_ptr=d_floor.data_ptr(), stride=stride,
                                d_tasks_ptr=d_tasks.data_ptr())
    h_floor, h_info, h_floor2 = d_floor.cpu().numpy(), d_info.cpu().numpy(), d_floor2.cpu().numpy()
    assert h_floor[:n * 8].tobytes() == floors.tobytes() == h_floor2[:n * 8].tobytes() and h_info[:n * 48].tobytes() == info.tobytes()
    assert (h_floor[n * 8:] == 0xA5).all() and (h_floor2[n * 8:] == 0xA5).all() and (h_info[n * 48:] == 0xA5).all()
    assert d_iq.cpu().numpy().tobytes() == buf.tobytes()


# ---- 4. the floor is the aided search's --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,stride,signed,dc", [(2, 80016, True, True), (3, 81920, False, False)])
def test_the_floor_is_the_aided_search_s(eng, capture, blocks, stride, signed, dc):
    import gpsacq
    tasks, pk = hand_peaks(eng.dmax, 12, seed=3, max_block=1)
    pk["lo_shift"] = np.clip(pk["lo_shift"], -eng.dmax + 1, eng.dmax - 1)
    iq = capture if signed else as_u8(capture)
    inp = inp_of(eng, signed, dc, REAL)
    fine = eng.refine_iq8(iq, inp, pk, tasks=tasks, stride=stride, params=gpsacq.refine_params(blocks=blocks)).reshape(2, 6)
    aid = np.zeros(12, gpsacq.AID_DTYPE)
    aid["ca_center"], aid["lo_center"] = pk["ca_shift"], pk["lo_shift"]
    aided, _ = eng.aided_search_iq8(iq, inp, aid, tasks=tasks, stride=stride, params=gpsacq.aided_params_iq8(blocks=blocks, code_half=2, dop_half=0))
    floors = eng.snap_floor_iq8(iq, inp, fine, tasks=tasks, stride=stride)
    print("blocks %d stride %d: floors %s" % (blocks, stride, floors.ravel().tolist()))
    assert (aided["segments"] == fine["segments"].ravel()).all() and (aided["floor"] > 0).all()
    assert floors.ravel().tolist() == aided["floor"].tolist()


# ---- 5. sign mode ------------------------------------------------------------------------------------------------------------------
def test_sign_mode_is_snap_quality(eng, capture):
    """GPSACQ_SAMPLES_SIGN: byte for byte Engine.snap_quality on the records of sign-mode refine_iq8, with the 1-bit defaults; the
    floors are 2 * spm * segments"""
    import gpsacq
    import torch
    tasks, pk = hand_peaks(eng.dmax, 24, seed=7, max_block=1)
    inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=FC - IF_HZ, multibit=0)
    fine = eng.refine_iq8(capture, inp, pk, tasks=tasks, stride=80016, params=gpsacq.refine_params(blocks=3)).reshape(4, 6)
    fine["flags"][0, 0], fine["segments"][0, 1] = 1, 0  # two records that are none
    obs = eng.coarse_obs(pk.reshape(4, 6), fine=fine)
    for prm in (None, gpsacq.snap_quality_params(cn0_ref_dbhz=46.0, min_segments=21)):
        want_obs, want = eng.snap_quality(fine, obs=obs, params=prm)
        got_obs, got = eng.snap_quality_iq8(capture, inp, fine, tasks=tasks, obs=obs, stride=80016, params=prm)
        assert got.tobytes() == want.tobytes() and got_obs.tobytes() == want_obs.tobytes()
    floors = eng.snap_floor_iq8(capture, inp, fine, tasks=tasks, stride=80016)
    record = (fine["flags"] & sq.FINE_UNUSABLE == 0) & (fine["segments"] > 0)
    print("sign mode: C/N0 %.2f .. %.2f dB-Hz, floors %s" % (want["cn0_dbhz"][record].min(), want["cn0_dbhz"].max(), sorted(set(floors.ravel().tolist()))))
    assert floors.tolist() == np.where(record, 2 * SPM * fine["segments"].astype(np.int64), 0).tolist() and record.sum() == 22
    assert set(want["flags"].ravel().tolist()) == {0, sq.NO_POWER, sq.NO_RECORD} and (want["lin"] > 0).any()  # (most hits are no satellite's)
    # the device form writes the floors only where they are asked for
    d_iq, d_tasks, d_fine = dev(capture), dev(tasks), dev(fine)
    d_info, d_floor = fill(24 * 48), fill(24 * 8)
    torch.cuda.synchronize()
    eng.snap_quality_iq8_device(inp, d_iq.data_ptr(), capture.size // 2, d_fine.data_ptr(), 4, 6, d_info.data_ptr(), stride=80016, d_tasks_ptr=d_tasks.data_ptr(),
                                params=prm)
    assert d_info.cpu().numpy().tobytes() == want.tobytes() and eng.snap_quality_iq8_last_ms()[0] == 0 and eng.snap_quality_iq8_last_ms()[1] > 0
    eng.snap_quality_iq8_device(inp, d_iq.data_ptr(), capture.size // 2, d_fine.data_ptr(), 4, 6, d_info.data_ptr(), d_floor_ptr=d_floor.data_ptr(),
                                stride=80016, d_tasks_ptr=d_tasks.data_ptr(), params=prm)
    assert d_floor.cpu().numpy().tobytes() == floors.tobytes() and eng.snap_quality_iq8_last_ms()[0] > 0


# ---- 6. host form, device form and chain -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(eng):
    """the scene of tests/test_gpu_snap_quality.py's chain test as an IQ capture: the northern receiver's eight satellites, six at
    amplitude 0.2 and two at 0.1, seven blocks, blocks 0..3 searched with search_iq8 in multi-bit mode and refined over four blocks"""
    geo = geometry("north")
    sel = geo["subsets"][8]
    ephs = [geo["ephs"][k] for k in sel]
    n_blocks, n_search, spb = 7, 4, 40960
    first_sample = 8 * 1_234_567
    ref_ms, ref_frac = geo["ref_ms"] + 4321, 0.6180e-3
    sats, _ = synth_sats(geo, sel, ref_ms, ref_frac, first_sample, FS, 0.2)
    sats = [tuple(s[:1]) + ((0.1,) if k in (2, 5) else (0.2,)) + tuple(s[2:]) for k, s in enumerate(sats)]
    iq = eng.generate_iq8(n_blocks * spb, sats, if_hz=IF_HZ, scale=16.0, signed=True, noise_sigma=1.0, seed=99, first_sample=first_sample)
    tasks = np.array([(b, s[0] - 1) for b in range(n_search) for s in sats], np.int32)
    inp = inp_of(eng, True, False, REAL)
    _, peaks = eng.search_iq8(iq[:2 * n_search * spb], inp, tasks=tasks, want_cells=False)
    blk_ms, _ = block_times(ref_ms, ref_frac, n_search, spb, FS)
    prior = priors(geo, blk_ms, seed=3, km=30.0, secs=20.0)
    iq.setflags(write=False)
    return dict(ephs=ephs, iq=iq, inp=inp, tasks=tasks, peaks=peaks.reshape(n_search, len(sel)), prior=prior, rec=to_records(ephs), weak=(2, 5))


def test_host_form_device_form_and_chain(eng, scene):
    """gpsacq_snap_quality_iq8 = gpsacq_snap_quality_iq8_device, and gpsacq_coarse_fix_quality_iq8_device = gpsacq_refine_iq8_device,
    gpsacq_coarse_obs_fine_device, gpsacq_snap_quality_iq8_device, gpsacq_coarse_fix_batch_device, byte for byte, with and without the
    optional buffers; the fix is tests/coarse_ref.py's on the weighted observations"""
    import gpsacq
    import torch
    n, m = scene["peaks"].shape
    inp, ns = scene["inp"], scene["iq"].size // 2
    rprm = gpsacq.refine_params(blocks=4)
    d_iq, d_tasks, d_pk, d_prior = dev(scene["iq"]), dev(scene["tasks"]), dev(scene["peaks"]), dev(scene["prior"])
    ptr = lambda t: t.data_ptr()
    sizes = dict(fine=n * m * 56, obs=n * m * 32, floor=n * m * 8, q=n * m * 48, fix=n * 80, info=n * 40, out=n * m * 32)
    a = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.refine_iq8_device(inp, ptr(d_iq), ns, ptr(d_pk), n * m, ptr(a["fine"]), d_tasks_ptr=ptr(d_tasks), params=rprm, sync=False)
    eng.coarse_obs_fine_device(ptr(d_pk), ptr(a["fine"]), n, m, ptr(a["obs"]), sync=True)
    obs_unit = np.frombuffer(a["obs"].cpu().numpy().tobytes(), gpsacq.OBS_DTYPE).reshape(n, m).copy()
    obs_unit["valid"][1, 3] = 0  # one observation that is not valid: the weights leave it alone
    raw = obs_unit.view(np.uint8).reshape(n, m, 32)
    raw[1, 3, 8:] = 0x5A
    a["obs"] = dev(obs_unit)
    eng.snap_quality_iq8_device(inp, ptr(d_iq), ns, ptr(a["fine"]), n, m, ptr(a["q"]), d_obs_ptr=ptr(a["obs"]), d_floor_ptr=ptr(a["floor"]),
                                d_tasks_ptr=ptr(d_tasks), sync=False)
    ms = eng.snap_quality_iq8_last_ms()
    eng.coarse_fix_device(scene["rec"], ptr(a["obs"]), ptr(d_prior), n, m, ptr(a["fix"]), ptr(a["info"]), ptr(a["out"]), sync=True)
    steps = {k: t.cpu().numpy().tobytes() for k, t in a.items()}
    fine = np.frombuffer(steps["fine"], gpsacq.FINE_DTYPE).reshape(n, m)
    obs = np.frombuffer(steps["obs"], gpsacq.OBS_DTYPE).reshape(n, m)
    qinfo = np.frombuffer(steps["q"], gpsacq.QUALITY_INFO_DTYPE).reshape(n, m)
    fix = np.frombuffer(steps["fix"], gpsacq.FIX_DTYPE)
    # the reference, and the host form
    rfl, rinfo = sqi.quality(scene["iq"], 81920, scene["tasks"].tolist(), fine, SPM, FS, signed=True, params=gpsacq.snap_quality_params_iq8())
    sq.same(qinfo, rinfo, "device form")
    assert np.frombuffer(steps["floor"], np.uint64).tolist() == rfl.ravel().tolist()
    h_obs, h_info = eng.snap_quality_iq8(scene["iq"], inp, fine, tasks=scene["tasks"], obs=obs_unit)
    assert h_info.tobytes() == steps["q"] and h_obs.tobytes() == steps["obs"] == sq.apply_weights(obs_unit, qinfo).tobytes()
    assert obs[1, 3].tobytes() == obs_unit[1, 3].tobytes() and ms[0] > 0 and ms[1] > 0
    weak = np.zeros(m, bool)
    weak[list(scene["weak"])] = True
    db, w = qinfo["cn0_dbhz"], qinfo["weight"]
    print("C/N0 strong %.2f .. %.2f dB-Hz, weak %.2f .. %.2f dB-Hz; weights strong %.3f .. %.3f, weak %.3f .. %.3f; floors %.4f ms, quality %.4f ms for %d tasks" %
          (db[:, ~weak].min(), db[:, ~weak].max(), db[:, weak].min(), db[:, weak].max(), w[:, ~weak].min(), w[:, ~weak].max(), w[:, weak].min(),
           w[:, weak].max(), ms[0], ms[1], n * m))
    assert (fine["flags"] == 0).all() and (qinfo["flags"] == 0).all() and w[:, weak].max() < w[:, ~weak].min() and w[:, weak].min() > 0
    # the fix is the reference's on the weighted observations
    assert (fix["status"] == 0).all() and fix["n_used"].tolist() == [m, m - 1, m, m]
    ref = coarse_ref.coarse_fix(scene["ephs"], obs, scene["prior"])
    dpos = max(float(np.linalg.norm(np.array([fix["x"][i], fix["y"][i], fix["z"][i]]) - ref[i]["xyz"])) for i in range(n))
    print("fixes against coarse_ref on the weighted observations: within %.3g m" % dpos)
    assert all(r["status"] == 0 for r in ref) and dpos <= POS_TOL
    # the chain with every optional buffer (its observations are all valid: compare with the steps run again on those)
    a2 = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.refine_iq8_device(inp, ptr(d_iq), ns, ptr(d_pk), n * m, ptr(a2["fine"]), d_tasks_ptr=ptr(d_tasks), params=rprm, sync=False)
    eng.coarse_obs_fine_device(ptr(d_pk), ptr(a2["fine"]), n, m, ptr(a2["obs"]), sync=False)
    eng.snap_quality_iq8_device(inp, ptr(d_iq), ns, ptr(a2["fine"]), n, m, ptr(a2["q"]), d_obs_ptr=ptr(a2["obs"]), d_floor_ptr=ptr(a2["floor"]),
                                d_tasks_ptr=ptr(d_tasks), sync=False)
    eng.coarse_fix_device(scene["rec"], ptr(a2["obs"]), ptr(d_prior), n, m, ptr(a2["fix"]), ptr(a2["info"]), ptr(a2["out"]), sync=True)
    steps2 = {k: t.cpu().numpy().tobytes() for k, t in a2.items()}
    b = {k: fill(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    eng.coarse_fix_quality_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_prior), ptr(b["fix"]), ptr(b["info"]),
                                      d_fine_ptr=ptr(b["fine"]), d_obs_ptr=ptr(b["obs"]), d_floor_ptr=ptr(b["floor"]), d_qinfo_ptr=ptr(b["q"]),
                                      d_obs_out_ptr=ptr(b["out"]), refine_params=rprm, sync=True)
    for k, t in b.items():
        assert t.cpu().numpy().tobytes() == steps2[k], k
    c = {k: fill(sizes[k]) for k in ("fix", "info")}
    torch.cuda.synchronize()
    eng.coarse_fix_quality_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_prior), ptr(c["fix"]), ptr(c["info"]),
                                      refine_params=rprm, sync=True)
    assert all(t.cpu().numpy().tobytes() == steps2[k] for k, t in c.items())
    ms_c = eng.snap_quality_iq8_last_ms()
    assert ms_c[0] > 0 and ms_c[1] > 0
    # ... and the fixes are the weighted ones: the unweighted chain gives other bytes
    u = {k: fill(sizes[k]) for k in ("fix", "info")}
    torch.cuda.synchronize()
    eng.coarse_fix_fine_iq8_device(scene["rec"], inp, ptr(d_iq), ns, ptr(d_tasks), ptr(d_pk), n, m, ptr(d_prior), ptr(u["fix"]), ptr(u["info"]),
                                   refine_params=rprm, sync=True)
    assert u["fix"].cpu().numpy().tobytes() != steps2["fix"]


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng, capture):
    """each returns GPSACQ_ERR_ARG and leaves every output byte as it was"""
    import gpsacq
    import torch
    stride, n, m = 80000, 2, 3
    ns = capture.size // 2
    tasks = np.array([(k % 2, 0) for k in range(n * m)], np.int32)
    fine = hand_fine([(0, 7, 10 ** 9)] * (n * m)).reshape(n, m)
    inp = inp_of(eng, True, True, REAL)
    lib, h, vp = eng._lib, eng._h, ctypes.c_void_p
    p = lambda x: x.ctypes.data_as(vp)
    ip = ctypes.byref(inp)
    obs = np.zeros((n, m), gpsacq.OBS_DTYPE)
    obs["valid"], obs["weight"] = 1, 1.0
    h_floor, h_info, h_obs = np.full(n * m, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(n * m * 48, 0xA5, np.uint8), obs.copy()
    iq = np.ascontiguousarray(capture)
    bad_inputs = [eng.iq8_input(signed=True, multibit=3), eng.iq8_input(signed=True, multibit=-1),
                  eng.iq8_input(signed=True, remove_dc=True, mean=(200.0, 0.0), multibit=REAL),
                  eng.iq8_input(signed=True, remove_dc=True, mean=(0.0, -129.0), multibit=REAL)]
    fmt = eng.iq8_input(signed=True, multibit=REAL)
    fmt.format = 2
    bad_inputs.append(fmt)
    bad_params = [gpsacq.snap_quality_params_iq8(**kw) for kw in (dict(min_segments=0), dict(cn0_min_lin=-1.0), dict(cn0_min_lin=np.nan),
                                                                  dict(cn0_ref_lin=0.0), dict(cn0_ref_lin=np.inf))]
    # the host forms
    q = lambda **kw: lib.gpsacq_snap_quality_iq8(h, kw.get("ip", ip), kw.get("iq", p(iq)), kw.get("ns", ns), kw.get("stride", stride), p(tasks),
                                                 kw.get("fine", p(fine)), kw.get("n", n), kw.get("m", m), kw.get("prm"), p(h_obs), kw.get("info", p(h_info)))
    f = lambda **kw: lib.gpsacq_snap_floor_iq8(h, kw.get("ip", ip), kw.get("iq", p(iq)), kw.get("ns", ns), kw.get("stride", stride), p(tasks),
                                               kw.get("fine", p(fine)), kw.get("n", n * m), kw.get("out", p(h_floor)))
    assert q() == 0 and f() == 0  # the good call, so that the bad ones differ from it in one argument
    h_floor[:], h_info[:], h_obs[:] = 0xA5A5A5A5A5A5A5A5, 0xA5, obs
    for kw in (dict(ip=None), dict(iq=None), dict(fine=None), dict(info=None), dict(n=0), dict(m=0), dict(m=13), dict(m=-1), dict(ns=0), dict(stride=79984),
               dict(stride=80008), dict(stride=2 ** 31 + 16)):
        assert q(**kw) == 1, kw
    for kw in (dict(ip=None), dict(iq=None), dict(fine=None), dict(out=None), dict(n=0), dict(ns=0), dict(stride=79984), dict(stride=80008),
               dict(stride=2 ** 31 + 16)):
        assert f(**kw) == 1, kw
    assert f(stride=80008) == 1 and b"stride" in lib.gpsacq_last_error()
    for bad in bad_inputs:
        assert q(ip=ctypes.byref(bad)) == 1 and f(ip=ctypes.byref(bad)) == 1
    for prm in bad_params:
        assert q(prm=p(prm)) == 1
    assert (h_floor == 0xA5A5A5A5A5A5A5A5).all() and (h_info == 0xA5).all() and h_obs.tobytes() == obs.tobytes()
    # the device forms and the chain, a misaligned pointer among them
    d_iq, d_tasks, d_fine, d_obs = dev(np.concatenate([iq.view(np.uint8), np.zeros(32, np.uint8)])), dev(tasks), dev(fine), dev(obs)
    d_floor, d_info = fill(n * m * 8), fill(n * m * 48)
    torch.cuda.synchronize()
    good = dict(inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=ns, d_fine_ptr=d_fine.data_ptr(), n_fix=n, n_chans=m, d_info_ptr=d_info.data_ptr(),
                d_obs_ptr=d_obs.data_ptr(), d_floor_ptr=d_floor.data_ptr(), stride=stride, d_tasks_ptr=d_tasks.data_ptr())
    for kw in ([dict(d_iq_ptr=d_iq.data_ptr() + 8), dict(d_iq_ptr=d_iq.data_ptr() + 2), dict(d_iq_ptr=None), dict(d_fine_ptr=None), dict(d_info_ptr=None),
                dict(n_fix=0), dict(n_chans=0), dict(n_chans=13), dict(n_samples=0), dict(stride=80008), dict(stride=79984)] +
               [dict(inp=bad) for bad in bad_inputs] + [dict(params=prm) for prm in bad_params]):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.snap_quality_iq8_device(**dict(good, **kw))
        assert ei.value.code == 1, kw
    for kw in (dict(d_iq_ptr=d_iq.data_ptr() + 4), dict(d_iq_ptr=None), dict(d_fine_ptr=None), dict(d_floor_ptr=None), dict(n_tasks=0), dict(stride=80008),
               dict(inp=bad_inputs[2])):
        a = dict(dict(inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=ns, d_fine_ptr=d_fine.data_ptr(), n_tasks=n * m, d_floor_ptr=d_floor.data_ptr(),
                      stride=stride, d_tasks_ptr=d_tasks.data_ptr()), **kw)
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.snap_floor_iq8_device(**a)
        assert ei.value.code == 1, kw
    geo = geometry("north")
    rec = to_records([geo["ephs"][k] for k in geo["subsets"][8]][:m])
    pk = np.zeros((n, m), gpsacq.PEAK_DTYPE)
    pk["snr"], pk["ca_shift"] = 40.0, 100
    blk_ms, _ = block_times(geo["ref_ms"], 0.0, n, 40000, FS)
    d_pk, d_prior = dev(pk), dev(priors(geo, blk_ms, seed=3, km=30.0, secs=20.0))
    d_fix, d_finfo, d_q = fill(n * 80), fill(n * 40), fill(n * m * 48)
    torch.cuda.synchronize()
    chain = dict(eph=rec, inp=inp, d_iq_ptr=d_iq.data_ptr(), n_samples=ns, d_tasks_ptr=d_tasks.data_ptr(), d_peaks_ptr=d_pk.data_ptr(), n_fix=n, n_chans=m,
                 d_prior_ptr=d_prior.data_ptr(), d_fix_ptr=d_fix.data_ptr(), d_info_ptr=d_finfo.data_ptr(), d_floor_ptr=d_floor.data_ptr(),
                 d_qinfo_ptr=d_q.data_ptr(), stride=stride)
    for kw in (dict(d_iq_ptr=None), dict(d_iq_ptr=d_iq.data_ptr() + 4), dict(inp=bad_inputs[0]), dict(inp=bad_inputs[2]), dict(d_peaks_ptr=None),
               dict(d_prior_ptr=None), dict(d_fix_ptr=None), dict(d_info_ptr=None), dict(n_fix=0), dict(n_chans=13), dict(n_samples=0), dict(stride=80008),
               dict(quality_params=bad_params[0]), dict(quality_params=bad_params[3]),
               dict(refine_params=np.array([(16, 0, 0.25, 25.0)], gpsacq.REFINE_PARAMS_DTYPE)), dict(params=gpsacq.coarse_params(0.0))):
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.coarse_fix_quality_iq8_device(**dict(chain, **kw))
        assert ei.value.code == 1, kw
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in (d_floor, d_info, d_fix, d_finfo, d_q)) and d_obs.cpu().numpy().tobytes() == obs.tobytes()
