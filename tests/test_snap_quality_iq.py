"""tests/snapq_iq_ref.py, the reference of "Snapshot signal quality on an 8-bit IQ capture" of include/gpsacq.h, checked on the CPU
before the kernels are held against it (tests/test_gpu_snap_quality_iq.py): where the model coincides with the 1-bit one it must
give tests/snapq_ref.py's bytes, its floor must be the aided search's, the mean identity the kernels use must be the direct sum, the
defaults must do on the 24-capture scene what the header says they do, and wrong readings of the text must show.  The references
alone, no GPU.  Each test prints what it measured before it asserts (pytest -s)."""
import numpy as np
import pytest

import aided_iq_ref
import gen_ref
import refine_iq_ref
import refine_ref
import snapq_iq_ref as sqi
import snapq_ref as sq


# ---- 1. against the 1-bit model ----------------------------------------------------------------------------------------------------
def test_against_the_one_bit_model():
    """v_q = 0, v_i = 1 - 2 x (tests/test_snapshot_iq.py, test_agreement_with_the_one_bit_references): the floor is 2 * spm *
    segments and every info byte is snapq_ref.quality's on refine_ref's records"""
    fs, fc, spm = 2.046e6, 0.4e6, 2046
    bits = np.random.default_rng(11).integers(0, 256, 3 * 5120, dtype=np.uint8)
    x = np.unpackbits(bits, bitorder="little").astype(np.int8)
    iq = np.zeros(2 * x.size, np.int8)
    iq[0::2] = 1 - 2 * x
    shifts = [lo for lo in range(-60, 61) if ((fc + lo * fs / 40000) / fs * 4294967296.0) % 1.0 < 0.5][:6]
    combos = list(zip(shifts, (0, 1, 777, spm - 1, 1022, 1500), (0, 31, 6, 0, 31, 17), (0, 1, 0, 1, 0, 1)))
    tasks = [(blk, prn) for _, _, prn, blk in combos]
    peaks = [(30.0, lo, ca, 0.0) for lo, ca, _, _ in combos]
    one = refine_ref.refine(bits, 5120, tasks, peaks, spm, fc, fs, blocks=2)
    multi = refine_iq_ref.refine(iq, 16 * 5120, tasks, peaks, spm, fc, fs, signed=True, blocks=2)
    for params in (sq.DEFAULTS, dict(sq.DEFAULTS, cn0_min_lin=0.0, cn0_ref_lin=50.0, min_segments=40)):
        fl, info = sqi.quality(iq, 16 * 5120, tasks, multi, spm, fs, signed=True, params=params)
        ref = sq.quality(one, spm, fs, params)
        print("floors %s, flags %s, lin %s" % (fl.tolist(), info["flags"].tolist(), np.round(info["lin"], 1).tolist()))
        assert fl.tolist() == [2 * spm * r["segments"] for r in one] and all(r["segments"] > 0 for r in one)
        assert info.tobytes() == ref.tobytes()
    assert (info["lin"] > 0).any() and (info["flags"] & sq.SHORT).any()
    # U8 bytes of the same samples
    u8 = (iq.astype(np.int16) + 128).astype(np.uint8)
    assert sqi.quality(u8, 16 * 5120, tasks, multi, spm, fs, signed=False, params=params)[1].tobytes() == ref.tobytes()


# ---- 2. against the aided search ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """three blocks of two satellites at 5.456 MHz, int8, with an offset so that a mean is worth removing"""
    n = 3 * 40960 + 700
    g = gen_ref.LAW.iq8(sqi.FS, [(3, 0.2, -4100.0, 100.3, 0.1), (22, 0.2, 900.0, 1801.2, 0.25)], sqi.IF_HZ, 16.0, 1.0, 9, 0, n)
    raw = gen_ref.LAW.quantise(g["v"], True).astype(np.int16)
    s8 = np.clip(raw + np.array([5, -7]), -128, 127).astype(np.int8).ravel()
    return s8, (s8.astype(np.int16) + 128).astype(np.uint8)


def test_the_floor_is_the_aided_search_s(small):
    """for the same task, blocks and min_segments the floor equals the `floor` field of tests/aided_iq_ref.py's record, a SHORT
    window at the capture's end among them"""
    s8, _ = small
    tasks = [(0, 2), (1, 21), (2, 2)]
    mix = sqi.FC - sqi.IF_HZ
    peaks = [(30.0, -30, 100, 0.0), (30.0, 7, 1801, 0.0), (30.0, -30, 55, 0.0)]
    aid = [dict(flags=0, ca_center=p[2], lo_center=p[1]) for p in peaks]
    seen = []
    for blocks, mean in ((1, None), (2, (5.2, -6.8)), (3, (5.2, -6.8))):
        fine = refine_iq_ref.refine(s8, 81920, tasks, peaks, sqi.SPM, sqi.FC, sqi.FS, signed=True, mean=mean, mix_hz=mix, blocks=blocks)
        got = sqi.floors(s8, 81920, tasks, fine, sqi.SPM, signed=True, mean=mean)
        ref = aided_iq_ref.aided_search(s8, 81920, tasks, aid, sqi.SPM, sqi.FC, sqi.FS, 36, signed=True, mean=mean, mix_hz=mix, blocks=blocks,
                                        code_half=1, dop_half=0, stream=True)
        seen.append([f for _, f in got])
        assert all(rec for rec, _ in got) and [f for _, f in got] == [r["floor"] for r in ref]
        assert [f["segments"] for f in fine] == [r["segments"] for r in ref]
    print("floors of blocks 1, 2, 3: %s" % seen)
    assert seen[2][2] < seen[2][0]  # block 2's window is cut short by the capture's end


# ---- 3. the mean identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_the_mean_identity(signed, small):
    """S2 - 2 (dc_i S_i + dc_q S_q) + n (dc_i^2 + dc_q^2) is the direct sum of (x - dc)^2: means at +-128 on both rails, a capture on
    the rails, and an ordinary one"""
    rails = np.zeros((1001, 2), np.uint8)
    rails[:, 0], rails[:, 1] = (0x7F, 0x80) if signed else (0xFF, 0x00)  # I at +127, Q at -128
    rails[::7] = rails[::7, ::-1]
    noisy = small[0] if signed else small[1]
    worst = 0
    for iq in (rails.ravel(), noisy[:2 * 4099]):
        xi, xq = refine_iq_ref.samples(iq, signed, None)
        for mean in ((128.0, -128.0), (-128.0, 128.0), (127.6, 127.5), (-128.4, -0.5), (0.4, 3.0), (0.0, 0.0)):
            dc_i, dc_q = refine_iq_ref.LAW.dc(mean[0]), refine_iq_ref.LAW.dc(mean[1])
            vi, vq = refine_iq_ref.samples(iq, signed, mean)
            direct = sqi.LAW.energy(vi, vq, 0, vi.size)
            assert sqi.mean_identity(xi, xq, dc_i, dc_q) == direct and abs(dc_i) <= 128 and abs(dc_q) <= 128, (mean, dc_i, dc_q)
            worst = max(worst, int(np.abs(vi).max()), int(np.abs(vq).max()))
    print("%s: identity = direct sum for six means on two captures; largest |v| %d" % ("S8" if signed else "U8", worst))
    assert worst >= 255  # a rail against a mean at the other end


# ---- 4. the 24-capture scene, with the defaults ------------------------------------------------------------------------------------
def test_the_scene_with_the_defaults():
    """Four satellites at amplitude 0.2, one at 0.05, one at 0.025 and two absent PRNs in 24 captures (snapq_iq_ref.scene_capture).

    Measured here, with tests/gen_ref.py, tests/refine_iq_ref.py and this reference (no GPU): strong median 48.68 dB-Hz (47.84 ..
    49.32); amplitude 0.05 median 36.83 dB-Hz, 11.89 dB below its capture's strong median (20 log10 4 = 12.04); amplitude 0.025
    median 31.46 dB-Hz, lowest 756 Hz, 10 of the 24 above the default gate of 1432.4 Hz; the 48 absent records median 77 Hz, largest 384 Hz."""
    amps, info = sqi.scene(24)
    lin, w = info["lin"], info["weight"]
    strong, a05, a025, absent = amps == 0.2, amps == 0.05, amps == 0.025, amps == 0.0
    med_strong = np.array([np.median(info["cn0_dbhz"][k][strong[k]]) for k in range(24)])
    drop = med_strong - info["cn0_dbhz"][a05]
    print("strong: median %.2f dB-Hz (%.2f .. %.2f), weights %.3f .. %.3f" %
          (np.median(info["cn0_dbhz"][strong]), info["cn0_dbhz"][strong].min(), info["cn0_dbhz"][strong].max(), w[strong].min(), w[strong].max()))
    print("amplitude 0.05: median %.2f dB-Hz, median drop below its capture's strong median %.2f dB, weights %.4f .. %.4f" %
          (np.median(info["cn0_dbhz"][a05]), np.median(drop), w[a05].min(), w[a05].max()))
    print("amplitude 0.025: median %.2f dB-Hz, lowest %.0f Hz (%.2f dB-Hz), weights %.4f .. %.4f, %d of 24 above the default gate %.1f Hz" %
          (np.median(info["cn0_dbhz"][a025]), lin[a025].min(), sqi.db(lin[a025].min()), w[a025].min(), w[a025].max(),
           int((lin[a025] >= sqi.DEFAULTS["cn0_min_lin"]).sum()), sqi.DEFAULTS["cn0_min_lin"]))
    print("absent: %d records, median %.0f Hz, largest %.0f Hz" % (absent.sum(), np.median(lin[absent]), lin[absent].max()))
    assert strong.sum() == 96 and a05.sum() == 24 and a025.sum() == 24 and absent.sum() == 48 and (info["flags"][~absent] == 0).all()
    assert abs(np.median(drop) - 12.04) <= 0.5
    assert (lin[absent] < 500.0).all()
    assert (lin[a025] >= 500.0).all()
    assert max(w[a05].max(), w[a025].max()) < w[strong].min()
    assert (w[absent] == 0.0).all()  # the default gate stands above the 500 Hz of the check


# ---- 5. wrong readings of the text must show ---------------------------------------------------------------------------------------
def test_wrong_readings_show(small):
    s8, u8 = small
    tasks, peaks = [(0, 2)], [(30.0, -30, 100, 0.0)]
    mean = (5.2, -6.8)
    kw = dict(signed=False, mean=mean)
    fine = refine_iq_ref.refine(u8, 81920, tasks, peaks, sqi.SPM, sqi.FC, sqi.FS, mix_hz=sqi.FC - sqi.IF_HZ, blocks=2, **kw)
    right = sqi.floors(u8, 81920, tasks, fine, sqi.SPM, **kw)[0][1]
    assert fine[0]["segments"] == 14 and right > 0

    class NoFactorTwo(sqi.Law):
        def floor_of_window(self, vi, vq, o, n):
            return self.energy(vi, vq, o, n)

    class WholeBlocks(sqi.Law):
        def window(self, block, segments, stride, spm, n_samples):
            return block * (stride // 2), 2 * 40000  # blocks * 40000 samples instead of segments * spm

    wrong = {"no factor 2": sqi.floors(u8, 81920, tasks, fine, sqi.SPM, law=NoFactorTwo(), **kw)[0][1],
             "blocks * 40000 samples": sqi.floors(u8, 81920, tasks, fine, sqi.SPM, law=WholeBlocks(), **kw)[0][1],
             "the mean left in": sqi.floors(u8, 81920, tasks, fine, sqi.SPM, signed=False, mean=None)[0][1],
             "the U8 offset forgotten": sqi.floors(u8, 81920, tasks, fine, sqi.SPM, signed=True, mean=mean)[0][1]}
    print("right floor %d; %s" % (right, wrong))
    assert all(v != right for v in wrong.values())
    assert wrong["no factor 2"] * 2 == right and wrong["blocks * 40000 samples"] > right and wrong["the mean left in"] > right


def test_records_that_are_not_of_the_capture(small):
    """step 1: unusable flags, segments <= 0, a block before or beyond the capture, a window that ends beyond it; an all-zero window"""
    s8, _ = small
    n = s8.size // 2
    rec = lambda flags, segments, prompt=10 ** 9: dict(flags=flags, segments=segments, prompt=prompt)
    fine = [rec(0, 7), rec(1, 7), rec(4, 7), rec(8, 7), rec(2, 7), rec(0, 0), rec(0, -3), rec(0, 7), rec(0, 7), rec(0, 2251), rec(0, 22), rec(0, 23)]
    tasks = [(0, 0)] * 7 + [(-1, 0), (4, 0), (0, 0), (0, 0), (0, 0)]
    got = sqi.floors(s8, 81920, tasks, fine, sqi.SPM, signed=True)
    print("record %s" % [r for r, _ in got])
    assert [r for r, _ in got] == [True, False, False, False, True, False, False, False, False, False, True, False]
    assert all(f == 0 for r, f in got if not r) and 22 * sqi.SPM <= n < 23 * sqi.SPM
    _, info = sqi.quality(s8, 81920, tasks, fine, sqi.SPM, sqi.FS, signed=True)
    assert all(info[k].tobytes() == np.int32(0).tobytes() + np.int32(sq.NO_RECORD).tobytes() + bytes(40) for k, (r, _) in enumerate(got) if not r)
    zero = np.zeros(2 * 3 * sqi.SPM, np.int8)
    fl, info = sqi.quality(zero, 81920, [(0, 0)], [rec(0, 3, 5)], sqi.SPM, sqi.FS, signed=True)
    assert fl.tolist() == [0] and info["flags"][0] == sq.NO_POWER and info["epochs"][0] == 3 and info["sig"][0] == 0 and info["weight"][0] == 0.0
