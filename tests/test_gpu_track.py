"""Tracking channels on the GPU (gpsacq_track, track_kernels.hip): the reference's own signal file, bit-exactness against the
CPU model of include/gpsacq.h (tests/c/track_model.c), tracking in pieces, NAV subframes end to end, the code-aided carrier
reset, loss, the generator with navigation data, and the gps_track front end."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

from track_helpers import nav_stream, run_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1, CPS = 1575.42e6, 1.023e6


def _engine(fc, fs):
    import gpsacq
    return gpsacq.Engine(fc, fs, 5000.0, device=0)


def _hit(eng, dop_hz, code_phase):
    """the peak a search reports for a satellite of gpsacq_generate's law, seen from a block that starts at sample 0"""
    import gpsacq
    pk = np.zeros(1, gpsacq.PEAK_DTYPE)
    pk["snr"] = 100.0
    pk["lo_shift"] = int(round(dop_hz * 40000 / eng.fs))
    pk["ca_shift"] = int(round(code_phase)) % eng.num_lags
    return pk[0]


def _nav_pm1(bits01):
    return np.where(np.asarray(bits01) > 0, -1, 1).astype(np.int8)


def _truth_bits(rec, cp, dop, fs, nav01):
    """the navigation bit each epoch was sent with (0/1), by the generator's law at the epoch's middle"""
    mid = rec["sample"].astype(np.float64) + fs / 2000
    q = np.floor((mid + cp) * CPS * (1 + dop / L1) / fs).astype(np.int64)
    return np.asarray(nav01)[(q // 20460) % len(nav01)]


def test_reference_signal_bits(golden_dir):
    """gps_sig_tmp.bin: search block 0 for PRN 8, start the channel from that hit (FLL off: the hit's Doppler bin 0 is exact here),
    track the whole file; the 100 bits of gps_sig_tmp_databits.json come back.  The file is noise-free, so its correlation
    amplitude is ~12x a live 1-bit capture's; both loops' gains (which scale with its square) are lowered by 2^7."""
    import gpsacq
    buf = np.fromfile(os.path.join(golden_dir, "gps_sig_tmp.bin"), np.uint8)
    want = np.array(json.load(open(os.path.join(golden_dir, "gps_sig_tmp_databits.json")))["bits_pm1"])
    with _engine(2.046e6, 8.184e6) as eng:
        _, pk = eng.search(buf[:gpsacq.BLOCK_BYTES], tasks=[(0, 7)], want_cells=False)
        assert pk["lo_shift"][0] == 0 and pk["snr"][0] > 100
        p = eng.track_params(fll_epochs=0)
        for f in ("lo_ki", "lo_kp", "ca_ki", "ca_kp"):
            setattr(p, f, getattr(p, f) - 7)
        ch = eng.track_start(8, pk[0], 0, params=p)
        prompt, rec, ne = eng.track(buf, ch, records=True, params=p)
    n = int(ne[0])
    assert ch["status"][0] == gpsacq.TRACK_OK and n >= 1995
    bits, e0 = gpsacq.nav_bits(prompt[0, :n, 0], first_epoch=0)
    assert e0 % 20 == 0  # the channel's epoch 0 is the file's code period 0 (the hit's pause lands on chip 0)
    got = 1 - 2 * bits.astype(int)
    truth = want[e0 // 20: e0 // 20 + got.size]
    assert got.size >= 97
    assert np.array_equal(got, truth) or np.array_equal(got, -truth)
    # after lock the carrier stays on fs/4
    dev_hz = (rec[0, 200:n]["lo_rate"].astype(np.int64) - (1 << 30)) / 2.0 ** 32 * 8.184e6
    assert np.abs(dev_hz).max() < 25.0


@pytest.mark.parametrize("fs,fc,n_sats,secs", [(2.8e6, 0.7e6, 4, 2.0), (5.456e6, 4.092e6, 8, 2.0), (8.184e6, 2.046e6, 6, 1.5)])
def test_bit_exact_with_cpu_model(fs, fc, n_sats, secs):
    import gpsacq
    rng = np.random.default_rng(int(fs))
    prns = rng.choice(np.arange(1, 33), n_sats, replace=False)
    sats, nav = [], []
    for prn in prns:
        sats.append((int(prn), float(rng.uniform(0.08, 0.2)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, fs / 1000)),
                     float(rng.uniform(0, 1))))
        nav.append(_nav_pm1(rng.integers(0, 2, 50)))
    n_bytes = int(secs * fs) // 8
    with _engine(fc, fs) as eng:
        buf = eng.generate(n_bytes, sats, noise_sigma=1.0, seed=11, nav=np.array(nav))
        p = eng.track_params()
        ch = np.concatenate([eng.track_start(s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        ch0 = ch.copy()
        prompt, rec, ne = eng.track(buf, ch, records=True, params=p)
    mch = ch0.copy()
    mprompt, mrec, mne = run_model(buf, 0, mch, p, prompt.shape[1])
    assert np.array_equal(ne, mne)
    assert ne.min() > secs * 1000 - 5 or (ch["status"] != 0).any()
    for c in range(len(sats)):
        n = int(ne[c])
        assert np.array_equal(rec[c, :n], mrec[c, :n]), c
        assert np.array_equal(prompt[c, :n], mprompt[c, :n]), c
    assert ch.tobytes() == mch.tobytes()


def test_pieces_equal_one_call():
    import gpsacq
    fs, fc = 5.456e6, 4.092e6
    sats = [(3, 0.15, 1234.0, 1000.5, 0.2), (17, 0.1, -3000.0, 4000.0, 0.7), (22, 0.12, 400.0, 17.0, 0.0)]
    nav = np.array([_nav_pm1(np.random.default_rng(k).integers(0, 2, 30)) for k in range(3)])
    n_bytes = int(1.2 * fs) // 8
    with _engine(fc, fs) as eng:
        buf = eng.generate(n_bytes, sats, seed=5, nav=nav)
        p = eng.track_params()
        start = np.concatenate([eng.track_start(s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        one = start.copy()
        prompt1, rec1, ne1 = eng.track(buf, one, records=True, params=p)
        # three unequal windows, each starting at the byte that holds the earliest channel's next_sample
        pieces = start.copy()
        ends = [n_bytes // 5, (3 * n_bytes) // 5, n_bytes]
        recs = [[] for _ in sats]
        for end in ends:
            first = int(pieces["next_sample"].min()) // 8 * 8
            _, r, ne = eng.track(buf[first // 8:end], pieces, first_sample=first, records=True, params=p)
            for c in range(len(sats)):
                recs[c].append(r[c, :ne[c]])
        assert pieces.tobytes() == one.tobytes()
        for c in range(len(sats)):
            assert np.array_equal(np.concatenate(recs[c]), rec1[c, :ne1[c]])
        # a max_epochs cut, then a resume
        cut = start.copy()
        _, ra, na = eng.track(buf, cut, max_epochs=333, records=True, params=p)
        assert (na == 333).all()
        first = int(cut["next_sample"].min()) // 8 * 8
        _, rb, nb = eng.track(buf[first // 8:], cut, first_sample=first, records=True, params=p)
        assert cut.tobytes() == one.tobytes()
        for c in range(len(sats)):
            assert np.array_equal(np.concatenate([ra[c, :na[c]], rb[c, :nb[c]]]), rec1[c, :ne1[c]])
        # a window that starts after a channel's next_sample is refused
        with pytest.raises(gpsacq.GpsAcqError):
            eng.track(buf[8:], cut, first_sample=int(cut["next_sample"].max()) + 8000, params=p)


def test_nav_end_to_end():
    """20 s at 5.456 MHz / 4.092 MHz, six satellites with parity-valid subframes (their own TOW), searched from block 0, tracked
    from those hits: every whole subframe decodes with its ID and TOW, no parity failure."""
    import gpsacq
    fs, fc = 5.456e6, 4.092e6
    rng = np.random.default_rng(20)
    prns = [2, 7, 13, 19, 24, 31]
    sats, nav01, metas = [], [], []
    for k, prn in enumerate(prns):
        sats.append((prn, float(rng.uniform(0.1, 0.2)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, 5456)), float(rng.uniform(0, 1))))
        b, meta = nav_stream(1000 * (k + 1), 4, seed=k)
        nav01.append(b)
        metas.append(meta)
    n_bytes = int(20 * fs) // 8
    with _engine(fc, fs) as eng:
        buf = eng.generate(n_bytes, sats, seed=21, nav=np.array([_nav_pm1(b) for b in nav01]))
        _, pk = eng.search(buf[:gpsacq.BLOCK_BYTES * 8], tasks=[(0, p - 1) for p in prns], want_cells=False)
        assert (pk["snr"] > 25).all()
        ch = np.concatenate([eng.track_start(prn, pk[i], 0) for i, prn in enumerate(prns)])
        prompt, rec, ne = eng.track(buf, ch, records=True)
    assert (ch["status"] == gpsacq.TRACK_OK).all()
    for c, prn in enumerate(prns):
        n = int(ne[c])
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=1000)
        assert e0 >= 1000
        truth = _truth_bits(rec[c, e0:e0 + 20 * bits.size:20], sats[c][3], sats[c][2], fs, nav01[c])
        assert np.array_equal(bits, truth) or np.array_equal(bits, 1 - truth), prn
        sf, _ = gpsacq.nav_subframes(bits)
        # before the first preamble the scan meets payload bits that look like one and fail parity (as CHANNEL::ParityCheck()
        # does); from the first subframe on, every word passes
        assert len(sf) >= 1
        first = sf["bit_offset"][0]
        sf, nfail = gpsacq.nav_subframes(bits[int(first):])
        assert nfail == 0
        # from the first subframe on every whole one decodes (the scan of CHANNEL::ParityCheck() may step over the first real
        # preamble when a look-alike just before it fails parity); the 1200-bit stream repeats, so every (id, tow) is one of the four
        got = [(int(a), int(b)) for a, b in zip(sf["id"], sf["tow"])]
        assert len(got) == (bits.size - int(first)) // 300 and set(got) <= set(metas[c]), (prn, got)


def test_reference_aid():
    """An 8-s capture whose carrier sits half a Doppler bin off the hit's bin centre, FLL off, the code-aided carrier reset at
    epoch 5000 (the reference's 5-s wait): afterwards the carrier is on frequency and every bit after epoch 5500 is right."""
    import gpsacq
    fs, fc = 5.456e6, 4.092e6
    binhz = fs / 40000
    dop, cp = -10 * binhz + 0.5 * binhz, 2222.0
    nav01 = np.random.default_rng(4).integers(0, 2, 400).astype(np.uint8)
    with _engine(fc, fs) as eng:
        buf = eng.generate(int(8 * fs) // 8, [(12, 0.2, dop, cp, 0.1)], seed=3, nav=_nav_pm1(nav01)[None, :])
        p = eng.track_params(fll_epochs=0, aid_epoch=5000)
        pk = _hit(eng, -10 * binhz, cp)
        ch = eng.track_start(12, pk, 0, params=p)
        prompt, rec, ne = eng.track(buf, ch, records=True, params=p)
    n = int(ne[0])
    assert ch["status"][0] == gpsacq.TRACK_OK and n > 7900
    lo_hz = rec[0, 5500:n]["lo_rate"].astype(np.float64) / 2 ** 32 * fs - fc
    assert np.abs(lo_hz - dop).max() < 40.0
    bits, e0 = gpsacq.nav_bits(prompt[0, 5500:n, 0], first_epoch=5500)
    truth = _truth_bits(rec[0, e0:e0 + 20 * bits.size:20], cp, dop, fs, nav01)
    assert bits.size > 110
    assert np.array_equal(bits, truth) or np.array_equal(bits, 1 - truth)


def test_absent_prn_is_lost_and_harmless():
    import gpsacq
    fs, fc = 5.456e6, 4.092e6
    sats = [(5, 0.15, 800.0, 300.0, 0.0), (9, 0.15, -2500.0, 3000.0, 0.5)]
    with _engine(fc, fs) as eng:
        buf = eng.generate(int(3 * fs) // 8, sats, seed=8)
        p = eng.track_params()
        good = np.concatenate([eng.track_start(s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        ghost = eng.track_start(27, _hit(eng, 2000.0, 1234.0), 0, params=p)  # not in the capture
        both = np.concatenate([good[:1], ghost, good[1:]])
        t0 = time.time()
        pb, rb, nb = eng.track(buf, both, records=True, params=p)
        assert time.time() - t0 < 30
        pa, ra, na = eng.track(buf, good, records=True, params=p)
    for i, j in ((0, 0), (2, 1)):
        assert nb[i] == na[j] and np.array_equal(rb[i, :nb[i]], ra[j, :na[j]])
    n = int(nb[1])
    locked_power = np.mean(pb[0, n // 2:nb[0], 0].astype(float) ** 2)
    ghost_power = np.mean(pb[1, n // 2:n, 0].astype(float) ** 2) if n > 10 else 0.0
    assert both["status"][1] == gpsacq.TRACK_LOST or ghost_power < locked_power / 20


def test_generator_nav_null_and_ones():
    fs, fc = 5.456e6, 4.092e6
    sats = [(1, 0.2, 1000.0, 10.0, 0.1), (2, 0.1, -700.0, 2000.5, 0.4)]
    with _engine(fc, fs) as eng:
        plain = eng.generate(100000, sats, seed=3, first_sample=8 * 4096)
        ones = eng.generate(100000, sats, seed=3, first_sample=8 * 4096, nav=np.ones((2, 7), np.int8))
        lib = eng._lib
        import ctypes
        out = np.zeros(100000, np.uint8)
        rc = lib.gpsacq_generate_nav_range(eng._h, out.ctypes.data_as(ctypes.c_void_p), 100000, 8 * 4096, eng._sats(sats), 2, None, 0,
                                           ctypes.c_float(1.0), 3)
        assert rc == 0
        flipped = eng.generate(100000, sats, seed=3, first_sample=8 * 4096, nav=-np.ones((2, 7), np.int8))
    assert np.array_equal(plain, ones) and np.array_equal(plain, out)
    assert not np.array_equal(plain, flipped)


def test_gps_track_cli(tmp_path):
    fs, fc = 5.456e6, 4.092e6
    prns = [4, 11, 26]
    sats = [(4, 0.18, 1500.0, 700.0, 0.0), (11, 0.16, -2000.0, 2500.0, 0.3), (26, 0.2, 300.0, 4100.0, 0.6)]
    navs = [nav_stream(777 + 100 * k, 3, seed=k) for k in range(3)]
    with _engine(fc, fs) as eng:
        buf = eng.generate(int(20 * fs) // 8, sats, seed=2, nav=np.array([_nav_pm1(b) for b, _ in navs]))
    path = tmp_path / "cap.bin"
    buf.tofile(path)
    exe = os.path.join(ROOT, "gnss-gps-sdr_amd", "bin", "gps_track")
    out = subprocess.run([exe, str(path), str(fc), str(fs)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    chans = [l for l in lines if l.startswith("chan ")]
    assert set(prns) <= {int(l.split()[3]) for l in chans}, out.stdout  # (a noise hit above the threshold may add a channel)
    for k, prn in enumerate(prns):
        sub = [l.split() for l in lines if l.startswith("subframe ") and int(l.split()[2]) == prn]
        assert len(sub) >= 1, out.stdout
        for s in sub:
            assert (int(s[4]), int(s[6])) in navs[k][1], s
