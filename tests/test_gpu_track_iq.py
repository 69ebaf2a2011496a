"""Tracking channels on an 8-bit IQ capture, on the GPU (gpsacq_track_iq8, track_iq_kernels.hip): sign mode against convert-then-
track, the multi-bit complex channels against their CPU model (tests/c/track_model_iq.c) and against the 1-bit kernel on a
degenerate capture, NAV subframes end to end at positive and negative residual IF (Python and the gps_track front end), the
sensitivity gained over sign mode, a ghost channel, the loop-setting and NCO-word arithmetic, and the capture generator."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

from track_helpers import nav_stream
from track_iq_helpers import model_dc, run_model_iq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1, CPS = 1575.42e6, 1.023e6
FC = {2.8e6: 0.7e6, 5.456e6: 4.092e6, 8.184e6: 2.046e6}


def _engine(fs):
    import gpsacq
    return gpsacq.Engine(FC[fs], fs, 5000.0, device=0)


def _hit(eng, dop_hz, code_phase):
    """the peak a search reports for a satellite of the generator's law, seen from a block that starts at sample 0"""
    import gpsacq
    pk = np.zeros(1, gpsacq.PEAK_DTYPE)
    pk["snr"] = 100.0
    pk["lo_shift"] = int(round(dop_hz * 40000 / eng.fs))
    pk["ca_shift"] = int(round(code_phase)) % eng.num_lags
    return pk[0]


def _nav_pm1(bits01):
    return np.where(np.asarray(bits01) > 0, -1, 1).astype(np.int8)


def _sats(rng, n, fs, lo=0.08, hi=0.2):
    prns = rng.choice(np.arange(1, 33), n, replace=False)
    return [(int(p), float(rng.uniform(lo, hi)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, fs / 1000)), float(rng.uniform(0, 1)))
            for p in prns]


def _add_dc(iq, signed, dc):
    """an integer offset on both arms (a front end's DC), kept inside the byte"""
    a = iq.astype(np.int16).reshape(-1, 2) + np.array(dc, np.int16)
    return (np.clip(a, -128, 127).astype(np.int8) if signed else np.clip(a, 0, 255).astype(np.uint8)).ravel()


def _same(a, b, ne_a, ne_b):
    """chans / prompt / records / n_epochs of two runs, byte for byte over the epochs run"""
    (cha, pa, ra), (chb, pb, rb) = a, b
    assert np.array_equal(ne_a, ne_b)
    assert cha.tobytes() == chb.tobytes()
    for c in range(len(ne_a)):
        n = int(ne_a[c])
        assert pa[c, :n].tobytes() == pb[c, :n].tobytes(), c
        assert ra[c, :n].tobytes() == rb[c, :n].tobytes(), c


# ---- sign mode: the reference's flow, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("fs,signed,remove_dc,if_hz", [(2.8e6, False, True, 80e3), (5.456e6, True, False, -600e3)])
def test_sign_mode_is_convert_then_track(fs, signed, remove_dc, if_hz):
    """uint8 with mixer and DC removal at 2.8 MHz (the rtl-sdr flow), int8 with the HackRF script's mixer at 5.456 MHz: chans,
    prompt, records equal gpsacq_iq8_to_bits + gpsacq_track, in one call and in three unequal windows; a window start off the
    byte grid is refused."""
    import gpsacq
    rng = np.random.default_rng(int(fs) + 1)
    sats = _sats(rng, 5, fs, 0.12, 0.2)
    nav = np.array([_nav_pm1(rng.integers(0, 2, 40)) for _ in sats])
    n = int(1.5 * fs) - 3  # a ragged last byte
    with _engine(fs) as eng:
        iq = eng.generate_iq8(n, sats, if_hz=if_hz, scale=20.0, signed=signed, seed=4, nav=nav)
        if remove_dc:
            iq = _add_dc(iq, signed, (6, -4))
        mix = eng.fc - if_hz
        mean = eng.iq8_mean(iq, signed=signed) if remove_dc else (0.0, 0.0)
        bits = eng.iq8_to_bits(iq, signed=signed, remove_dc=remove_dc, mix_hz=mix, fs=fs)
        inp = eng.iq8_input(signed=signed, remove_dc=remove_dc, mean=mean, mix_hz=mix, fs=fs, total_samples=n, multibit=0)
        p = eng.track_params()
        start = np.concatenate([eng.track_start_iq8(inp, s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        assert start.tobytes() == np.concatenate([eng.track_start(s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats]).tobytes()
        ref = start.copy()
        pr, rr, nr = eng.track(bits, ref, records=True, params=p)
        one = start.copy()
        po, ro, no = eng.track_iq8(iq, inp, one, records=True, params=p, max_epochs=pr.shape[1])
        assert nr.min() > 1400
        _same((ref, pr, rr), (one, po, ro), nr, no)
        # three unequal windows, each starting at the byte that holds the earliest channel's next_sample
        pieces, recs = start.copy(), [[] for _ in sats]
        for end in (n // 5, (3 * n) // 5, n):
            first = int(pieces["next_sample"].min()) // 8 * 8
            w = eng.iq8_input(signed=signed, remove_dc=remove_dc, mean=mean, mix_hz=mix, fs=fs, first_sample=first, total_samples=n, multibit=0)
            _, r, ne = eng.track_iq8(iq[2 * first:2 * end], w, pieces, first_sample=first, records=True, params=p)
            for c in range(len(sats)):
                recs[c].append(r[c, :ne[c]])
        assert pieces.tobytes() == ref.tobytes()
        for c in range(len(sats)):
            assert np.concatenate(recs[c]).tobytes() == rr[c, :nr[c]].tobytes()
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.track_iq8(iq[8:], inp, start.copy(), first_sample=4, params=p)
        assert ei.value.code == 1


# ---- multi-bit complex channels = the CPU model ---------------------------------------------------------------------------
@pytest.mark.parametrize("if_hz", [300e3, -250e3, 0.0])
@pytest.mark.parametrize("remove_dc", [False, True])
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("fs,n_sats,secs", [(2.8e6, 4, 1.5), (5.456e6, 8, 1.5), (8.184e6, 6, 1.5)])
def test_multibit_bit_exact_with_cpu_model(fs, n_sats, secs, signed, remove_dc, if_hz):
    import gpsacq
    rng = np.random.default_rng(int(fs) + 7 * signed + 3 * remove_dc + int(if_hz) % 1000)
    sats = _sats(rng, n_sats, fs)
    nav = np.array([_nav_pm1(rng.integers(0, 2, 50)) for _ in sats])
    n = int(secs * fs) - 5
    with _engine(fs) as eng:
        iq = eng.generate_iq8(n, sats, if_hz=if_hz, scale=float(rng.uniform(8, 30)), signed=signed, seed=11, nav=nav)
        if remove_dc:
            iq = _add_dc(iq, signed, (int(rng.integers(-9, 10)), int(rng.integers(-9, 10))))
        mean = eng.iq8_mean(iq, signed=signed) if remove_dc else (0.0, 0.0)
        inp = eng.iq8_input(signed=signed, remove_dc=remove_dc, mean=mean, mix_hz=eng.fc - if_hz, fs=fs, total_samples=n, multibit=1)
        p = eng.track_params_iq8(eng.iq8_rms(iq[:2 * 400000], inp))
        start = np.concatenate([eng.track_start_iq8(inp, s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        one = start.copy()
        prompt, rec, ne = eng.track_iq8(iq, inp, one, records=True, params=p)
        # pieces whose starts are not multiples of 8 samples
        pieces, recs = start.copy(), [[] for _ in sats]
        for end in (n // 5 + 1, (3 * n) // 5 + 2, n):
            first = max(0, int(pieces["next_sample"].min()) - 3)
            _, r, k = eng.track_iq8(iq[2 * first:2 * end], inp, pieces, first_sample=first, records=True, params=p)
            for c in range(n_sats):
                recs[c].append(r[c, :k[c]])
        # a max_epochs cut, then a resume
        cut = start.copy()
        _, ra, na = eng.track_iq8(iq, inp, cut, max_epochs=333, records=True, params=p)
        first = int(cut["next_sample"].min()) - 1
        _, rb, nb = eng.track_iq8(iq[2 * first:], inp, cut, first_sample=first, records=True, params=p)
    dc = model_dc(inp)
    mch = start.copy()
    mprompt, mrec, mne = run_model_iq(iq, 0, signed, dc, mch, p, prompt.shape[1])
    assert ne.min() > secs * 1000 - 5 or (one["status"] != 0).any()
    _same((one, prompt, rec), (mch, mprompt, mrec), ne, mne)
    assert (one["status"] == gpsacq.TRACK_OK).sum() >= n_sats - 1  # these are live channels, not noise
    assert pieces.tobytes() == one.tobytes() and cut.tobytes() == one.tobytes() and (na == 333).all()
    for c in range(n_sats):
        assert np.concatenate(recs[c]).tobytes() == rec[c, :ne[c]].tobytes(), c
        assert np.concatenate([ra[c, :na[c]], rb[c, :nb[c]]]).tobytes() == rec[c, :ne[c]].tobytes(), c


def test_degenerate_capture_equals_one_bit_kernel():
    """I = 1 - 2 bit, Q = 0 through the multi-bit kernel = gpsacq_track on the bits, byte for byte: the new kernel against the old
    one with no CPU model in between."""
    import gpsacq
    fs = 5.456e6
    rng = np.random.default_rng(66)
    sats = _sats(rng, 6, fs)
    nav = np.array([_nav_pm1(rng.integers(0, 2, 50)) for _ in sats])
    n_bytes = int(2.0 * fs) // 8
    with _engine(fs) as eng:
        bits = eng.generate(n_bytes, sats, seed=12, nav=nav)
        iq = np.zeros(16 * n_bytes, np.int8)
        iq[0::2] = 1 - 2 * np.unpackbits(bits, bitorder="little").astype(np.int8)
        p = eng.track_params()
        start = np.concatenate([eng.track_start(s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        a = start.copy()
        pa, ra, na = eng.track(bits, a, records=True, params=p)
        inp = eng.iq8_input(signed=True, remove_dc=False, multibit=1)
        b = start.copy()
        pb, rb, nb = eng.track_iq8(iq, inp, b, records=True, params=p, max_epochs=pa.shape[1])
    assert na.min() > 1990
    _same((a, pa, ra), (b, pb, rb), na, nb)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _e2e_capture(eng, fs, if_hz, secs, seed, signed):
    rng = np.random.default_rng(seed)
    prns = [2, 7, 13, 19, 24, 31]
    sats, nav01, metas = [], [], []
    for k, prn in enumerate(prns):
        sats.append((prn, float(rng.uniform(0.1, 0.2)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, fs / 1000)), float(rng.uniform(0, 1))))
        b, meta = nav_stream(1000 * (k + 1), 4, seed=k)
        nav01.append(b)
        metas.append(meta)
    iq = eng.generate_iq8(int(secs * fs), sats, if_hz=if_hz, scale=16.0, signed=signed, seed=seed + 1, nav=np.array([_nav_pm1(b) for b in nav01]))
    return prns, sats, nav01, metas, iq


@pytest.mark.parametrize("if_hz,mode", [(400e3, 1), (-300e3, 2)])
def test_nav_end_to_end_multibit(if_hz, mode):
    """20 s at 5.456 MHz, six satellites with parity-valid subframes, at a positive residual IF searched as a real IF (mixer fc -
    if) and at a negative one searched as complex baseband (mixer -if): channels from the hits with the settings of the measured
    RMS, tracked multi-bit: all OK, every whole subframe decodes with its (id, tow), no parity failure after the first."""
    import gpsacq
    fs = 5.456e6
    with _engine(fs) as eng:
        prns, sats, nav01, metas, iq = _e2e_capture(eng, fs, if_hz, 20.0, 20, signed=(mode == 2))
        signed = mode == 2
        mean = eng.iq8_mean(iq, signed=signed)
        mix = eng.fc - if_hz if mode == 1 else -if_hz
        inp = eng.iq8_input(signed=signed, remove_dc=True, mean=mean, mix_hz=mix, fs=fs, total_samples=iq.size // 2, multibit=mode)
        _, pk = eng.search_iq8(iq[:16 * gpsacq.BLOCK_BYTES * 8], inp, tasks=[(0, p - 1) for p in prns], want_cells=False)
        assert (pk["snr"] > 25).all()
        p = eng.track_params_iq8(eng.iq8_rms(iq[:2 * 1000000], inp))
        ch = np.concatenate([eng.track_start_iq8(inp, prn, pk[i], 0, params=p) for i, prn in enumerate(prns)])
        prompt, rec, ne = eng.track_iq8(iq, inp, ch, records=True, params=p)
    assert (ch["status"] == gpsacq.TRACK_OK).all()
    for c, prn in enumerate(prns):
        n = int(ne[c])
        assert n > 19900
        # the carrier the channel ends on is the satellite's frequency in the raw capture
        f = rec[c, n - 500:n]["lo_rate"].astype(np.int32).astype(np.float64).mean() / 2 ** 32 * fs
        assert abs(f - (if_hz + sats[c][2])) < 20.0, (prn, f)
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=1000)
        assert e0 >= 1000
        sf, _ = gpsacq.nav_subframes(bits)
        assert len(sf) >= 1
        first = sf["bit_offset"][0]
        sf, nfail = gpsacq.nav_subframes(bits[int(first):])
        assert nfail == 0
        got = [(int(a), int(b)) for a, b in zip(sf["id"], sf["tow"])]
        assert len(got) == (bits.size - int(first)) // 300 and set(got) <= set(metas[c]), (prn, got)


@pytest.mark.parametrize("env,if_hz", [({"GPSACQ_IQ_MULTIBIT": "1"}, 200e3), ({"GPSACQ_IQ_COMPLEX": "1"}, -150e3), ({}, 200e3)])
def test_gps_track_cli_iq8(tmp_path, env, if_hz):
    """the gps_track front end on an rtl-like uint8 file, with the environment gps_test honours: multi-bit real IF, complex
    baseband at a negative residual IF, and sign mode"""
    fs = 2.8e6
    fc = FC[fs]
    prns = [4, 11, 26]
    sats = [(4, 0.18, 1500.0, 700.0, 0.0), (11, 0.16, -2000.0, 2500.0, 0.3), (26, 0.2, 300.0, 1100.0, 0.6)]
    navs = [nav_stream(777 + 100 * k, 3, seed=k) for k in range(3)]
    with _engine(fs) as eng:
        iq = eng.generate_iq8(int(20 * fs), sats, if_hz=if_hz, scale=16.0, signed=False, seed=2, nav=np.array([_nav_pm1(b) for b, _ in navs]))
    path = tmp_path / "cap_iq.bin"
    iq.tofile(path)
    mix = -if_hz if "GPSACQ_IQ_COMPLEX" in env else fc - if_hz
    full = dict(os.environ, GPSACQ_INPUT="iq_u8", GPSACQ_MIX_HZ=repr(mix), **env)
    exe = os.path.join(ROOT, "gnss-gps-sdr_amd", "bin", "gps_track")
    out = subprocess.run([exe, str(path), str(fc), str(fs)], capture_output=True, text=True, timeout=300, env=full)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    chans = {int(l.split()[3]): l.split() for l in lines if l.startswith("chan ")}
    assert set(prns) <= set(chans), out.stdout
    for k, prn in enumerate(prns):
        assert chans[prn][5] == "ok" and abs(float(chans[prn][9]) - sats[k][2]) < 50.0, chans[prn]  # well inside one 70-Hz Doppler bin
        sub = [l.split() for l in lines if l.startswith("subframe ") and int(l.split()[2]) == prn]
        assert len(sub) >= 1, out.stdout
        for s in sub:
            assert (int(s[4]), int(s[6])) in navs[k][1], s


def test_multibit_buys_sensitivity():
    """One capture tracked in sign mode and in multi-bit mode: the post-correlation SNR of the prompt arm, mean(|IP|)^2 / var(|IP|)
    over the same locked epochs, is higher multi-bit for every satellite (the hard limiter's 2 / pi, and the real part folding the
    image band's noise onto the signal).  Only ratio > 1 is asserted; the ratios are printed (DESIGN.md section 8 records them)."""
    import gpsacq
    fs, if_hz = 2.8e6, 120e3
    sats = [(3, 0.10, 1234.0, 1000.3, 0.2), (8, 0.12, -3100.0, 2000.0, 0.7), (15, 0.15, 430.0, 17.0, 0.0), (21, 0.18, 3900.0, 2400.0, 0.4),
            (28, 0.2, -800.0, 555.0, 0.9)]
    rng = np.random.default_rng(5)
    nav = np.array([_nav_pm1(rng.integers(0, 2, 60)) for _ in sats])
    n = int(8 * fs)
    with _engine(fs) as eng:
        iq = eng.generate_iq8(n, sats, if_hz=if_hz, scale=16.0, signed=False, seed=31, nav=nav)
        mean = eng.iq8_mean(iq)
        kw = dict(signed=False, remove_dc=True, mean=mean, mix_hz=eng.fc - if_hz, fs=fs, total_samples=n)
        snr = {}
        for mode in (0, 1):
            inp = eng.iq8_input(multibit=mode, **kw)
            p = eng.track_params_iq8(eng.iq8_rms(iq[:2 * 1000000], inp)) if mode else eng.track_params()
            ch = np.concatenate([eng.track_start_iq8(inp, s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
            prompt, _, ne = eng.track_iq8(iq, inp, ch, params=p)
            assert (ch["status"] == gpsacq.TRACK_OK).all() and ne.min() > 7900, mode
            a = np.abs(prompt[:, 2000:7900, 0].astype(np.float64))
            snr[mode] = a.mean(axis=1) ** 2 / a.var(axis=1)
    ratio = snr[1] / snr[0]
    print("post-correlation SNR sign", np.round(snr[0], 2), "multi-bit", np.round(snr[1], 2), "ratio", np.round(ratio, 3))
    assert (ratio > 1).all(), ratio


def test_absent_prn_is_lost_and_harmless_multibit():
    import gpsacq
    fs, if_hz = 5.456e6, -200e3
    sats = [(5, 0.15, 800.0, 300.0, 0.0), (9, 0.15, -2500.0, 3000.0, 0.5)]
    n = int(3 * fs)
    with _engine(fs) as eng:
        iq = eng.generate_iq8(n, sats, if_hz=if_hz, scale=16.0, signed=True, seed=8)
        inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=eng.fc - if_hz, fs=fs, multibit=1)
        p = eng.track_params_iq8(eng.iq8_rms(iq[:2 * 1000000], inp))
        good = np.concatenate([eng.track_start_iq8(inp, s[0], _hit(eng, s[2], s[3]), 0, params=p) for s in sats])
        ghost = eng.track_start_iq8(inp, 27, _hit(eng, 2000.0, 1234.0), 0, params=p)  # not in the capture
        both = np.concatenate([good[:1], ghost, good[1:]])
        t0 = time.time()
        pb, rb, nb = eng.track_iq8(iq, inp, both, records=True, params=p)
        assert time.time() - t0 < 30
        pa, ra, na = eng.track_iq8(iq, inp, good, records=True, params=p)
    for i, j in ((0, 0), (2, 1)):
        assert nb[i] == na[j] and np.array_equal(rb[i, :nb[i]], ra[j, :na[j]])
    assert (good["status"] == gpsacq.TRACK_OK).all() and na.min() > 2990
    k = int(nb[1])
    locked_power = np.mean(pb[0, k // 2:nb[0], 0].astype(float) ** 2)
    ghost_power = np.mean(pb[1, k // 2:k, 0].astype(float) ** 2) if k > 10 else 0.0
    assert both["status"][1] == gpsacq.TRACK_LOST or ghost_power < locked_power / 20


# ---- host arithmetic that needs an engine ----------------------------------------------------------------------------------
def test_default_params_iq8_and_nco_words():
    import gpsacq
    fs = 2.8e6
    with _engine(fs) as eng:
        base = eng.track_params()
        for rms in (0.9, 1.0, 11.3, 16.0, 23.0, 90.5):
            g = int(round(math.log2(4 * rms * rms)))  # GPSACQ_TRACK_IQ8_GAIN = 4
            p = eng.track_params_iq8(rms)
            for f in ("lo_ki", "lo_kp", "ca_ki", "ca_kp", "fll_k"):
                assert getattr(p, f) == getattr(base, f) - g, (rms, f)
            assert p.agc_lo == math.floor(base.agc_lo * 2.0 ** g) and p.agc_hi == math.floor(base.agc_hi * 2.0 ** g)
            for f in ("fll_epochs", "aid_epoch", "agc_period", "lo_window", "ca_window", "min_epoch", "max_epoch"):
                assert getattr(p, f) == getattr(base, f)
        # a tiny RMS raises the shifts only as far as 62; a huge one cannot keep them >= 0
        p = eng.track_params_iq8(1e-9)
        assert max(p.lo_ki, p.lo_kp, p.ca_ki, p.ca_kp, p.fll_k) == 62
        for bad in (1e6, 0.0, -1.0, float("nan")):
            with pytest.raises(gpsacq.GpsAcqError) as ei:
                eng.track_params_iq8(bad)
            assert ei.value.code == 3
        # carrier words of multi-bit channels: llround(f / fs 2^32) as two's complement, f = lo_dop - mix_hz + fc (complex: no fc)
        pk = _hit(eng, 2100.0, 1000.0)
        lo_dop = pk["lo_shift"] * fs / 40000
        one_bit = eng.track_start(7, pk, 4096)
        for mode, mix in ((1, eng.fc - 300e3), (1, eng.fc + 250e3), (1, eng.fc), (2, -300e3), (2, 250e3), (1, eng.fc + lo_dop)):
            inp = eng.iq8_input(signed=True, remove_dc=False, mix_hz=mix, fs=fs, multibit=mode)
            ch = eng.track_start_iq8(inp, 7, pk, 4096, params=base)
            f = lo_dop - mix + (eng.fc if mode == 1 else 0.0)
            word = int(np.rint(f / fs * 2 ** 32)) & 0xFFFFFFFF
            assert int(ch["lo_rate"][0]) == word and int(ch["lo_int"][0]) & (2 ** 64 - 1) == word << 32 and ch["lo_nom"][0] == ch["lo_int"][0]
            assert int(ch["lo_phase"][0]) == (int(ch["next_sample"][0]) * word) & 0xFFFFFFFF
            for k in ("prn", "next_sample", "ca_pos", "ca_rate", "ca_int", "ca_nom", "fll_left", "status"):
                assert ch[k][0] == one_bit[k][0], k
        with pytest.raises(gpsacq.GpsAcqError):
            eng.track_start_iq8(eng.iq8_input(signed=True, mix_hz=eng.fc + 1.5e6, multibit=1), 7, pk, 0, params=base)  # |f| >= fs / 2
        with pytest.raises(ValueError):
            eng.track_iq8(np.zeros(200000, np.int8), eng.iq8_input(signed=True, multibit=1), one_bit.copy())  # multi-bit needs params


def test_generate_iq8_law():
    """any window of the stream is that window; uint8 = int8 + 128; level, clamp and the satellites' presence"""
    fs = 5.456e6
    sats = [(1, 0.2, 1000.0, 10.0, 0.1), (2, 0.1, -700.0, 2000.5, 0.4)]
    with _engine(fs) as eng:
        whole = eng.generate_iq8(300000, sats, if_hz=-123e3, scale=16.0, signed=True, seed=3, nav=np.ones((2, 5), np.int8))
        part = eng.generate_iq8(100001, sats, if_hz=-123e3, scale=16.0, signed=True, seed=3, first_sample=77777, nav=np.ones((2, 5), np.int8))
        plain = eng.generate_iq8(300000, sats, if_hz=-123e3, scale=16.0, signed=True, seed=3)
        u8 = eng.generate_iq8(300000, sats, if_hz=-123e3, scale=16.0, signed=False, seed=3)
        hot = eng.generate_iq8(100000, sats, if_hz=0.0, scale=100.0, signed=True, seed=3)
        quiet = eng.generate_iq8(40000, [(1, 1.0, 0.0, 0.0, 0.0)], if_hz=fs / 8, scale=100.0, signed=True, noise_sigma=0.0, seed=1)
    assert np.array_equal(whole[2 * 77777:2 * (77777 + 100001)], part) and np.array_equal(whole, plain)
    assert np.array_equal(u8.astype(np.int16) - 128, whole.astype(np.int16))
    a = whole.astype(np.float64)
    assert abs(a[0::2].std() - 16.0 * math.sqrt(1 + 0.025)) < 0.2 and abs(a[1::2].std() - 16.0 * math.sqrt(1 + 0.025)) < 0.2
    assert abs(np.corrcoef(a[0::2], a[1::2])[0, 1]) < 0.01 and abs(a.mean()) < 0.1
    assert hot.max() == 127 and hot.min() == -127
    # noise-free: chip * exp(2 pi i m / 8) * 100, a positive frequency (I leads Q by a quarter turn)
    z = quiet[0::2].astype(np.float64) + 1j * quiet[1::2]
    from track_iq_helpers import chips_pm1
    q = np.floor(np.arange(40000) * CPS / fs).astype(np.int64) % 1023
    want = 100.0 * chips_pm1(1)[q] * np.exp(2j * np.pi * np.arange(40000) / 8)
    assert np.abs(z - want).max() < 1.0
