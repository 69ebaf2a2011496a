"""Helpers of the 8-bit IQ tracking tests: the CPU model of a multi-bit complex channel (tests/c/track_model_iq.c, compiled with
gcc on first use), a numpy restatement of its six sums, host-side makers of small IQ captures and channel states (the CPU
tests have no engine), gpsacq_track_default_params_iq8 restated from the header, and sweep_iq: the scenarios of
test_track_ref.sweep on multi-bit complex channels, under the independent reference of tests/track_ref.py."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

from track_helpers import ROOT, chip_words

FULL = 1023 << 32
L1, CPS = 1575.42e6, 1.023e6
_model = None


def model_iq_lib():
    global _model
    if _model is None:
        out = os.path.join(tempfile.mkdtemp(prefix="track_model_iq_"), "libtrack_model_iq.so")
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "track_model_iq.c"), "-o", out])
        lib = ctypes.CDLL(out)
        vp = ctypes.c_void_p
        lib.track_model_iq.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int]
        lib.track_model_iq.restype = ctypes.c_int
        _model = lib
    return _model


def model_dc(inp):
    """the integers the model subtracts for a gpsacq_iq8_input: nearbyint(mean) when the mean is removed"""
    if not inp.remove_dc:
        return 0, 0
    return int(np.rint(inp.mean_i)), int(np.rint(inp.mean_q))


def run_model_iq(iq, first_sample, signed, dc, chans, params, max_epochs):
    """The CPU model over a window of interleaved I,Q bytes: chans (TRACK_CHAN_DTYPE) updated in place; returns (prompt, records,
    n_epochs) shaped like Engine.track_iq8(..., records=True)."""
    import gpsacq
    lib = model_iq_lib()
    buf = np.ascontiguousarray(np.asarray(iq).view(np.uint8).ravel())
    n = chans.size
    prompt = np.zeros((n, max_epochs, 2), np.int32)
    rec = np.zeros((n, max_epochs), gpsacq.TRACK_RECORD_DTYPE)
    ne = np.zeros(n, np.int32)
    for c in range(n):
        ch = chans[c:c + 1].copy()
        w = chip_words(int(ch["prn"][0]))
        ne[c] = lib.track_model_iq(buf.ctypes.data, buf.size // 2, int(first_sample), 1 if signed else 0, int(dc[0]), int(dc[1]), ch.ctypes.data,
                                   ctypes.addressof(params), w.ctypes.data, prompt[c].ctypes.data, rec[c].ctypes.data, int(max_epochs))
        chans[c] = ch[0]
    return prompt, rec, ne


def chips_pm1(prn):
    """the 1023 chips of PRN prn as +1 / -1 (h = 1 - 2 chip)"""
    w = chip_words(prn)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:1023]
    return 1 - 2 * bits.astype(np.int64)


def numpy_epoch_sums(iq, first_sample, signed, dc, ch, prn):
    """The six sums of the epoch that starts at ch's state, straight from the header's formulas with numpy integer arrays
    (vectorised over the epoch's samples; a restatement independent of the C model's loop).  Returns (n, [IE, QE, IP, QP, IL, QL])."""
    lo_phase, lo_rate = int(ch["lo_phase"]), int(ch["lo_rate"])
    ca_pos, ca_rate, s = int(ch["ca_pos"]), int(ch["ca_rate"]), int(ch["next_sample"])
    n = -((ca_pos - FULL) // ca_rate)  # ceil((FULL - ca_pos) / ca_rate)
    raw = np.asarray(iq).view(np.uint8).ravel()[2 * (s - first_sample):2 * (s - first_sample + n)]
    a = raw.view(np.int8).astype(np.int64) if signed else raw.astype(np.int64) - 128
    vi, vq = a[0::2] - dc[0], a[1::2] - dc[1]
    j = np.arange(n, dtype=np.uint64)
    ph = (np.uint64(lo_phase) + j * np.uint64(lo_rate)) & np.uint64(0xFFFFFFFF)
    b31, b30 = (ph >> np.uint64(31)).astype(np.int64) & 1, (ph >> np.uint64(30)).astype(np.int64) & 1
    C, S = 1 - 2 * (b31 ^ b30), 1 - 2 * (1 - b31)
    P = np.uint64(ca_pos) + j * np.uint64(ca_rate)
    h = chips_pm1(prn)
    out = []
    for X in ((P + np.uint64(1 << 31)) % np.uint64(FULL), P, (P + np.uint64(FULL - (1 << 31))) % np.uint64(FULL)):
        hx = h[(X >> np.uint64(32)).astype(np.int64)]
        out += [int(np.sum(hx * (vi * C - vq * S))), int(np.sum(hx * (vi * S + vq * C)))]
    return n, out


def host_chan(prn, fs, f_carrier, doppler, code_phase, fll_epochs, first=0):
    """A channel state as gpsacq_track_start_iq8 builds it in multi-bit mode, restated on the host (the CPU tests have no engine):
    carrier word llround(f / fs 2^32) as two's complement, code from the code phase in samples at sample `first`."""
    import gpsacq
    ch = np.zeros(1, gpsacq.TRACK_CHAN_DTYPE)
    ca_rate = int((CPS + doppler / L1 * CPS) / fs * 2 ** 32)
    word = int(np.rint(f_carrier / fs * 2 ** 32)) & 0xFFFFFFFF
    pos = (int(round(code_phase)) * ca_rate) % FULL
    n0 = -((pos - FULL) // ca_rate)
    ch["prn"], ch["status"] = prn, 0
    ch["lo_rate"], ch["ca_rate"] = word, ca_rate
    ch["lo_int"] = np.array([word << 32], np.uint64).view(np.int64)[0]
    ch["lo_nom"] = ch["lo_int"]
    ch["ca_int"] = ca_rate << 32
    ch["ca_nom"] = int(CPS / fs * 2 ** 32) << 32
    ch["fll_left"] = fll_epochs
    ch["next_sample"] = first + n0
    ch["lo_phase"] = ((first + n0) * word) & 0xFFFFFFFF
    ch["ca_pos"] = pos + n0 * ca_rate - FULL
    return ch


def host_capture(n, fs, sats, if_hz, scale, signed, seed, dc=(0.0, 0.0), nav=None, first_sample=0):
    """A small 8-bit complex capture made with numpy (gpsacq_generate_iq8_range's law, its own noise): sats = [(prn, amplitude,
    doppler, code_phase, carrier_phase)], dc added before rounding; samples first_sample .. first_sample + n - 1 of the law.
    Returns interleaved int8 / uint8."""
    rng = np.random.default_rng(seed)
    m = np.arange(first_sample, first_sample + n, dtype=np.float64)
    y = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for k, (prn, amp, dop, cp, ph) in enumerate(sats):
        q = np.floor((m + cp) * CPS * (1 + dop / L1) / fs).astype(np.int64)
        cyc = (if_hz + dop) / fs * m + ph
        s = amp * chips_pm1(prn)[q % 1023] * np.exp(2j * np.pi * (cyc - np.floor(cyc)))
        if nav is not None:
            s = s * np.asarray(nav[k])[(q // 20460) % len(nav[k])]
        y = y + s
    v = np.clip(np.rint(scale * y.real + dc[0]), -127, 127), np.clip(np.rint(scale * y.imag + dc[1]), -127, 127)
    out = np.empty(2 * n, np.int16)
    out[0::2], out[1::2] = v[0], v[1]
    return out.astype(np.int8) if signed else (out + 128).astype(np.uint8)


# ---- rails, means, the loop settings restated ---------------------------------------------------------------------------------
def to_rails(iq, signed):
    """The rail mapping: every sample that came out at -127 (the generators clamp to [-127, 127]) becomes -128, the value an
    ADC rests on while it clips: byte 0x80 as int8, byte 0x00 as uint8."""
    a = np.asarray(iq)
    out = a.copy()
    out[a == (-127 if signed else 1)] = -128 if signed else 0
    return out


def add_dc(iq, signed, dc):
    """an integer mean on both arms of a finished capture, clamped like the generator's own output (to [-127, 127])"""
    a = np.asarray(iq).astype(np.int16).reshape(-1, 2) - (0 if signed else 128)
    a = np.clip(a + np.array(dc, np.int16), -127, 127).ravel()
    return a.astype(np.int8) if signed else (a + 128).astype(np.uint8)


def rail_share(iq, signed):
    """(share of the bytes at -128, share at +127), as sample values"""
    a = np.asarray(iq).view(np.uint8).ravel()
    lo, hi = (0x80, 0x7F) if signed else (0x00, 0xFF)
    return float(np.mean(a == lo)), float(np.mean(a == hi))


def capture_rms(iq, signed, dc):
    """the RMS of v_i, v_q over the capture: what gpsacq_track_default_params_iq8 takes"""
    import track_ref
    vi, vq = track_ref.iq_samples(iq, signed, dc[0], dc[1])
    return math.sqrt((float(np.sum(vi.astype(np.int64) ** 2)) + float(np.sum(vq.astype(np.int64) ** 2))) / (2 * vi.size))


IQ8_GAIN = 4  # GPSACQ_TRACK_IQ8_GAIN


def default_params_iq8(fs, sample_rms):
    """gpsacq_track_default_params_iq8 restated from the header: gpsacq_track_default_params with the five shifts lowered by
    g = round(log2(4 rms^2)) and agc_lo, agc_hi multiplied by 2^g; g raised as far as keeps every shift <= 62; None
    (GPSACQ_ERR_UNSUPPORTED) for an RMS that is not a positive finite number or that would take a shift below 0 (lo_ki, lo_kp
    below 1: they run at shift + gain_adj)."""
    from test_track_ref import default_params, with_
    if not (sample_rms > 0) or not math.isfinite(sample_rms):
        return None
    p = default_params(fs)
    x = math.log2(IQ8_GAIN * sample_rms * sample_rms)
    g = int(math.copysign(math.floor(abs(x) + 0.5), x))  # to nearest, halves away from zero
    shifts = dict(lo_ki=p.lo_ki, lo_kp=p.lo_kp, ca_ki=p.ca_ki, ca_kp=p.ca_kp, fll_k=p.fll_k)
    g = max(g, max(shifts.values()) - 62)
    if any(v - g < (1 if k.startswith("lo_") else 0) for k, v in shifts.items()):
        return None
    return with_(p, agc_lo=math.floor(p.agc_lo * 2.0 ** g), agc_hi=math.floor(p.agc_hi * 2.0 ** g), **{k: v - g for k, v in shifts.items()})


def iq8_rms_bound(fs):
    """the sample RMS at which log2(4 rms^2) = ca_ki + 1/2, ca_ki the smallest shift of the 1-bit defaults: below it
    gpsacq_track_default_params_iq8 has an answer, above it none"""
    from test_track_ref import default_params
    return math.sqrt(2.0 ** (default_params(fs).ca_ki + 0.5) / IQ8_GAIN)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
SCENARIOS = ("default", "agc", "aid", "fll_long", "wrap", "window_terms", "window_tight", "epoch_len", "entered_lost", "max_epochs", "ragged_end")
IQ_SCALE = {2.046e6: 60, 2.8e6: 60, 4.0e6: 60, 5.456e6: 50, 6.5e6: 35, 8.184e6: 35, 10.0e6: 25, 16.368e6: 12, 20.0e6: 9, 40.0e6: 3}
IQ_DC = ((0, 0), (7, -5), (-128, 127))


def iq_case(fs):
    """What rotates over the rates of test_track_ref.FS_FC: the carrier (about +0.26 fs, about -0.21 fs, within 500 Hz of zero:
    there the channels' NCO words and lo_nom lie on both sides of the two's-complement wrap), int8 / uint8 bytes, and the mean
    (0, 0), (7, -5) or (-128, 127); eight of the nine (carrier, mean) pairs occur."""
    from test_track_ref import FS_FC
    i = [f for f, _ in FS_FC].index(fs)
    if_hz = (0.26 * fs, -0.21 * fs, float(np.random.default_rng(i).uniform(-500, 500)))[i % 3]
    return dict(i=i, if_hz=if_hz, signed=i % 2 == 0, dc=IQ_DC[(i + i // 3) % 3], scale=IQ_SCALE[fs])


def start_chan_iq(fs, if_hz, prn, fd, cp, th, s_min, p, **kw):
    """test_track_ref.start_chan for a satellite at if_hz + fd in a complex capture: the carrier word may be negative (two's
    complement), lo_nom is the word of if_hz"""
    from test_track_ref import s64, start_chan
    ch = start_chan(fs, if_hz, prn, fd, cp, th, s_min, p, **kw)
    ch["lo_nom"] = s64((int(np.rint(if_hz / fs * 2 ** 32)) % 2 ** 32) << 32)
    return ch


def run_and_audit_iq(buf, first, chans, p, max_epochs=None, sum_epochs=None, fmt=(True, 0, 0)):
    """the model over the window of interleaved bytes, then the reference's audit of every channel; fmt = (signed, dc_i, dc_q).
    Returns (reports, prompt, records, n_epochs); chans updated in place."""
    import track_ref
    if max_epochs is None:  # a short first epoch, then periods of at least spm / 2 samples
        max_epochs = len(buf) // 2 // max(int(p.min_epoch), int(p.max_epoch) // 4) + 2
    c0 = chans.copy()
    prompt, rec, ne = run_model_iq(buf, first, fmt[0], fmt[1:], chans, p, max_epochs)
    reps = [track_ref.audit(buf, first, c0[c], p, rec[c], ne[c], chans[c], max_epochs=max_epochs, prompt=prompt[c], sum_epochs=sum_epochs, iq=fmt)
            for c in range(chans.size)]
    return reps, prompt, rec, ne


_cache = {}


def sweep_iq(fs, capture=None, runner=None, first_offset=None, only=None):
    """The scenarios of test_track_ref.sweep at one sampling rate on multi-bit complex channels: ({scenario: runner's result}, the
    satellites, the window's first sample, its bytes, the case: iq_case(fs) plus n, rms and params).
    capture(sats, n_samples, first_sample, seed, case) makes the window of interleaved bytes, mean and rails included (default:
    host_capture, the mean added before rounding, then to_rails); runner(buf, first, chans, params, max_epochs=, sum_epochs=,
    fmt=) runs and checks one call (default: run_and_audit_iq, the model under the reference).  The window starts at any sample
    (first_offset: what is added to a multiple of 8) and holds n = 1 .. 7 mod 8 samples, so its byte count runs over the even
    residues 2 .. 14 mod 16 with the rates.  only: the scenarios to run (default all)."""
    from test_track_ref import FS_FC, TWO32, _prn_set, s64, spm_of, with_
    key = (fs, first_offset, only)
    if capture is None and runner is None and key in _cache:
        return _cache[key]
    run = runner or run_and_audit_iq
    case = iq_case(fs)
    i = case["i"]
    rng = np.random.default_rng(int(fs) + 1)
    spm = spm_of(fs)
    secs = 0.06 if fs >= 10e6 else 0.12
    se = 30 if fs >= 10e6 else None  # from 10 MHz on the sums of 30 seeded epochs per channel (the loop arithmetic of all)
    first = 8 * int(rng.integers(0, 1 << 20)) + (1 + (2 * i) % 7 if first_offset is None else first_offset)
    prns = _prn_set(i)
    sats = []
    for prn in prns:
        nav = 1 - 2 * rng.integers(0, 2, 9)
        # amplitudes a little below the 1-bit sweep's: four of them add sum a^2 / 2 <= 0.12 to the unit noise power of an arm, which
        # keeps scale * sqrt(1 + sum a^2 / 2 + 1 / 12 / scale^2) inside the supported RMS at every rate
        sats.append((prn, float(rng.uniform(0.15, 0.24)), float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spm)), float(rng.uniform(0, 1)), nav))
    n = int(secs * fs) // 8 * 8 + 1 + i % 7
    if_hz, signed, dc = case["if_hz"], case["signed"], case["dc"]
    if capture:
        buf = capture(sats, n, first, i, case)
    else:
        buf = to_rails(host_capture(n, fs, [s[:5] for s in sats], if_hz, float(case["scale"]), signed, seed=i, dc=(float(dc[0]), float(dc[1])),
                                    nav=[s[5] for s in sats], first_sample=first), signed)
    assert np.asarray(buf).size == 2 * n
    rms = capture_rms(buf, signed, dc)
    base = default_params_iq8(fs, rms)
    assert base is not None, (fs, rms)
    case = dict(case, n=n, rms=rms, params=base)
    fmt = (signed, dc[0], dc[1])
    s_min = first + int(rng.integers(0, spm))
    want = set(SCENARIOS if only is None else only)
    reps = {}

    def go(name, ch, p, buf=buf, **kw):
        if name in want:
            reps[name] = run(buf, first, ch, p, fmt=fmt, **kw)

    def chans_for(p, dop_err=None):
        return np.concatenate([start_chan_iq(fs, if_hz, s[0], s[2], s[3], s[4], s_min, p,
                                             dop_err=float(rng.uniform(-60, 60)) if dop_err is None else dop_err) for s in sats])

    # defaults: the FLL pull-in (it is longer than these windows)
    go("default", chans_for(base), base, sum_epochs=se)
    # AGC: a 3-epoch poll, any power above agc_hi and below agc_lo (|IP|, |QP| <= 2 * 256 n), so that gain_adj goes to -1 and back
    # at every poll; the ring wraps
    p = with_(base, agc_period=3, agc_hi=0, agc_lo=(512 * 2 * spm) ** 2, fll_epochs=20)
    go("agc", chans_for(p), p, sum_epochs=se)
    # the code-aided carrier reset, FLL off; and an FLL longer than the run
    p = with_(base, aid_epoch=37, fll_epochs=0)
    go("aid", chans_for(p, dop_err=0.0), p, sum_epochs=se)
    p = with_(base, fll_epochs=100000)
    go("fll_long", chans_for(p), p, sum_epochs=se)
    # code phase within a chip of the 1022 -> 0 wrap (a short first epoch), min_epoch 1
    p = with_(base, min_epoch=1)
    ch = np.concatenate([start_chan_iq(fs, if_hz, s[0], s[2], s[3], s[4], s_min, p, at_chip=a) for s, a in zip(sats, (1022.05, 1022.49, 1022.51, 1022.97))])
    go("wrap", ch, p)
    # each of the four window terms alone: integrators 3.75 / 3.25 units of 2^32 off nominal against a window of 3.5 units, and
    # the smallest gains there are.  One epoch's error term must stay below the 1/8 unit that decides (2^29): the channels
    # therefore run PRNs that are not in the capture, where IP, QP, IE .. are noise sums of deviation sqrt(2 n) rms and the
    # products IP QP, IE^2 - IL^2 about 2 n rms^2 < 2^25 at every rate of the sweep
    w = 3 * TWO32 + TWO32 // 2
    p = with_(base, lo_ki=1, lo_kp=1, ca_ki=0, ca_kp=0, fll_epochs=0, lo_window=w, ca_window=w)
    ch = chans_for(p, dop_err=0.0)
    for f in ("lo", "ca"):  # both loops on their nominal words, then one integrator moved
        ch[f + "_int"] = ch[f + "_nom"]
        ch[f + "_rate"] = (ch[f + "_nom"].astype(np.uint64) >> np.uint64(32)).astype(np.uint32)
    ch["prn"] = [q for q in range(1, 33) if q not in prns][:len(sats)]
    for c, (field, off) in enumerate((("lo_int", 3.75), ("lo_int", -3.25), ("ca_int", 3.75), ("ca_int", -3.25))):
        v = (int(ch[field.replace("int", "nom")][c]) + int(off * TWO32)) % 2 ** 64
        ch[field][c] = s64(v)
        ch[field.replace("int", "rate")][c] = v >> 32
    go("window_terms", ch, p)
    # tight default windows: lost on the way
    p = with_(base, lo_window=base.lo_window // 200, ca_window=base.ca_window // 50)
    go("window_tight", chans_for(p), p, sum_epochs=se)
    # min_epoch / max_epoch: a short first epoch against the default min_epoch; a code NCO 1 % slow against max_epoch = 1.005 spm
    # (the code window wide enough that only the epoch length decides); a code word whose period is max_epoch + 0.3 samples,
    # started half a sample into its first: one epoch of max_epoch samples, then one of max_epoch + 1
    top = int(spm * 1.005) + 1
    p = with_(base, max_epoch=top, ca_window=base.ca_window * 1000)
    ch = np.concatenate([start_chan_iq(fs, if_hz, s[0], s[2], s[3], s[4], s_min, p, at_chip=1022.6) for s in sats[:1]] + [chans_for(p)[1:3]])
    ch["ca_rate"][1] = int(ch["ca_rate"][1]) * 99 // 100
    ch["ca_int"][1] = int(ch["ca_rate"][1]) << 32
    ch["ca_rate"][2] = round(1023 * TWO32 / (top + 0.3))
    ch["ca_pos"][2] = int(ch["ca_rate"][2]) // 2
    ch["ca_int"][2] = int(ch["ca_rate"][2]) << 32
    go("epoch_len", ch, p)
    # a channel that starts LOST, among live ones; and a max_epochs cut
    ch = chans_for(base)
    ch["status"][1] = 1
    go("entered_lost", ch, base, sum_epochs=se)
    go("max_epochs", chans_for(base), base, max_epochs=50)
    # a window cut where an epoch of a channel ends, a few samples past a multiple of 8: that epoch's last samples lie in the
    # window's last, incomplete 16-byte group (no epoch of the runs above needs to reach theirs).  The cut comes from a run of the
    # model; that channel must then stop exactly at the window's end.
    if "ragged_end" in want:
        ch = chans_for(base)
        probe = ch.copy()
        _, prec, pne = run_model_iq(buf, first, signed, dc, probe, base, 64)
        ends = [(int(prec[c, t + 1]["sample"]) - first, c) for c in range(ch.size) for t in range(8, int(pne[c]) - 1)]
        pick = [e for e in ends if e[0] % 8 == 1 + (i + 3) % 7] or [e for e in ends if e[0] % 8]  # (at 4 MHz an epoch is 4000 samples: one residue per channel)
        m, c = pick[0]
        go("ragged_end", ch, base, buf=buf[:2 * m])
        assert int(ch["next_sample"][c]) == first + m and ch["status"][c] == 0
    out = (reps, sats, first, buf, case)
    if capture is None and runner is None:
        _cache[key] = out
    return out


def check_sweep_reports(reps):
    """what every run of the sweep must have reached, on the branch reports of whichever scenarios were run"""
    r = {name: v[0] for name, v in reps.items()}
    if "window_terms" in r:
        assert [x["lost"] for x in r["window_terms"]] == [{"lo_int"}, {"lo_rate"}, {"ca_int"}, {"ca_rate"}]
    if "epoch_len" in r:
        assert [x["lost"] for x in r["epoch_len"]] == [{"min_epoch"}, {"max_epoch"}, {"max_epoch"}]
        assert r["epoch_len"][2]["epochs"] == 1
    if "entered_lost" in r:
        assert r["entered_lost"][1]["stop"] == "entered_lost"
    if "agc" in r:
        assert all(x["agc_down"] > 0 and x["agc_up"] > 0 and x["ring_wraps"] > 0 for x in r["agc"])
    if "aid" in r:
        assert all(x["aid"] == [37] for x in r["aid"])
    if "max_epochs" in r:
        assert all(x["stop"] == "max_epochs" for x in r["max_epochs"])
    if "ragged_end" in r:
        assert all(x["stop"] == "window" and x["epochs"] >= 7 for x in r["ragged_end"])
    if "default" in r:
        assert sum(x["stop"] == "window" for x in r["default"]) >= len(r["default"]) - 1  # at least n - 1 channels end TRACK_OK


# ---- lock from 60 Hz off at 10, 20 and 40 MHz ---------------------------------------------------------------------------------
LOCK_SECS = 1.1
LOCK_CASES = {10.0e6: dict(if_hz=2.6e6, scale=25, signed=True, dc=(0, 0)),       # the reference's HackRF flow: 10e6, IF 2.6e6
              20.0e6: dict(if_hz=-0.21 * 20.0e6, scale=9, signed=False, dc=(7, -5)),
              40.0e6: dict(if_hz=0.26 * 40.0e6, scale=3, signed=True, dc=(0, 0))}


def lock_setup(fs):
    """the recipe of test_track_ref.test_defaults_lock_at_high_fs: its two satellites of amplitude 0.25 (Doppler, code and carrier
    phase, NAV bits from the same seed) over 1.1 s; (sats with nav, n_samples, case)"""
    from test_track_ref import spm_of
    rng = np.random.default_rng(7)
    sats = [(p, 0.25, float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spm_of(fs))), float(rng.uniform(0, 1)), 1 - 2 * rng.integers(0, 2, 7))
            for p in (6, 29)]
    return sats, int(LOCK_SECS * fs) // 8 * 8, LOCK_CASES[fs]


def lock_params_and_chans(fs, buf, sats, case):
    """the settings of the RMS of the capture's first 2^22 samples, and the two channels started at sample 0"""
    rms = capture_rms(np.asarray(buf).ravel()[:2 << 22], case["signed"], case["dc"])
    p = default_params_iq8(fs, rms)
    assert p is not None, rms
    ch = np.concatenate([start_chan_iq(fs, case["if_hz"], s[0], s[2], s[3], s[4], 0, p, dop_err=(-60.0, 60.0)[k]) for k, s in enumerate(sats)])
    return p, ch, rms


def host_lock_capture(fs, sats, n, case, step=1 << 22):
    return np.concatenate([to_rails(host_capture(min(step, n - a), fs, [s[:5] for s in sats], case["if_hz"], float(case["scale"]), case["signed"], seed=a,
                                                 dc=(float(case["dc"][0]), float(case["dc"][1])), nav=[s[5] for s in sats], first_sample=a), case["signed"])
                           for a in range(0, n, step)])


def assert_locked(fs, case, sats, reps, prompt, rec, ne):
    """both channels OK to the end of the window and past the FLL; after epoch 700 the carrier deviates less than the 60 Hz it
    started with; the prompt power on I at least 10 times that on Q.  Returns the figures per channel."""
    out = []
    for c, s in enumerate(sats):
        assert reps[c]["stop"] == "window" and reps[c]["costas_epochs"] > 500, (c, reps[c])
        m = int(ne[c])
        lo_hz = rec[c, 700:m]["lo_rate"].astype(np.int32).astype(np.float64) / 2 ** 32 * fs - case["if_hz"]
        dev = float(np.abs(lo_hz - s[2]).max())
        ip, qp = prompt[c, 700:m, 0].astype(float), prompt[c, 700:m, 1].astype(float)
        ratio = float(np.mean(ip ** 2) / np.mean(qp ** 2))
        out.append((dev, ratio))
        assert dev < 60.0, (c, dev)
        assert ratio >= 10.0, (c, ratio)
    return out
