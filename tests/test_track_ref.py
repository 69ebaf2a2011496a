"""The CPU model of a tracking channel (tests/c/track_model.c) against the independent reference of tests/track_ref.py, bit for
bit, on captures built in numpy, over sampling rates 2.046 .. 40 MHz, all 32 PRNs and parameter sets that reach every branch of
"THE CHANNEL MODEL" (include/gpsacq.h); and the NAV decoder (gpsacq_nav_bits, gpsacq_nav_subframes) against a restatement of
its header text.  No GPU: the model is compiled with gcc, the NAV decoder is host code of libgpsacq.so."""
import math

import numpy as np
import pytest

import track_ref
from track_helpers import encode_subframe, make_subframe_words, run_model

L1, CPS = 1575.42e6, 1.023e6
TWO32 = 2 ** 32
FS_FC = [(2.046e6, 0.5115e6), (4.0e6, 1.25e6), (5.456e6, 4.092e6), (6.5e6, 1.6e6), (10.0e6, 2.5e6), (16.368e6, 4.092e6),
         (20.0e6, 5.0e6), (40.0e6, 10.0e6)]
HIGH_FS = {16.368e6, 20.0e6, 40.0e6}


def spm_of(fs):
    """gpsacq_info.num_lags: the smallest integer >= fs / 1000, at most 40000"""
    return min(math.ceil(fs / 1000), 40000)


def default_params(fs):
    """gpsacq_track_default_params, restated from the header's params comment"""
    import gpsacq
    spm = spm_of(fs)
    adj = round((3 if spm > 10000 else 2) * math.log2(10000 / spm))
    r = spm / 10000
    p = gpsacq.TrackParams()
    p.lo_ki, p.lo_kp, p.ca_ki, p.ca_kp, p.fll_k = 20 + adj, 27 + adj, 11 + adj, 23 + adj, 25 + adj
    p.fll_epochs, p.aid_epoch, p.agc_period = 500, -1, 250
    p.agc_lo, p.agc_hi = math.floor(1200.0 ** 2 * r * r), math.floor(1400.0 ** 2 * r * r)
    p.lo_window = int(10000.0 / fs * 2.0 ** 64)
    p.ca_window = int(4.0 * 10000.0 / 1540.0 / fs * 2.0 ** 64)
    p.min_epoch, p.max_epoch = spm // 2, min(2 * spm, 65535)
    return p


def with_(p, **kw):
    """a copy of TrackParams p with fields overridden by name"""
    import gpsacq
    q = gpsacq.TrackParams.from_buffer_copy(bytes(p))
    for k, v in kw.items():
        setattr(q, k, int(v))
    return q


def make_capture(fs, fc, sats, n_samples, first_sample=0, noise=1.0, seed=0):
    """1-bit capture (bit 1 = negative) of sign(sum a chip nav cos(2 pi ((fc + fd) / fs m + theta)) + noise), the generator's law:
    sats = [(prn, a, fd, code_phase_samples, theta, nav +-1 array)].  Returns packed bytes (LSB first)."""
    rng = np.random.default_rng(seed)
    m = np.arange(first_sample, first_sample + n_samples, dtype=np.int64)
    y = noise * rng.standard_normal(n_samples)
    for prn, a, fd, cp, th, nav in sats:
        q = np.floor((m.astype(np.float64) + cp) * (CPS * (1 + fd / L1) / fs)).astype(np.int64)
        c = 1 - 2 * track_ref.chips(prn)[q % 1023].astype(np.float64)
        d = np.asarray(nav, np.float64)[(q // 20460) % len(nav)]
        ph = (fc + fd) / fs * m.astype(np.float64) + th
        y += a * c * d * np.cos(2 * np.pi * (ph - np.floor(ph)))
    return np.packbits((y < 0).astype(np.uint8), bitorder="little")


def s64(v):
    """an unsigned 64-bit pattern as the int64 field value"""
    v %= 2 ** 64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def start_chan(fs, fc, prn, fd, cp, th, s_min, p, dop_err=0.0, phase_err=0.0, at_chip=None):
    """A channel state for a satellite of make_capture's law: NCOs at its true code rate and at fd + dop_err, started at the first
    code epoch after sample s_min (or, with at_chip, at the first sample after s_min whose prompt position is past that chip)."""
    import gpsacq
    cps = CPS * (1 + fd / L1) / fs
    ch = np.zeros(1, gpsacq.TRACK_CHAN_DTYPE)
    ch["prn"] = prn
    ch["lo_rate"] = lo_rate = int(round((fc + fd + dop_err) / fs * TWO32)) % TWO32
    ch["ca_rate"] = ca_rate = int(round(cps * TWO32))
    ch["lo_int"] = s64(lo_rate << 32)
    ch["ca_int"] = s64(ca_rate << 32)
    ch["lo_nom"] = s64(int(fc / fs * TWO32) << 32)
    ch["ca_nom"] = s64(int(CPS / fs * TWO32) << 32)
    ch["fll_left"] = p.fll_epochs
    pos0 = (s_min + cp) * cps
    if at_chip is None:
        k = math.floor(pos0 / 1023) + 1
        s0 = math.ceil(k * 1023 / cps - cp)
        chip = (s0 + cp) * cps - k * 1023
    else:
        k = math.floor((pos0 - at_chip) / 1023) + 1
        s0 = math.ceil((k * 1023 + at_chip) / cps - cp)
        chip = (s0 + cp) * cps - k * 1023
    ch["next_sample"] = s0
    ch["ca_pos"] = min(int(chip * TWO32) % (1023 * TWO32), 1023 * TWO32 - 1)
    ph = (fc + fd) / fs * s0 + th + phase_err
    ch["lo_phase"] = int((ph - math.floor(ph)) * TWO32) % TWO32
    return ch


def run_and_audit(buf, first, chans, p, max_epochs=None, sum_epochs=None):
    """model over the window, then the reference's audit of every channel; returns (reports, prompt, records, n_epochs, chans)"""
    if max_epochs is None:  # a short first epoch, then periods of at least spm / 2 samples
        max_epochs = len(buf) * 8 // max(int(p.min_epoch), int(p.max_epoch) // 4) + 2
    c0 = chans.copy()
    prompt, rec, ne = run_model(buf, first, chans, p, max_epochs)
    reps = [track_ref.audit(buf, first, c0[c], p, rec[c], ne[c], chans[c], max_epochs=max_epochs, prompt=prompt[c], sum_epochs=sum_epochs)
            for c in range(chans.size)]
    return reps, prompt, rec, ne


def _prn_set(i):
    """four PRNs per sampling rate: the eight rates cover all 32"""
    return [int(x) for x in np.random.default_rng(77).permutation(np.arange(1, 33))[4 * i:4 * i + 4]]


_cache = {}


def sweep(fs, fc, capture=None, runner=None, first_offset=0):
    """All scenarios at one sampling rate: {scenario: runner's result}, the satellites, the window's first sample and bytes.
    capture(sats, n_samples, first_sample, seed) makes the window (default: make_capture); runner(buf, first, chans, params,
    max_epochs=, sum_epochs=) runs and checks one call (default: run_and_audit, the model and the reference)."""
    if capture is None and fs in _cache:
        return _cache[fs]
    runner = runner or run_and_audit
    i = [f for f, _ in FS_FC].index(fs)
    rng = np.random.default_rng(int(fs))
    spm = spm_of(fs)
    secs = 0.15 if fs >= 10e6 else 0.4
    se = 60 if fs >= 10e6 else None  # above 10 MHz the sums of 60 seeded epochs per channel (the loop arithmetic of all)
    first = 8 * int(rng.integers(0, 1 << 20)) + (1 << 26 if fs > 9e6 else 0) + first_offset
    prns = _prn_set(i)
    sats = []
    for prn in prns:
        nav = 1 - 2 * rng.integers(0, 2, 9)
        sats.append((prn, float(rng.uniform(0.2, 0.35)), float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spm)), float(rng.uniform(0, 1)), nav))
    n = int(secs * fs) // 8 * 8
    buf = capture(sats, n, first, i) if capture else make_capture(fs, fc, sats, n, first, seed=i)
    base = default_params(fs)
    s_min = first + int(rng.integers(0, spm))
    reps = {}

    def chans_for(p, dop_err=None):
        return np.concatenate([start_chan(fs, fc, s[0], s[2], s[3], s[4], s_min, p,
                                          dop_err=float(rng.uniform(-60, 60)) if dop_err is None else dop_err) for s in sats])

    # defaults (the FLL pull-in then Costas; at 16 MHz and above the defaults only exist since max_epoch may reach 65535)
    reps["default"] = runner(buf, first, chans_for(base), base, sum_epochs=se)
    # AGC: a 3-epoch poll, any power above agc_hi and below agc_lo, so that gain_adj goes to -1 and back at every poll; the ring wraps
    p = with_(base, agc_period=3, agc_hi=0, agc_lo=4 * spm * spm, fll_epochs=20)
    reps["agc"] = runner(buf, first, chans_for(p), p, sum_epochs=se)
    # the code-aided carrier reset, FLL off; and an FLL longer than the run
    p = with_(base, aid_epoch=37, fll_epochs=0)
    reps["aid"] = runner(buf, first, chans_for(p, dop_err=0.0), p, sum_epochs=se)
    p = with_(base, fll_epochs=100000)
    reps["fll_long"] = runner(buf, first, chans_for(p), p, sum_epochs=se)
    # code phase within a chip of the 1022 -> 0 wrap (a short first epoch), min_epoch 1
    p = with_(base, min_epoch=1)
    ch = np.concatenate([start_chan(fs, fc, s[0], s[2], s[3], s[4], s_min, p, at_chip=a) for s, a in zip(sats, (1022.05, 1022.49, 1022.51, 1022.97))])
    reps["wrap"] = runner(buf, first, ch, p)
    # each of the four window terms alone: integrators 3.75 / 3.25 units of 2^32 off nominal against a window of 3.5 units, and
    # gains so small that the NCO word is the integrator's floor
    w = 3 * TWO32 + TWO32 // 2
    p = with_(base, lo_ki=1, lo_kp=1, ca_ki=0, ca_kp=0, fll_epochs=0, lo_window=w, ca_window=w)
    ch = chans_for(p, dop_err=0.0)
    for f in ("lo", "ca"):  # both loops on their nominal words, then one integrator moved
        ch[f + "_int"] = ch[f + "_nom"]
        ch[f + "_rate"] = (ch[f + "_nom"].astype(np.uint64) >> np.uint64(32)).astype(np.uint32)
    for c, (field, off) in enumerate((("lo_int", 3.75), ("lo_int", -3.25), ("ca_int", 3.75), ("ca_int", -3.25))):
        v = (int(ch[field.replace("int", "nom")][c]) + int(off * TWO32)) % 2 ** 64
        ch[field][c] = s64(v)
        ch[field.replace("int", "rate")][c] = v >> 32
    reps["window_terms"] = runner(buf, first, ch, p)
    # tight default windows: lost on the way
    p = with_(base, lo_window=base.lo_window // 200, ca_window=base.ca_window // 50)
    reps["window_tight"] = runner(buf, first, chans_for(p), p, sum_epochs=se)
    # min_epoch / max_epoch: a short first epoch against the default min_epoch; a code NCO 1 % slow against max_epoch = 1.005 spm
    # (the code window wide enough, and below ca_nom, so that only the epoch length decides)
    # a code word whose period is max_epoch + 0.3 samples, started half a sample into its first: one epoch of max_epoch samples,
    # then one of max_epoch + 1
    top = int(spm * 1.005) + 1
    p = with_(base, max_epoch=top, ca_window=base.ca_window * 1000)
    ch = np.concatenate([start_chan(fs, fc, s[0], s[2], s[3], s[4], s_min, p, at_chip=1022.6) for s in sats[:1]] + [chans_for(p)[1:3]])
    ch["ca_rate"][1] = int(ch["ca_rate"][1]) * 99 // 100
    ch["ca_int"][1] = int(ch["ca_rate"][1]) << 32
    ch["ca_rate"][2] = round(1023 * TWO32 / (top + 0.3))
    ch["ca_pos"][2] = int(ch["ca_rate"][2]) // 2
    ch["ca_int"][2] = int(ch["ca_rate"][2]) << 32
    reps["epoch_len"] = runner(buf, first, ch, p)
    # a channel that starts LOST, among live ones; and a max_epochs cut
    ch = chans_for(base)
    ch["status"][1] = 1
    reps["entered_lost"] = runner(buf, first, ch, base, sum_epochs=se)
    reps["max_epochs"] = runner(buf, first, chans_for(base), base, max_epochs=50)
    if capture is None:
        _cache[fs] = (reps, sats, first, buf)
    return reps, sats, first, buf


@pytest.mark.parametrize("fs,fc", FS_FC, ids=[f"{fs / 1e6:g}MHz" for fs, _ in FS_FC])
def test_model_equals_reference(fs, fc):
    reps, sats, first, buf = sweep(fs, fc)
    r = {k: [x for x in v[0]] for k, v in reps.items()}
    assert all(x["stop"] == "entered_lost" for x in r["entered_lost"][1:2])
    assert all(x["stop"] == "max_epochs" for x in r["max_epochs"])
    assert [x["lost"] for x in r["window_terms"]] == [{"lo_int"}, {"lo_rate"}, {"ca_int"}, {"ca_rate"}]
    assert [x["lost"] for x in r["epoch_len"]] == [{"min_epoch"}, {"max_epoch"}, {"max_epoch"}]
    assert r["epoch_len"][2]["epochs"] == 1
    assert sum(x["short_first"] for x in r["wrap"]) >= 2  # (a start past 1022.97 chips may land on the next period)


@pytest.mark.parametrize("fs,fc", [x for x in FS_FC if x[0] in HIGH_FS], ids=lambda v: f"{v / 1e6:g}MHz" if v > 8e6 else None)
def test_defaults_lock_at_high_fs(fs, fc):
    """With the default parameters of 16.368, 20 and 40 MHz (which gpsacq_track refused above 16.384 MHz before max_epoch could
    reach 65535), two satellites 60 Hz off the hit go through the 500-epoch FLL pull-in and stay locked under the Costas loop:
    OK to the end, the carrier within 40 Hz of the truth, the prompt power on I.  The model run is audited too."""
    rng = np.random.default_rng(7)
    sats = [(p, 0.25, float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spm_of(fs))), float(rng.uniform(0, 1)), 1 - 2 * rng.integers(0, 2, 7))
            for p in (6, 29)]
    n = int(1.1 * fs) // 8 * 8
    step = 1 << 22
    buf = np.concatenate([make_capture(fs, fc, sats, min(step, n - a), a, seed=a) for a in range(0, n, step)])
    p = default_params(fs)
    ch = np.concatenate([start_chan(fs, fc, s[0], s[2], s[3], s[4], 0, p, dop_err=(-60.0, 60.0)[k]) for k, s in enumerate(sats)])
    reps, prompt, rec, ne = run_and_audit(buf, 0, ch, p, sum_epochs=30)
    for c, s in enumerate(sats):
        assert reps[c]["stop"] == "window" and reps[c]["costas_epochs"] > 500, (c, reps[c])
        m = int(ne[c])
        lo_hz = rec[c, 700:m]["lo_rate"].astype(np.float64) / TWO32 * fs - fc
        assert np.abs(lo_hz - s[2]).max() < 40.0, (c, np.abs(lo_hz - s[2]).max())
        ip, qp = prompt[c, 700:m, 0].astype(float), prompt[c, 700:m, 1].astype(float)
        assert np.mean(ip ** 2) > 10 * np.mean(qp ** 2), c


def test_branch_coverage():
    """every branch the sweep aims at was taken somewhere"""
    tot = dict(agc_down=0, agc_up=0, ring_wraps=0, fll_epochs=0, costas_epochs=0, costas_adj_epochs=0, aid=0, late_wrap=0, early_wrap=0,
               short_first=0)
    lost, stops, prns = set(), set(), set()
    for fs, fc in FS_FC:
        reps, sats, _, _ = sweep(fs, fc)
        prns |= {s[0] for s in sats}
        for v in reps.values():
            for x in v[0]:
                for k in tot:
                    tot[k] += len(x[k]) if k == "aid" else int(x[k])
                lost |= x["lost"]
                stops.add(x["stop"])
    assert all(v > 0 for v in tot.values()), tot
    assert lost == {"lo_int", "lo_rate", "ca_int", "ca_rate", "min_epoch", "max_epoch"}
    assert stops == {"window", "max_epochs", "lost", "entered_lost"}
    assert prns == set(range(1, 33))


# ---- NAV decoder ------------------------------------------------------------------------------------------------------
def ref_nav_bits(ip, first_epoch, sync_epochs, max_bits):
    """gpsacq_nav_bits from its header text: (ok, bits, bit_epoch0, n_bits).  'Sign' is that of the summed I arm: negative
    below 0, so an ip of exactly 0 counts as positive, as a 20-epoch sum of exactly 0 gives bit 0."""
    ip = [int(v) for v in ip]
    n = len(ip)
    ns = n if sync_epochs <= 0 or sync_epochs > n else sync_epochs
    hist = [0] * 20
    for k in range(1, ns):
        if (ip[k - 1] < 0) != (ip[k] < 0):
            hist[(first_epoch + k) % 20] += 1
    best = max(range(20), key=lambda b: (hist[b], -b))  # the fullest bin, ties to the lowest
    runner = max(h for b, h in enumerate(hist) if b != best)
    if hist[best] == 0 or hist[best] < 2 * runner:
        return False, [], -1, 0
    k0 = (best - first_epoch) % 20
    bits = [1 if sum(ip[k:k + 20]) < 0 else 0 for k in range(k0, n - 19, 20)]
    return True, bits[:max_bits], first_epoch + k0, min(len(bits), max_bits)


_STAR = [29, 30, 29, 30, 30, 29]
_EQ = [[1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23], [2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24],
       [1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22], [2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23],
       [1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24], [3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24]]  # IS-GPS-200 Table 20-XIV


def ref_nav_subframes(bits, max_out):
    """gpsacq_nav_subframes from its header text (the scan of CHANNEL::ParityCheck()): (subframes, n_out, n_parity_fail)"""
    b = [int(v) & 1 for v in bits]
    out, n_out, n_fail, i = [], 0, 0, 0
    while i + 300 <= len(b):
        pre = b[i:i + 8]
        if pre == [1, 0, 0, 0, 1, 0, 1, 1]:
            inv = 0
        elif pre == [0, 1, 1, 1, 0, 1, 0, 0]:
            inv = 1
        else:
            i += 1
            continue
        d29, d30, words, bad = inv, inv, [], -1
        for w in range(10):
            D = b[i + 30 * w:i + 30 * w + 30]
            d = [D[k] ^ d30 for k in range(24)]
            for q in range(6):
                par = d29 if _STAR[q] == 29 else d30
                for idx in _EQ[q]:
                    par ^= d[idx - 1]
                if par != D[24 + q]:
                    bad = w
            if bad >= 0:
                break
            words.append(int("".join(map(str, d)), 2))
            d29, d30 = D[28], D[29]
        if bad >= 0:
            n_fail += 1
            i += 30 * (bad + 1)
            continue
        if n_out < max_out:
            out.append((i, inv, words, (words[1] >> 2) & 7, words[1] >> 7))
        n_out += 1
        i += 300
    return out, n_out, n_fail


def lib_nav_bits(ip, first_epoch, sync_epochs, max_bits):
    import ctypes
    import gpsacq
    lib = gpsacq.load_library()
    a = np.ascontiguousarray(np.asarray(ip, np.int32))
    out = np.full(max(max_bits, 1), 0xEE, np.uint8)
    e0, nb = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.gpsacq_nav_bits(a.ctypes.data_as(ctypes.c_void_p), int(a.size), int(first_epoch), int(sync_epochs), out.ctypes.data_as(ctypes.c_void_p),
                             int(max_bits), ctypes.byref(e0), ctypes.byref(nb))
    assert (out[nb.value:] == 0xEE).all(), "wrote past n_bits"
    return rc == 0, out[:nb.value].tolist(), e0.value, nb.value


def lib_nav_subframes(bits, max_out):
    import ctypes
    import gpsacq
    lib = gpsacq.load_library()
    b = np.ascontiguousarray(np.asarray(bits, np.uint8))
    out = np.zeros(max(max_out, 1) + 1, gpsacq.SUBFRAME_DTYPE)
    out[:] = np.frombuffer(b"\xee" * out.nbytes, gpsacq.SUBFRAME_DTYPE)
    n, nf = ctypes.c_int(), ctypes.c_int()
    assert lib.gpsacq_nav_subframes(b.ctypes.data_as(ctypes.c_void_p), int(b.size), out.ctypes.data_as(ctypes.c_void_p), int(max_out),
                                    ctypes.byref(n), ctypes.byref(nf)) == 0
    k = min(n.value, max_out)
    assert out[k:].tobytes() == b"\xee" * out[k:].nbytes, "wrote past max_out"
    sf = [(int(r["bit_offset"]), int(r["inverted"]), [int(w) for w in r["words"]], int(r["id"]), int(r["tow"])) for r in out[:k]]
    return sf, n.value, nf.value


def _nav_case(rng):
    """junk, then upright or inverted runs of subframes (with the D29* / D30* of each word carried on), damaged at random"""
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        junk = rng.integers(0, 2, int(rng.integers(0, 400))).astype(np.uint8)
        if junk.size > 20 and rng.random() < 0.7:  # preamble look-alikes in the junk
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, junk.size - 8))
                junk[at:at + 8] = [1, 0, 0, 0, 1, 0, 1, 1] if rng.random() < 0.5 else [0, 1, 1, 1, 0, 1, 0, 0]
        parts.append(junk)
        d29 = d30 = 0
        run = []
        for k in range(int(rng.integers(1, 5))):
            b, d29, d30 = encode_subframe(make_subframe_words(int(rng.integers(0, 1 << 17)), int(rng.integers(1, 6)), rng), d29, d30)
            run += b
        run = np.array(run, np.uint8)
        parts.append(1 - run if rng.random() < 0.5 else run)
    bits = np.concatenate(parts)
    for _ in range(int(rng.choice([0, 0, 1, 2]))):  # single and double bit flips
        bits[int(rng.integers(0, bits.size))] ^= 1
    return bits


@pytest.mark.usefixtures("hip_artifacts")
def test_nav_subframes_fuzz():
    rng = np.random.default_rng(2024)
    seen = dict(inverted=0, upright=0, fail=0, truncated=0)
    for case in range(400):
        bits = _nav_case(rng)
        want = ref_nav_subframes(bits, 1 << 20)
        max_out = int(rng.integers(0, want[1] + 2)) if case % 3 == 0 else want[1] + 1
        want = ref_nav_subframes(bits, max_out)
        got = lib_nav_subframes(bits, max_out)
        assert got == want, case
        seen["inverted"] += sum(s[1] for s in want[0])
        seen["upright"] += sum(1 - s[1] for s in want[0])
        seen["fail"] += want[2] > 0
        seen["truncated"] += max_out < want[1]
    assert all(v > 10 for v in seen.values()), seen


def _bit_ip(rng, n, phase, amp, noise, zeros=0.0):
    """prompt I of n epochs whose data bits change at epochs == phase (mod 20)"""
    nb = n // 20 + 2
    d = 1 - 2 * rng.integers(0, 2, nb)
    k = np.arange(n)
    ip = amp * d[(k - phase + 20) // 20] + rng.normal(0, noise, n)
    ip = np.round(ip).astype(np.int32)
    ip[rng.random(n) < zeros] = 0
    return ip


@pytest.mark.usefixtures("hip_artifacts")
def test_nav_bits_fuzz():
    rng = np.random.default_rng(99)
    seen = dict(ok=0, nosync=0, zero_sum=0, tie=0, exactly_twice=0)
    for case in range(600):
        n = int(rng.integers(0, 900))
        first = int(rng.integers(0, 5000))
        kind = case % 6
        ph = int(rng.integers(0, 20))
        ip = _bit_ip(rng, n, ph, float(rng.uniform(5, 2000)), float(rng.choice([0, 50, 800, 3000])), zeros=float(rng.choice([0, 0.05, 0.5])))
        if kind == 1 and n >= 40:  # bit windows whose sum is exactly 0 (the bit changes around them keep the sync)
            for k in range(ph, n - 19, 20):
                if rng.random() < 0.3:
                    v = rng.integers(-50, 50, 10)
                    ip[k:k + 20] = np.concatenate([v, -v])[rng.permutation(20)]
        if kind == 2 and n >= 60:  # a histogram tie: changes in exactly two bins, the same number in each
            ip = np.ones(n, np.int32)
            a, b = sorted(rng.choice(20, 2, replace=False))
            sgn = 1
            for k in range(1, n):
                if (first + k) % 20 in (a, b):
                    sgn = -sgn
                ip[k] = sgn * int(rng.integers(1, 9))
        if kind == 3 and n >= 100:  # the winner with exactly twice the runner-up (sync), or one fewer (none)
            ip = np.ones(n, np.int32)
            a, b = rng.choice(20, 2, replace=False)
            na = int(rng.integers(2, max(3, n // 20)))
            nb = na // 2
            ka = [k for k in range(1, n) if (first + k) % 20 == a][:na]
            kb = [k for k in range(1, n) if (first + k) % 20 == b][:nb]
            if rng.random() < 0.5 and kb and len(ka) == 2 * len(kb):
                ka = ka[:-1]
            flip = np.zeros(n, bool)
            flip[ka + kb] = True
            ip = np.where(np.cumsum(flip) % 2 == 1, -1, 1).astype(np.int32) * rng.integers(1, 30, n).astype(np.int32)
        sync = int(rng.choice([0, -3, 1, n + 5, max(1, n // 3), n]))
        max_bits = int(rng.choice([0, 1, 3, n // 20 + 1]))
        want = ref_nav_bits(ip, first, sync, max_bits)
        got = lib_nav_bits(ip, first, sync, max_bits)
        assert got == want, (case, kind, n, first, sync, max_bits)
        seen["ok" if want[0] else "nosync"] += 1
        if want[0]:
            k0 = want[2] - first
            sums = [int(ip[k:k + 20].sum()) for k in range(k0, n - 19, 20)]
            seen["zero_sum"] += 0 in sums
        ns = n if sync <= 0 or sync > n else sync
        hist = np.bincount([(first + k) % 20 for k in range(1, ns) if (ip[k - 1] < 0) != (ip[k] < 0)], minlength=20)
        top = np.sort(hist)[::-1]
        seen["tie"] += bool(top[0] > 0 and top[0] == top[1])
        seen["exactly_twice"] += bool(top[0] > 0 and top[0] == 2 * top[1])
    assert all(v > 5 for v in seen.values()), seen
