"""Helpers of the 8-bit IQ tracking tests: the CPU model of a multi-bit complex channel (tests/c/track_model_iq.c, compiled with
gcc on first use), a numpy restatement of its six sums, and host-side makers of small IQ captures and channel states (the CPU
tests have no engine)."""
import ctypes
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


def host_capture(n, fs, sats, if_hz, scale, signed, seed, dc=(0.0, 0.0), nav=None):
    """A small 8-bit complex capture made with numpy (gpsacq_generate_iq8_range's law, its own noise): sats = [(prn, amplitude,
    doppler, code_phase, carrier_phase)], dc added before rounding.  Returns interleaved int8 / uint8."""
    rng = np.random.default_rng(seed)
    m = np.arange(n, dtype=np.float64)
    y = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for k, (prn, amp, dop, cp, ph) in enumerate(sats):
        q = np.floor((m + cp) * CPS * (1 + dop / L1) / fs).astype(np.int64)
        s = amp * chips_pm1(prn)[q % 1023] * np.exp(2j * np.pi * ((if_hz + dop) / fs * m + ph))
        if nav is not None:
            s = s * np.asarray(nav[k])[(q // 20460) % len(nav[k])]
        y = y + s
    v = np.clip(np.rint(scale * y.real + dc[0]), -127, 127), np.clip(np.rint(scale * y.imag + dc[1]), -127, 127)
    out = np.empty(2 * n, np.int16)
    out[0::2], out[1::2] = v[0], v[1]
    return out.astype(np.int8) if signed else (out + 128).astype(np.uint8)
