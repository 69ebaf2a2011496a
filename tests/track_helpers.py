"""Helpers of the tracking / NAV tests: the CPU model of a channel (tests/c/track_model.c, compiled with gcc on first use),
the C/A chip words it reads, and an encoder of parity-valid NAV subframes (IS-GPS-200 Table 20-XIV)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_model = None


def chip_words(prn):
    """The 1023 chips of PRN `prn` (1..32) as 32 uint32 words, chip i in bit i % 32 of word i / 32 (from the oracle's generator)."""
    from oracle_lib import lib, _p
    c = np.zeros(1023, np.uint8)
    lib("f64").oracle_ca_chips(prn - 1, _p(c))
    bits = np.zeros(1024, np.uint8)
    bits[:1023] = c
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def model_lib():
    global _model
    if _model is None:
        out = os.path.join(tempfile.mkdtemp(prefix="track_model_"), "libtrack_model.so")
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "track_model.c"), "-o", out])
        lib = ctypes.CDLL(out)
        vp = ctypes.c_void_p
        lib.track_model.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, vp, vp, vp, vp, vp, ctypes.c_int]
        lib.track_model.restype = ctypes.c_int
        _model = lib
    return _model


def run_model(bits, first_sample, chans, params, max_epochs):
    """The CPU model over a window: chans (TRACK_CHAN_DTYPE) updated in place; returns (prompt, records, n_epochs) shaped like
    Engine.track(..., records=True)."""
    import gpsacq
    lib = model_lib()
    buf = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8))
    n = chans.size
    prompt = np.zeros((n, max_epochs, 2), np.int32)
    rec = np.zeros((n, max_epochs), gpsacq.TRACK_RECORD_DTYPE)
    ne = np.zeros(n, np.int32)
    for c in range(n):
        ch = chans[c:c + 1].copy()
        w = chip_words(int(ch["prn"][0]))
        ne[c] = lib.track_model(buf.ctypes.data, buf.size, int(first_sample), ch.ctypes.data, ctypes.addressof(params), w.ctypes.data,
                                prompt[c].ctypes.data, rec[c].ctypes.data, int(max_epochs))
        chans[c] = ch[0]
    return prompt, rec, ne


# ---- NAV subframes ----------------------------------------------------------------------------------------------------
PREAMBLE = 0x8B
_PARITY = [(29, [1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23]), (30, [2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24]),
           (29, [1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22]), (30, [2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23]),
           (30, [1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24]), (29, [3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24])]


def encode_word(data24, d29, d30):
    """30 transmitted bits of one word: D_k = d_k ^ D30*, then the six parity bits."""
    d = [(data24 >> (23 - i)) & 1 for i in range(24)]
    out = [b ^ d30 for b in d]
    for star, idx in _PARITY:
        v = d29 if star == 29 else d30
        for i in idx:
            v ^= d[i - 1]
        out.append(v)
    return out


def encode_subframe(words, d29=0, d30=0):
    """300 bits of ten 24-bit data words; words 2 and 10 get the two trailing data bits that make D29 = D30 = 0
    (IS-GPS-200 20.3.5.2), so the next subframe's preamble is upright.  Returns (bits, D29, D30 of the last word)."""
    bits = []
    for w, data in enumerate(words):
        if w in (1, 9):  # solve t1 t2 (bits 23, 24) so that D29 = D30 = 0
            for t in range(4):
                cand = (data & ~3) | t
                enc = encode_word(cand, d29, d30)
                if enc[28] == 0 and enc[29] == 0:
                    data = cand
                    break
        enc = encode_word(data, d29, d30)
        bits += enc
        d29, d30 = enc[28], enc[29]
    return bits, d29, d30


def make_subframe_words(tow, sf_id, rng):
    """Ten data words: TLM (preamble), HOW with TOW count and subframe ID, random payload."""
    words = [int(x) for x in rng.integers(0, 1 << 24, size=10)]
    words[0] = (PREAMBLE << 16) | (words[0] & 0xFFFF)
    words[1] = ((tow & 0x1FFFF) << 7) | (words[1] & 0x60) | ((sf_id & 7) << 2)
    return words


def nav_stream(tow0, n_subframes, seed=1):
    """Consecutive subframes with TOW tow0, tow0 + 1, ... and IDs cycling 1..5.  Returns (0/1 bits, [(id, tow), ...])."""
    rng = np.random.default_rng(seed)
    bits, d29, d30, meta = [], 0, 0, []
    for k in range(n_subframes):
        tow = tow0 + k
        sf_id = k % 5 + 1
        b, d29, d30 = encode_subframe(make_subframe_words(tow, sf_id, rng), d29, d30)
        bits += b
        meta.append((sf_id, tow))
    return np.array(bits, np.uint8), meta
