"""iq_ref.py -- an independent reference of the 8-bit IQ -> 1-bit conversion, written from include/gpsacq.h (the gpsacq_iq8_*
section: formats, `y - mean(y)` over the whole capture from exact integer sums, real(y exp(2 pi i mix_hz n / fs)), bit = 1 where
the value is <= 0, sample n in bit n % 8 of byte n / 8, bits beyond total_samples read 0) and the two script lines it cites:

    proc_rtl_bin_for_gps.m:41     real(y.' .* exp(1i.*2.*pi.*fc.*(0:n-1).*(1./2.8e6)))
    proc_hackrf_bin_for_gps.m:15  real(y.' .* exp(1i.*(0:n-1).*2.6e6.*2.*pi./10e6))

MATLAB evaluates a chain of .* and ./ left to right in double, and a real factor times a purely imaginary number rounds like the
real product, so the phase is (((2 pi) fc) n) (1 / fs) for the unsigned format and (((n fc) 2) pi) / fs for the signed one;
real((a + bi)(c + si)) = a c - b s with the two products rounded separately.  numpy float64 and Python integers only; nothing
here is taken from the device code or from oracle/iq8_oracle.py (tests/test_iq_ref.py compares the two).

A sample whose value is within 1e-9 of zero has no certain sign: two correct double evaluations differ only through their sincos,
each within a couple of ulp, so by at most about 8 2^-53 (|yi| + |yq|) < 5e-13 for bytes; 1e-9 leaves a factor of 1000 over that.
decided() marks the others, and those whose value is exact or a single product by structure.  The limit is a condition for
leaving a sample out of a comparison, not a tolerance on anything.

The builders below make captures, seeded, in both formats, on which a conversion can go wrong: every byte pair at many phases,
pairs chosen per sample index to put the value next to zero or next to 5e-3 (where the device takes its double-precision path),
fc = fs / 4 with one arm zero (the value is one product with the rounding residue of the phase), and the byte rails.
"""
import functools

import numpy as np

DECIDED = 1e-9      # |r| above this: the sign is certain
THRESHOLD = 5e-3    # the device's fast / slow limit on |r| (csrc/iq_convert.hpp); only the builders and the reports use it
BIG = 2 ** 33 + 12345


# ---- the conversion --------------------------------------------------------------------------------------------------------------
def levels(raw, signed):
    """interleaved bytes -> (I, Q) as int64 sample values: int8 as it is, uint8 less 128"""
    b = np.ascontiguousarray(np.asarray(raw)).view(np.uint8).ravel()
    v = b.view(np.int8).astype(np.int64) if signed else b.astype(np.int64) - 128
    return v[0::2], v[1::2]


def encode(vi, vq, signed):
    """sample values in [-128, 127] -> interleaved bytes (uint8 array)"""
    v = np.empty(2 * len(vi), np.int64)
    v[0::2], v[1::2] = vi, vq
    assert v.min() >= -128 and v.max() <= 127
    return v.astype(np.int8).view(np.uint8) if signed else (v + 128).astype(np.uint8)


def sums(raw, signed):
    vi, vq = levels(raw, signed)
    return int(vi.sum()), int(vq.sum())


def means(raw, signed):
    """the exact integer sums divided once by the count (Python's int / int is correctly rounded)"""
    si, sq = sums(raw, signed)
    n = np.asarray(raw).size // 2
    return si / n, sq / n


def index(first, count):
    """capture indices first .. first + count - 1 as doubles (exact below 2^53)"""
    assert first + count < 2 ** 53
    return (np.arange(count, dtype=np.uint64) + np.uint64(first)).astype(np.float64)


def theta(n, fc, fs, signed):
    n = np.asarray(n, dtype=np.float64)
    if signed:
        return (((n * fc) * 2.0) * np.pi) / fs
    return (((2.0 * np.pi) * fc) * n) * (1.0 / fs)


def _arms(raw, signed, mean):
    vi, vq = levels(raw, signed)
    mi, mq = means(raw, signed) if mean is None else mean
    return vi.astype(np.float64) - float(mi), vq.astype(np.float64) - float(mq)


def value(raw, signed=False, mean=None, mix_hz=0.0, fs=2.8e6, first=0):
    """r of every sample.  mean: (mean_i, mean_q) as given, or None for this buffer's own; (0, 0) is `remove_dc` off."""
    yi, yq = _arms(raw, signed, mean)
    if mix_hz == 0.0:
        return yi
    th = theta(index(first, yi.size), mix_hz, fs, signed)
    return yi * np.cos(th) - yq * np.sin(th)


def bits(raw, signed=False, mean=None, mix_hz=0.0, fs=2.8e6, first=0, total=None):
    r = value(raw, signed, mean, mix_hz, fs, first)
    b = np.where(r > 0, 0, 1).astype(np.uint8)
    if total is not None and total < first + b.size:
        b[max(0, total - first):] = 0
    return np.packbits(b, bitorder="little")


def decided(raw, signed=False, mean=None, mix_hz=0.0, fs=2.8e6, first=0):
    yi, yq = _arms(raw, signed, mean)
    if mix_hz == 0.0:
        return np.ones(yi.size, bool)
    r = value(raw, signed, mean, mix_hz, fs, first)
    return (np.abs(r) > DECIDED) | (yi == 0) | (yq == 0)  # one arm zero: a single product; both: exactly zero


def unpack(packed, n):
    return np.unpackbits(np.asarray(packed, np.uint8), bitorder="little")[:n]


class Capture:
    """bytes plus how they are to be converted.  mean None: the converter derives it (remove_dc on, this buffer is the whole
    capture); remove_dc False: no mean; else the explicit mean of a longer capture this buffer is a piece of."""

    def __init__(self, name, raw, signed, mix_hz, fs, mean=None, remove_dc=True, first=0, total=None):
        self.name, self.raw, self.signed, self.mix_hz, self.fs = name, np.ascontiguousarray(raw, dtype=np.uint8), bool(signed), float(mix_hz), float(fs)
        self.remove_dc, self.first = bool(remove_dc), int(first)
        self.mean = (0.0, 0.0) if not remove_dc else mean
        self.n = self.raw.size // 2
        self.total = self.first + self.n if total is None else int(total)

    def _args(self):
        return self.raw, self.signed, self.mean, self.mix_hz, self.fs, self.first

    def mean_used(self):
        return means(self.raw, self.signed) if self.mean is None else self.mean

    def value(self):
        return value(*self._args())

    def bits(self):
        return bits(*self._args(), total=self.total)

    def decided(self):
        d = decided(*self._args())
        d[max(0, self.total - self.first):] = True  # past the capture's end the bit is 0 whatever the bytes
        return d

    def report(self):
        """(samples, undecided, within 1e-3 of the fast / slow threshold)"""
        r = np.abs(self.value()[:max(0, self.total - self.first)])
        return self.n, int(np.count_nonzero(~self.decided())), int(np.count_nonzero(np.abs(r - THRESHOLD) < 1e-3)) if self.mix_hz else 0

    def line(self):
        n, und, thr = self.report()
        return f"{self.name}: {n} samples, {und} undecided, {thr} within 1e-3 of the threshold"


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _fmt(signed):
    return "s8" if signed else "u8"


def exhaustive(signed, mix_hz, fs, remove_dc=True, reps=16, seed=1):
    """all 65 536 (I, Q) byte pairs `reps` times over, each time in another seeded order: every pair meets `reps` phases.  Each
    value occurs equally often, so the mean is (-0.5, -0.5) exactly."""
    rng = np.random.default_rng([seed, signed, reps])
    p = np.concatenate([rng.permutation(65536) for _ in range(reps)])
    raw = np.empty(2 * p.size, np.uint8)
    raw[0::2], raw[1::2] = p & 0xff, p >> 8
    return Capture(f"exhaustive {_fmt(signed)} dc={int(remove_dc)} {mix_hz / 1e6:g}@{fs / 1e6:g}", raw, signed, mix_hz, fs, remove_dc=remove_dc)


def _filler(have, want, count):
    """`count` values in [-128, 127] that bring a sum from `have` to `want`"""
    base, rem = divmod(want - have, count)
    v = np.full(count, base, np.int64)
    v[:rem] += 1
    assert v.min() >= -128 and v.max() <= 127, (have, want, count)
    return v


def adversarial(signed, mix_hz, fs, n, mean, first=0, target=0.0, seed=1, n_i=128, filler=0):
    """Sample first + j gets, among n_i seeded values of I and for each the two Q next to the real q* that solves
    yi cos(theta) - (q* - mean_q) sin(theta) = +-target, the pair whose |r| is closest to target (a number or one per sample):
    0 puts the value next to zero, THRESHOLD next to the limit of the device's fast path.
    filler > 0: for a converter that derives its own mean.  The mean becomes round(mean (n + filler)) / (n + filler), the pairs are
    chosen for THAT mean, and `filler` samples are appended that complete the integer sums to it exactly."""
    rng = np.random.default_rng([seed, signed, n, first % (2 ** 32)])
    count = n + filler
    want = (round(mean[0] * count), round(mean[1] * count))
    mi, mq = (want[0] / count, want[1] / count) if filler else (float(mean[0]), float(mean[1]))
    th = theta(index(first, n), mix_hz, fs, signed)
    cs, sn = np.cos(th), np.sin(th)
    tgt = np.broadcast_to(np.asarray(target, np.float64), (n,))
    t = tgt * rng.choice([-1.0, 1.0], n)
    best = np.full(n, np.inf)
    bi, bq = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for _ in range(n_i):
        vi = rng.integers(-128, 128, n)
        a = (vi - mi) * cs
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = mq + (a - t) / sn
        q0 = np.clip(np.floor(np.where(np.isfinite(q), q, 0.0)), -128, 126).astype(np.int64)
        for vq in (q0, q0 + 1):
            err = np.abs(np.abs(a - (vq - mq) * sn) - tgt)
            take = err < best
            best[take], bi[take], bq[take] = err[take], vi[take], vq[take]
    if filler:
        bi = np.concatenate([bi, _filler(int(bi.sum()), want[0], filler)])
        bq = np.concatenate([bq, _filler(int(bq.sum()), want[1], filler)])
    raw = encode(bi, bq, signed)
    kind = "zero" if np.all(tgt == 0) else "threshold" if np.all(tgt == THRESHOLD) else "zero+threshold"
    cap = Capture(f"adversarial {kind} {_fmt(signed)} {mix_hz / 1e6:g}@{fs / 1e6:g} n0={first}", raw, signed, mix_hz, fs,
                  mean=None if filler else (mi, mq), first=first)
    if filler:
        assert sums(raw, signed) == want and cap.mean_used() == (mi, mq)
    return cap


def quarter_rate(signed, fs, n, mean=(0, 0), seed=1, filler=512):
    """fc = fs / 4 and an integer mean: a third of the samples have yi = 0, a third yq = 0, a few both, so r is one product -- with
    a cosine or sine that is only the rounding residue of its argument on every other sample -- or exactly zero.  mean (0, 0):
    remove_dc off.  Otherwise `filler` samples complete the sums to mean x count, and the converter derives that mean."""
    rng = np.random.default_rng([seed, signed, n])
    dc = tuple(mean) != (0, 0)
    m = n - filler if dc else n
    kind = rng.integers(0, 10, m)
    vi = rng.integers(-100, 101, m)
    vq = rng.integers(-100, 101, m)
    vi[(kind < 3) | (kind == 9)] = mean[0]
    vq[((kind >= 3) & (kind < 6)) | (kind == 9)] = mean[1]
    if dc:
        vi = np.concatenate([vi, _filler(int(vi.sum()), mean[0] * n, filler)])
        vq = np.concatenate([vq, _filler(int(vq.sum()), mean[1] * n, filler)])
    raw = encode(vi, vq, signed)
    cap = Capture(f"quarter_rate {_fmt(signed)} mean={tuple(mean)} fs={fs / 1e6:g}", raw, signed, fs / 4, fs, remove_dc=dc)
    if dc:
        assert sums(raw, signed) == (mean[0] * n, mean[1] * n) and cap.mean_used() == (float(mean[0]), float(mean[1]))
    return cap


_RAIL_COUNTS = {  # per 510 samples, of the values (-128, -1, 0, 127): bytes 0x00 0x7F 0x80 0xFF (uint8), 0x80 0xFF 0x00 0x7F (int8)
    "low": (509, 0, 0, 1),       # mean -127.5
    "mid": (128, 126, 126, 130),  # mean 0
    "high": (1, 0, 0, 509),      # mean 126.5 (no capture has a mean above 127)
}
_RAIL_MEAN = {"low": -127.5, "mid": 0.0, "high": 126.5}


def rails(signed, mix_hz, fs, kind_i, kind_q, reps=16, seed=1):
    """only the four rail bytes, in proportions that make the derived mean -127.5, 0 or 126.5 exactly, I and Q shuffled apart"""
    rng = np.random.default_rng([seed, signed, reps])
    arm = lambda k: rng.permutation(np.repeat(np.array([-128, -1, 0, 127]), np.array(_RAIL_COUNTS[k]) * reps))
    raw = encode(arm(kind_i), arm(kind_q), signed)
    cap = Capture(f"rails {_fmt(signed)} {kind_i}/{kind_q} {mix_hz / 1e6:g}@{fs / 1e6:g}", raw, signed, mix_hz, fs)
    assert cap.mean_used() == (_RAIL_MEAN[kind_i], _RAIL_MEAN[kind_q])
    return cap


def rails_explicit(signed, mix_hz, fs, mean, n=4096, first=0, seed=1):
    """the four rail bytes uniformly, converted with a mean handed in (a piece of a longer capture): +-127.5 puts |y| at 255.5"""
    rng = np.random.default_rng([seed, signed, n])
    v = np.array([-128, -1, 0, 127])
    raw = encode(v[rng.integers(0, 4, n)], v[rng.integers(0, 4, n)], signed)
    return Capture(f"rails {_fmt(signed)} mean={tuple(mean)} {mix_hz / 1e6:g}@{fs / 1e6:g} n0={first}", raw, signed, mix_hz, fs, mean=tuple(mean), first=first)


def random_bytes(signed, mix_hz, fs, n, remove_dc=True, seed=1):
    rng = np.random.default_rng([seed, signed, n])
    return Capture(f"random {_fmt(signed)} n={n}", rng.integers(0, 256, 2 * n, dtype=np.uint8), signed, mix_hz, fs, remove_dc=remove_dc)


# ---- the cases both test files use (built once per process; nobody writes to them) -------------------------------------------------
RTL = (0.6180339887e6, 2.8e6)     # mixers whose fc / fs is no small rational, next to the scripts' 0.62e6 @ 2.8e6 and 2.6e6 @ 10e6
HACKRF = (2.6180339887e6, 10e6)
LENGTHS = (1, 7, 8, 9, 15, 17, 4099, 16375, 16376, 16377, 16383, 16384, 16385)  # 2047, 2048, 2049 output bytes: eight workgroups +- 1


N_STANDALONE = 60


def _both(n):
    return np.where(np.arange(n) % 2, THRESHOLD, 0.0)


@functools.lru_cache(maxsize=None)
def standalone_cases():
    """what tests/test_gpu_iq_edges.py hands to the stand-alone converter (it starts at sample 0 and derives its mean)"""
    out = []
    for signed in (False, True):
        for mix in ((0.0, 2.8e6), (0.62e6, 2.8e6), (2.6e6, 10e6)):
            for dc in (True, False):
                out.append(exhaustive(signed, *mix, remove_dc=dc))
        for mix, mean in ((RTL, (0.3721, -0.6183)), (HACKRF, (-1.4142, 0.5772))):
            for tgt in (0.0, THRESHOLD):
                out.append(adversarial(signed, *mix, 65536 - 4096, mean, target=tgt, filler=4096))
        for mean in ((0, 0), (3, -2)):
            out.append(quarter_rate(signed, 2.8e6, 16384 + 5, mean))
        out.append(quarter_rate(signed, 10e6, 16384 + 5, (0, 0), seed=2))
        for ki, kq in (("low", "high"), ("mid", "mid"), ("high", "low"), ("mid", "low")):
            out.append(rails(signed, *(HACKRF if signed else RTL), ki, kq))
        for n in LENGTHS:
            out.append(random_bytes(signed, *(HACKRF if signed else RTL), n, remove_dc=n % 2 == 1))
    return out


@functools.lru_cache(maxsize=None)
def search_cases():
    """three blocks of 40 960 samples each for the fused search: nothing can be masked there, so no sample may be undecided"""
    n = 3 * 40960
    a = adversarial(False, *RTL, n, (0.3721, -0.6183), first=0, target=_both(n), seed=11)
    b = adversarial(True, *HACKRF, n, (-1.4142, 0.5772), first=BIG, target=_both(n), seed=12)
    c = adversarial(False, *RTL, n, (-0.2915, 0.7071), first=BIG, target=_both(n), seed=13)
    c.total = BIG + 2 * 40960 + 23459  # the capture ends inside the last block, off the byte grid
    c.name += " ragged"
    d = adversarial(False, *RTL, n, (0.3721, -0.6183), first=2 ** 40 + 12345, target=_both(n), seed=14)  # the phase's ulp is 2.4e-4 there
    return [a, b, c, d]


@functools.lru_cache(maxsize=None)
def track_case():
    """30 ms at 2.8 MHz from capture sample 2^33 + 12345 on, ending inside a byte"""
    n = 84000 - 3
    return adversarial(False, *RTL, n, (0.3721, -0.6183), first=BIG, target=_both(n), seed=21)
