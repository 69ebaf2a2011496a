"""An independent reference of the synthetic capture generators (gpsacq_generate*, gpsacq_generate_iq8_range*), written in numpy
float64 and Python integers from the text "THE GENERATOR'S LAW" in include/gpsacq.h alone.  It shares nothing with csrc/: the
chips come from the oracle's C/A generator (track_ref.chips), the hash is computed in uint64, the uniforms are built as float32
values and carried in float64, ln / cos / sin are numpy's float64 ones.

Large sample indices cost nothing: for samples m0 + j the code position (m + code_phase) * chips_per_sample and the carrier phase
cycles_per_sample * m + theta are split into their value at m0, computed exactly with fractions.Fraction from the *double* values
of the two rates (the host's IEEE expressions of the law, one operation per line in Python floats), and j * rate with j < 2^20,
computed in float64 from a 30-bit head of the rate (j * head is exact) and its tail (j * tail is exact and below 2^-10).

The functions never return bits alone.  bits() returns the decision value y_ref[m] of the 1-bit stream, iq8() returns
v_ref = scale * y_ref per arm, both with a margin per sample and a mask of samples to leave out:

  tau[m] = noise_sigma * 2^-10                      room for __logf, __cosf, __sinf and fp32 Box-Muller (fixed, not tuned)
         + sum |a_k| * 2^-20                        the fp32 sum and cospif
         + sum |a_k| * 2 pi * (2^-23 + 2^-51 * max(1, |cycles_per_sample * m| + |theta|))
                                                    the float cast of the phase (a last-bit difference of the double can move it
                                                    by one float ulp) and the fp64 evaluation of the phase, fused or not
  skip[m]: for some satellite the exact code position lies within 2^-50 * max(1, |position|) of an integer: the fp64 product
           of the law may floor to either side there, so the chip could legitimately differ.

Law is a class so that tests/test_gen_ref.py can derive wrong laws from it, one method each, and show that the case table of
tests/gen_cases.py tells them from the right one."""
import math
from fractions import Fraction

import numpy as np

import track_ref

L1, CPS = 1575.42e6, 1.023e6
CHIPS, NAV_CHIPS = 1023, 20460
GOLDEN = 0x9E3779B97F4A7C15
MAX_SAMPLES = 1 << 20
_M64 = (1 << 64) - 1


def _u64(v):
    return np.uint64(int(v) & _M64)


def mix64(z):
    """the splitmix64 finaliser on a uint64 array (numpy wraps modulo 2^64)"""
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def affine(base, rate, n):
    """(floor, fractional part in [0, 1]) of base + j * rate for j = 0 .. n - 1.  base is a Fraction and enters exactly; rate is a
    double with |rate| < 4.  The result is good to about 2^-52 whatever the size of base."""
    assert n <= MAX_SAMPLES and abs(rate) < 4.0
    b0 = math.floor(base)
    f0 = float(base - b0)
    j = np.arange(n, dtype=np.float64)
    head = float(np.rint(rate * 2.0 ** 30)) / 2.0 ** 30   # at most 32 bits: j * head has at most 52
    tail = rate - head                                    # exact, below 2^-31 and no longer than 32 bits: j * tail is exact
    a = j * head
    ai = np.floor(a)
    g = (a - ai) + (f0 + j * tail)
    gi = np.floor(g)
    return b0 + ai.astype(np.int64) + gi.astype(np.int64), g - gi


def cos_sin_2pi(x):
    """cos and sin of 2 pi x for x in [0, 1] (float64), exact at the quarter points like cospif / sincospif"""
    c, s = np.cos(2.0 * np.pi * x), np.sin(2.0 * np.pi * x)
    c = np.where((x == 0.25) | (x == 0.75), 0.0, c)
    s = np.where((x == 0.0) | (x == 0.5) | (x == 1.0), 0.0, s)
    return c, s


class Law:
    """The generator's law.  Every method restates one sentence of the header; a mutant overrides one of them."""
    clamp_lo, clamp_hi = -127.0, 127.0

    # ---- the host's two rates: IEEE doubles, one operation per line -------------------------------------------------------------
    def chips_per_sample(self, doppler, fs):
        r = doppler / L1
        r = 1.0 + r
        r = CPS * r
        return r / fs

    def cycles_per_sample(self, f_carrier, doppler, fs):
        r = f_carrier + doppler
        return r / fs

    # ---- noise --------------------------------------------------------------------------------------------------------------
    def sample_index(self, m):
        """the absolute sample index, all 64 bits of it"""
        return m

    def noise(self, seed, m):
        """(n_I, n_Q) of samples m (uint64 array)"""
        h = mix64(_u64(seed) ^ (m * _u64(GOLDEN)))
        one, two_m32 = np.float32(1.0), np.float32(2.0 ** -32)
        u1 = (((h >> np.uint64(32)).astype(np.float32) + one) * two_m32).astype(np.float64)   # (0, 1]
        u2 = ((h & _u64(0xFFFFFFFF)).astype(np.float32) * two_m32).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u1))
        return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)

    def noise_1bit(self, n_i, n_q):
        return n_i

    # ---- code ---------------------------------------------------------------------------------------------------------------
    def chip_count(self, q_floor):
        """q = floor(position), also below zero"""
        return q_floor

    def chip_index(self, q):
        return np.mod(q, CHIPS)            # numpy's mod of integers is the true modulo

    def nav_index(self, q, n_nav):
        return np.mod(np.floor_divide(q, NAV_CHIPS), n_nav)

    # ---- carrier ------------------------------------------------------------------------------------------------------------
    def theta(self, carrier_phase_cycles):
        return carrier_phase_cycles

    def q_arm(self, sin):
        return sin

    # ---- 8-bit value --------------------------------------------------------------------------------------------------------
    def round(self, v):
        return np.rint(v)                  # ties to even

    def quantise(self, v, signed):
        """the bytes of decision values v = scale * y: int8, or uint8 = int8 + 128"""
        q = np.clip(self.round(v), self.clamp_lo, self.clamp_hi).astype(np.int16)
        return q.astype(np.int8) if signed else (q + 128).astype(np.uint8)

    # ---- the sum ------------------------------------------------------------------------------------------------------------
    def signal(self, f_carrier, fs, sats, first, n, nav):
        """(I, Q, skip, phase part of tau, chips [n_sats][n], q [n_sats][n]) of the noise-free sum over the satellites"""
        m = self.sample_index(np.uint64(first) + np.arange(n, dtype=np.uint64))
        parts = [self._run(f_carrier, fs, sats, int(m[a]), b - a, nav) for a, b in _runs(m)]   # one run, unless a wrong law wraps m
        return tuple(np.concatenate([p[k] for p in parts], axis=-1) for k in range(6))

    def _run(self, f_carrier, fs, sats, m0, n, nav):
        """signal() of the consecutive samples m0 .. m0 + n - 1"""
        yi, yq, tau3 = np.zeros(n), np.zeros(n), np.zeros(n)
        skip = np.zeros(n, bool)
        chips, qs = np.zeros((len(sats), n), np.int8), np.zeros((len(sats), n), np.int64)
        nv = None if nav is None else np.asarray(nav, np.int8).reshape(len(sats), -1)
        j = np.arange(n, dtype=np.float64)
        for s, (prn, amp, doppler, code_phase, phase) in enumerate(sats):
            amp = float(np.float32(amp))
            cps, cyc = self.chips_per_sample(float(doppler), fs), self.cycles_per_sample(f_carrier, float(doppler), fs)
            th = float(self.theta(float(phase)))
            q, frac = affine((m0 + Fraction(float(code_phase))) * Fraction(cps), cps, n)
            skip |= np.minimum(frac, 1.0 - frac) <= 2.0 ** -50 * np.maximum(1.0, np.abs(q.astype(np.float64)))
            q = self.chip_count(q)
            chip = 1 - 2 * track_ref.chips(int(prn))[self.chip_index(q)].astype(np.int8)
            if nv is not None:
                chip = chip * nv[s][self.nav_index(q, nv.shape[1])]
            _, ph = affine(Fraction(cyc) * m0 + Fraction(th), cyc, n)
            c, sn = cos_sin_2pi(ph.astype(np.float32).astype(np.float64))   # reduced to [0, 1), cast to float
            yi += amp * chip * c
            yq += amp * chip * self.q_arm(sn)
            tau3 += abs(amp) * 2.0 * np.pi * (2.0 ** -23 + 2.0 ** -51 * np.maximum(1.0, np.abs(cyc * (m0 + j)) + abs(th)))
            chips[s], qs[s] = chip, q
        return yi, yq, skip, tau3, chips, qs

    def tau(self, sats, sigma, tau3):
        a = sum(abs(float(np.float32(s[1]))) for s in sats)
        return float(np.float32(sigma)) * 2.0 ** -10 + a * 2.0 ** -20 + tau3

    def bits(self, fc, fs, sats, sigma, seed, first, n, nav=None):
        """The 1-bit stream, samples first .. first + n - 1: dict(y, tau, skip, chips, q).  bit = (y < 0), a sum of +-0 is bit 0."""
        yi, _, skip, tau3, chips, q = self.signal(fc, fs, sats, first, n, nav)
        n_i, n_q = self.noise(seed, self.sample_index(np.uint64(first) + np.arange(n, dtype=np.uint64)))
        y = float(np.float32(sigma)) * self.noise_1bit(n_i, n_q) + yi
        return dict(y=y, tau=self.tau(sats, sigma, tau3), skip=skip, chips=chips, q=q)

    def iq8(self, fs, sats, if_hz, scale, sigma, seed, first, n, nav=None):
        """The 8-bit stream: dict(v [n][2] = scale * y per arm, margin [n] = scale * tau, skip, chips, q)"""
        yi, yq, skip, tau3, chips, q = self.signal(if_hz, fs, sats, first, n, nav)
        n_i, n_q = self.noise(seed, self.sample_index(np.uint64(first) + np.arange(n, dtype=np.uint64)))
        sg, sc = float(np.float32(sigma)), float(np.float32(scale))
        v = sc * np.stack([sg * n_i + yi, sg * n_q + yq], axis=1)
        return dict(v=v, margin=sc * self.tau(sats, sigma, tau3), skip=skip, chips=chips, q=q)


def _runs(m):
    """[(a, b)] such that m[a:b] are consecutive sample indices"""
    cut = np.flatnonzero(np.diff(m.astype(np.int64)) != 1) + 1
    edges = [0, *cut.tolist(), len(m)]
    return list(zip(edges[:-1], edges[1:]))


LAW = Law()


def unpack(bits):
    """samples of packed bytes: sample m in bit m % 8 of byte m / 8"""
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")
