"""tests/iq_ref.py, the independent reference of the 8-bit IQ -> 1-bit conversion, checked on the CPU before the GPU suite
(tests/test_gpu_iq_edges.py) leans on it:

  - against oracle/iq8_oracle.py (written from the scripts alone, its mean from numpy's pairwise mean()) on every decided sample of
    every capture the stand-alone converter is given;
  - against the same expression in mpmath at 40 digits -- the phase as the double the script's operation order gives, its cosine
    and sine, the two products and their difference exact to 40 digits -- on the adversarial and quarter-rate captures: the sign is
    the reference's on every decided sample, and the double value is within 5e-13 (iq_ref's own bound on two correct evaluations);
  - the share of samples whose sign is not certain (|r| <= 1e-9 and not exact by structure) is at most 1e-5 in every capture, and
    zero in the captures of the fused-search and tracking comparisons, where nothing can be masked;
  - gpsacq_iq8_accumulate_power (host arithmetic) against Python integers on the rails and on lengths 1 .. 17.

Measured here: no capture has an undecided sample; largest |r_double - r_40| 7.2e-14 over some 49 000 samples (the rails at a
mean of +-127.5 and n = 2^40; 2.2e-14 elsewhere).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import iq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def test_theta_is_the_scripts_order():
    """hand cases: the two orders differ in the last place now and then, and n = 0 is exact"""
    n = np.array([0.0, 1.0, 3.0, 2.0 ** 40 + 1])
    a, b = iq_ref.theta(n, 0.62e6, 2.8e6, False), iq_ref.theta(n, 0.62e6, 2.8e6, True)
    assert a[0] == 0 and b[0] == 0
    assert a[1] == ((2.0 * np.pi) * 0.62e6) * (1.0 / 2.8e6) and b[1] == ((0.62e6 * 2.0) * np.pi) / 2.8e6
    assert np.all(np.abs(a - b) <= 2 * np.spacing(a))
    many = np.arange(100000.0)
    assert 0 < np.count_nonzero(iq_ref.theta(many, 0.62e6, 2.8e6, False) != iq_ref.theta(many, 0.62e6, 2.8e6, True)) < many.size


def test_small_cases_by_hand():
    raw = np.array([130, 9, 126, 9, 128, 9, 128, 9], np.uint8)  # I - 128 = 2, -2, 0, 0: mean 0; r = 0 gives 1
    assert iq_ref.bits(raw, False, None)[0] == 0b1110 and iq_ref.bits(raw, False, (0.0, 0.0))[0] == 0b1110
    raw = np.array([133, 0, 131, 0, 133, 0, 131, 0], np.uint8)  # 5, 3, 5, 3: mean 4
    assert iq_ref.bits(raw, False, (0.0, 0.0))[0] == 0 and iq_ref.bits(raw, False, None)[0] == 0b1010
    iq = np.array([10, 3] * 4, np.int8)  # fs / 4: real((I + jQ) e^{j pi n / 2}) = I, -Q, -I, Q
    assert iq_ref.bits(iq, True, (0.0, 0.0), 0.25, 1.0)[0] == 0b0110
    raw = np.full(22, 128, np.uint8)
    raw[18] = 200
    out = iq_ref.bits(raw, False, (0.0, 0.0))
    assert out.size == 2 and out[0] == 0xFF and out[1] == 0b101  # LSB first, tail bits zero
    assert iq_ref.bits(raw, False, (0.0, 0.0), first=40, total=44)[0] == 0x0F and iq_ref.bits(raw, False, (0.0, 0.0), first=40, total=40)[1] == 0
    assert iq_ref.means(np.array([0, 255, 1, 255, 1, 254], np.uint8), False) == (-382 / 3, 380 / 3)
    d = iq_ref.decided(np.array([128, 128, 128, 9, 9, 128, 9, 9], np.uint8), False, (0.0, 0.0), 0.25, 1.0)
    assert d.all()  # zero, two single products, and an ordinary sample
    assert not iq_ref.decided(np.array([1, 1], np.int8), True, (0.0, 0.0), 0.125, 1.0, first=1)[0]  # cos(pi / 4) - sin(pi / 4)


@pytest.mark.parametrize("k", range(iq_ref.N_STANDALONE))  # (by number: the captures are built when the first test runs, not on collection)
def test_reference_equals_the_numpy_oracle_on_decided_samples(k):
    from iq8_oracle import iq8_to_bits
    assert len(iq_ref.standalone_cases()) == iq_ref.N_STANDALONE
    cap = iq_ref.standalone_cases()[k]
    want = iq8_to_bits(cap.raw, signed=cap.signed, remove_dc=cap.remove_dc, mix_hz=cap.mix_hz, fs=cap.fs)
    got = cap.bits()
    assert got.size == want.size == (cap.n + 7) // 8
    dec = cap.decided()
    n, und, thr = cap.report()
    print(cap.line())
    assert und <= 1e-5 * n
    assert not ((iq_ref.unpack(got, n) != iq_ref.unpack(want, n)) & dec).any()
    if "adversarial threshold" in cap.name:
        assert thr >= 100
    if "adversarial zero" in cap.name:
        assert np.count_nonzero(np.abs(cap.value()) < 1e-4) >= 100  # far inside the band where the device must fall back to double


def test_no_undecided_sample_where_nothing_can_be_masked():
    for cap in iq_ref.search_cases() + [iq_ref.track_case()]:
        n, und, thr = cap.report()
        print(cap.line())
        assert und == 0 and thr >= 100 and cap.decided().all()
        assert np.count_nonzero(np.abs(cap.value()) < 1e-4) >= 100
        assert cap.first % 8 != 0 or cap.first == 0
    assert iq_ref.search_cases()[2].total % 8 != 0 and 2 * 40960 < iq_ref.search_cases()[2].total - iq_ref.BIG < 2 * 40960 + 40000


@functools.lru_cache(maxsize=None)
def _mp_cases():
    s = [c for c in iq_ref.standalone_cases() if c.name.startswith(("adversarial", "quarter_rate"))]
    e = [iq_ref.rails_explicit(sg, *mix, mean, first=first) for sg, mix, first in ((False, iq_ref.RTL, 2 ** 40), (True, iq_ref.HACKRF, iq_ref.BIG))
         for mean in ((127.5, -127.5), (-127.5, 127.5), (0.0, 0.0))]
    return s + iq_ref.search_cases() + [iq_ref.track_case()] + e


N_MP = 25


@pytest.mark.parametrize("k", range(N_MP))
def test_reference_against_40_digits(k):
    """the 1024 samples nearest to zero, and 1024 spread over the capture"""
    mp = pytest.importorskip("mpmath")
    assert len(_mp_cases()) == N_MP
    cap = _mp_cases()[k]
    r = cap.value()
    dec = cap.decided()
    live = min(cap.n, cap.total - cap.first)
    pick = np.unique(np.concatenate([np.argsort(np.abs(r[:live]))[:1024], np.arange(0, live, max(1, live // 1024))]))
    vi, vq = iq_ref.levels(cap.raw, cap.signed)
    mi, mq = cap.mean_used()
    th = iq_ref.theta(iq_ref.index(cap.first, cap.n), cap.mix_hz, cap.fs, cap.signed)
    worst = 0.0
    with mp.workdps(40):
        for s in pick:
            yi, yq = float(vi[s]) - mi, float(vq[s]) - mq  # the subtraction is the double one: part of the definition
            t = mp.mpf(float(th[s]))
            r40 = mp.mpf(yi) * mp.cos(t) - mp.mpf(yq) * mp.sin(t)
            worst = max(worst, float(abs(mp.mpf(float(r[s])) - r40)))
            if dec[s]:
                assert (r40 > 0) == (r[s] > 0), (s, r[s], r40)
    print(f"{cap.name}: {pick.size} samples, largest |r_double - r_40| {worst:.2e}")
    assert worst < 5e-13


@pytest.mark.usefixtures("hip_artifacts")
def test_accumulate_power_on_rails_and_short_lengths():
    import gpsacq
    lib = gpsacq.load_library()
    rng = np.random.default_rng(5)
    bufs = [np.full(2 * 1000, b, np.uint8) for b in (0x00, 0xFF, 0x80, 0x7F)] + [np.tile(np.array([0x00, 0xFF, 0xFF, 0x00], np.uint8), 777)]
    bufs += [rng.integers(0, 256, 2 * n, dtype=np.uint8) for n in range(1, 18)]
    for raw in bufs:
        for fmt in (0, 1):
            vi, vq = iq_ref.levels(raw, fmt == 1)
            pw = (ctypes.c_uint64 * 2)(11, 13)
            assert lib.gpsacq_iq8_accumulate_power(None, raw.ctypes.data_as(ctypes.c_void_p), raw.size // 2, fmt, pw) == 0
            assert pw[0] == 11 + sum(int(v) ** 2 for v in vi) and pw[1] == 13 + sum(int(v) ** 2 for v in vq)
