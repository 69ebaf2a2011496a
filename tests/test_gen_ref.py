"""tests/gen_ref.py and the case table of tests/gen_cases.py, checked on the CPU before the GPU tests (tests/test_gpu_generate.py)
lean on them: the reference's noise has the moments of a unit Gaussian, its exact cases equal predictions made by hand in Python
integers, its integer laws for q < 0 are Python's // and %, every case of the table leaves few enough samples undecided to mean
something, and ten wrong laws -- each one sentence of "THE GENERATOR'S LAW" of include/gpsacq.h misread -- are told from the right
one by at least 100 decided samples of some case.  The last is the evidence, had without a GPU, that the GPU tests would fail on a
subtly wrong kernel."""
import math
from fractions import Fraction

import numpy as np
import pytest

import gen_cases
import gen_ref
from gen_cases import CASES, case_id, cases, decided, expected, hand, n_samples, reference


# ---- noise -----------------------------------------------------------------------------------------------------------------------
def test_noise_moments():
    """2^20 samples of seed 77, every figure within five standard errors"""
    n = 1 << 20
    ni, nq = gen_ref.LAW.noise(77, np.arange(n, dtype=np.uint64))
    se = 1.0 / math.sqrt(n)
    for name, x in (("I", ni), ("Q", nq)):
        mean, var, m4 = x.mean(), x.var(), (x ** 4).mean()
        lags = [float((x[:-k] * x[k:]).mean()) for k in range(1, 9)]
        print("%s: mean %.3g, variance %.5f, fourth moment %.4f, lags 1..8 %s" % (name, mean, var, m4, " ".join("%.2g" % v for v in lags)))
        assert abs(mean) <= 5 * se
        assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / n)
        assert abs(m4 - 3.0) <= 5 * math.sqrt(96.0 / n)
        assert max(abs(v) for v in lags) <= 5 * se
    corr = float((ni * nq).mean())
    print("I.Q correlation %.3g" % corr)
    assert abs(corr) <= 5 * se


def test_uniforms_are_float32_values_in_their_ranges():
    """u1 = 1 is reached only through the float rounding of 2^32 - 1 + 1 and gives r = 0: no infinity, no NaN"""
    ni, nq = gen_ref.LAW.noise(2 ** 63 + 5, np.arange(1 << 16, dtype=np.uint64) + np.uint64(2 ** 40))
    assert np.isfinite(ni).all() and np.isfinite(nq).all() and np.abs(ni).max() < 6.7 and np.abs(nq).max() < 6.7
    z = 1                                                  # the finaliser of 1 in Python integers
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert int(gen_ref.mix64(np.array([1], np.uint64))[0]) == z ^ (z >> 31)


# ---- by hand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases("ties") + cases("iq-rint"), ids=case_id)
def test_exact_cases_equal_the_hand_prediction(c):
    ref = reference(c)
    want = hand(c)
    assert not ref["skip"].any()
    assert (expected(c, ref) == want).all()
    if c["group"] == "ties":
        assert set(np.unique(ref["y"][1::2]).tolist()) == {0.0} and set(np.unique(np.abs(ref["y"][0::2])).tolist()) == {1.0}
        assert 0.3 < want[0::2].mean() < 0.7 and not want[1::2].any()
    else:
        mag = {0.5: 0, 1.5: 2, 2.5: 2}[c["sats"][0][1]]
        off = 0 if c["signed"] else 128
        assert set(np.unique(want[:, 0]).tolist()) == {off - mag, off + mag} and set(np.unique(want[:, 1]).tolist()) == {off}
        assert (np.abs(ref["v"][:, 0]) == c["sats"][0][1]).all() and (ref["v"][:, 1] == 0.0).all()


def test_negative_chip_counts_against_python_integers():
    """q, the chip index and the navigation bit index where q < 0, and q itself at 2^40, against Fraction, // and %"""
    law = gen_ref.LAW
    seen_negative = 0
    for c in cases("nav") + [x for x in cases("sweep") if x["sats"][0][3] == -16368.75][:4] + cases("starts"):
        ref = reference(c)
        rng = np.random.default_rng(5)
        pick = np.unique(np.concatenate([np.arange(40), rng.integers(0, n_samples(c), 200), [n_samples(c) - 1]]))
        for s, (prn, amp, dop, cp, th) in enumerate(c["sats"]):
            cps = Fraction(law.chips_per_sample(dop, c["fs"]))
            for j in pick.tolist():
                q = math.floor((c["first"] + j + Fraction(cp)) * cps)
                assert int(ref["q"][s][j]) == q
                seen_negative += q < 0
                assert int(law.chip_index(np.array([q]))[0]) == q % 1023
                for n_nav in (1, 3, 50):
                    assert int(law.nav_index(np.array([q]), n_nav)[0]) == (q // 20460) % n_nav
    assert seen_negative > 100
    assert int(law.chip_index(np.array([-1]))[0]) == 1022 and int(law.nav_index(np.array([-1]), 50)[0]) == 49
    assert int(law.nav_index(np.array([-20460]), 50)[0]) == 49 and int(law.nav_index(np.array([-20461]), 50)[0]) == 48


def test_the_split_of_base_and_j_times_rate_against_fractions():
    """floor and fractional part of base + j * rate to 2^-50 where the whole is of size 2^40, rates of both signs, j up to 2^20"""
    rng = np.random.default_rng(9)
    for base, rate in ((Fraction(2 ** 40) * Fraction(0.1875000012) + Fraction(-0.5), 0.1875000012), (Fraction(-12345.678), -0.0458),
                       (Fraction(0.3), 0.0), (Fraction(0.7481671554252199) * (2 ** 40 + 8) + Fraction(7.9), 0.7481671554252199)):
        fl, fr = gen_ref.affine(base, rate, 1 << 20)
        for j in [0, 1, 2, (1 << 20) - 1] + rng.integers(0, 1 << 20, 300).tolist():
            exact = base + j * Fraction(rate)
            assert abs((int(fl[j]) + Fraction(float(fr[j]))) - exact) <= Fraction(1, 2 ** 50)
            assert 0.0 <= fr[j] <= 1.0 and (int(fl[j]) == math.floor(exact) or min(fr[j], 1.0 - fr[j]) < 2.0 ** -50)


def test_nav_windows_hold_what_they_are_for():
    for c in cases("nav"):
        q = reference(c)["q"]
        if c["name"].startswith("negative"):
            assert (q[0] < 0).sum() > 900 and (q[1] < 0).any() and (q[0] > 0).any()
        else:
            assert q[0][0] < 200 * 20460 <= q[0][-1]
            b = gen_ref.LAW.nav_index(q[0], c["nav"].shape[1])
            assert c["nav"].shape[1] == 1 or c["nav"][0][b[0]] != c["nav"][0][b[-1]]


def test_the_table_has_the_shapes_the_kernels_can_go_wrong_at():
    assert max(n_samples(c) for c in CASES) <= 1 << 20
    assert {c["n"] for c in cases("lengths")} == {1, 255, 256, 257, 8192}
    assert {c["first"] for c in cases("starts")} == {0, 8, 2 ** 32 - 8, 2 ** 40} and all(c["first"] % 8 == 0 for c in cases(kind="bits"))
    assert {c["first"] for c in cases("iq-lengths")} >= {0, 12345, 2 ** 32 - 3} and {c["n"] for c in cases("iq-lengths")} >= {1, 255, 256, 257}
    assert {c["seed"] for c in cases("noisy")} == {0, 77, 2 ** 63 + 5} and {c["sigma"] for c in cases("noisy")} == {1.0, 0.25}
    assert len({s[0] for s in cases("twelve")[0]["sats"]}) == 12
    assert set(gen_cases.GROUPS) == {c["group"] for c in CASES}


# ---- the caps: conditions on the inputs, checked on the reference alone -------------------------------------------------------------
@pytest.mark.parametrize("group", gen_cases.GROUPS)
def test_caps(group):
    for c in cases(group):
        ref = reference(c)
        dec = decided(c, ref)
        n = dec.size
        left_out = float(ref["skip"].mean())
        undecided = 1.0 - float(dec.mean())
        print("%-34s left out %.3g, undecided %.3g of %d" % (case_id(c), left_out, undecided, n))
        if c["exact"]:                       # predicted by hand everywhere: nothing may be left out
            assert left_out == 0.0
            continue
        assert left_out <= 1e-4 or n < 1 << 14
        if c["sigma"] == 0.0 and c["kind"] == "bits":
            # 1e-4 in all.  On top of it, where the true carrier (fc + doppler) / fs is 31/140 or 61/280 cycle per sample (rate B,
            # Doppler 0 or -10 000 Hz) and theta a multiple of 1/10: the 2 of every 140, or 280, samples whose cosine is zero but
            # for rounding.
            zeros = {0.0: 2.0 / 140, -10000.0: 2.0 / 280}.get(c["sats"][0][2], 0.0) if group == "sweep" and c["fs"] == 2.8e6 else 0.0
            assert undecided <= 1e-4 + zeros or n < 1 << 14
        elif c["sigma"] == 0.0:
            # The fractional part of a noise-free 8-bit value is spread evenly at the scale of the margin, so a share of 2 * margin of
            # them lies next to a half-integer; twice that is allowed for the uneven density of a cosine.
            assert undecided - left_out <= 4.0 * float(ref["margin"].max())
        elif c["kind"] == "bits":
            assert undecided - left_out <= 2e-3 or n < 1 << 14
        else:
            assert undecided - left_out <= 0.04 or n < 1 << 14
    if group == "iq-clamp":
        for c in cases(group):
            want = expected(c, reference(c)).astype(np.int16) - (0 if c["signed"] else 128)
            assert want.min() == -127 and want.max() == 127 and (want == -127).sum() > 100 and (want == 127).sum() > 100


# ---- power -----------------------------------------------------------------------------------------------------------------------
class CodeDopplerOfTheWrongSign(gen_ref.Law):
    def chips_per_sample(self, doppler, fs):
        return gen_ref.CPS * (1.0 - doppler / gen_ref.L1) / fs


class ChipIndexPlusOne(gen_ref.Law):
    def chip_index(self, q):
        return np.mod(q + 1, 1023)


class ThetaIgnored(gen_ref.Law):
    def theta(self, carrier_phase_cycles):
        return 0.0


class QNegated(gen_ref.Law):
    def q_arm(self, sin):
        return -sin


class TruncForFloor(gen_ref.Law):
    def chip_count(self, q_floor):
        return np.where(q_floor < 0, q_floor + 1, q_floor)      # positions on an integer are left out anyway


class NavBitOf20461Chips(gen_ref.Law):
    def nav_index(self, q, n_nav):
        return np.mod(np.floor_divide(q, 20461), n_nav)


class RoundHalfAwayFromZero(gen_ref.Law):
    def round(self, v):
        return np.sign(v) * np.floor(np.abs(v) + 0.5)


class ClampToMinus128(gen_ref.Law):
    clamp_lo = -128.0


class NoiseQForOneBit(gen_ref.Law):
    def noise_1bit(self, n_i, n_q):
        return n_q


class SampleIndexModulo2To32(gen_ref.Law):
    def sample_index(self, m):
        return m & np.uint64(0xFFFFFFFF)


MUTANTS = [
    (CodeDopplerOfTheWrongSign, ["sweep/A-prn1-d-10000-c1e+06-t0.3", "sweep/B-prn32-d7654.3-c1e+06-t7.9"]),
    (ChipIndexPlusOne, ["sweep/A-prn1-d-10000-c-0.5-t0.3", "twelve/twelve", "iq-sense/if+250000"]),
    (ThetaIgnored, ["sweep/A-prn1-d0-c-0.5-t0.3", "sweep/B-prn32-d0-c-0.5-t-1.3", "iq-sense/if-250000"]),
    (QNegated, ["iq-sense/if+250000", "iq-sense/if-250000", "iq-noisy/plain"]),
    (TruncForFloor, ["sweep/A-prn1-d0-c-16368.8-t0.3", "nav/negative-3"]),
    (NavBitOf20461Chips, ["nav/boundary-3", "nav/boundary-50", "iq-noisy/nav"]),
    (RoundHalfAwayFromZero, ["iq-rint/amp-0.5-s8", "iq-rint/amp-2.5-u8"]),
    (ClampToMinus128, ["iq-clamp/clamp-s8", "iq-clamp/clamp-u8"]),
    (NoiseQForOneBit, ["noisy/sigma1-seed77", "lengths/noise-8192"]),
    (SampleIndexModulo2To32, ["starts/first-4294967288", "starts/first-1099511627776", "iq-lengths/first-2^32-3"]),
]


def disagreements(c, law):
    """decided values of case c on which the wrong law's output differs from the right one's: decided under both laws, so that no
    margin could excuse them; in an exact case, every value that differs from the hand prediction"""
    mut = reference(c, law)
    got = expected(c, mut, law)
    if c["exact"]:
        return int((got != hand(c)).sum())
    ref = reference(c)
    return int((decided(c, ref) & decided(c, mut) & (got != expected(c, ref))).sum())


@pytest.mark.parametrize("law,where", MUTANTS, ids=[m[0].__name__ for m in MUTANTS])
def test_the_table_tells_a_wrong_law_from_the_right_one(law, where):
    by_id = {case_id(c): c for c in CASES}
    counts = {w: disagreements(by_id[w], law()) for w in where}
    print(law.__name__, counts)
    assert max(counts.values()) >= 100


def test_the_right_law_has_no_disagreement_with_itself():
    c = cases("noisy")[1]
    assert disagreements(c, gen_ref.Law()) == 0
