"""The signs of the 8-bit IQ front end (csrc/iq_convert.hpp: iq8_bit's float fast path with its double fall-back below |r| = 5e-3)
on the GPU against tests/iq_ref.py, a reference written from include/gpsacq.h and the scripts, itself held against 40 digits in
tests/test_iq_ref.py -- not against the device's own converter, which shares the function under test:

  a. gpsacq_iq8_to_bits (k_iq_to_bits): every decided sample equal on all 65 536 byte pairs x 16 phases (both formats, no mixer /
     0.62e6 @ 2.8e6 / 2.6e6 @ 10e6, mean removed or not), on captures whose pairs were chosen per sample index to put r next to zero
     or next to the 5e-3 threshold, on fc = fs / 4 with one arm zero, on the byte rails with means -127.5, 0 and 126.5, and on
     lengths 1 .. 17, 4099 and eight workgroups +- 1 output byte;
  b. gpsacq_search_iq8 in sign mode (k_fwd2<SRC_IQ8>) with explicit fractional means at first_sample 0, 2^33 + 12345 and
     2^40 + 12345, and with the capture ending inside the last block: cells and peaks byte for byte those of gpsacq_search on the
     reference's bits;
  c. gpsacq_track_iq8 in sign mode from capture sample 2^33 + 12345, in one window and in three: prompt sums, records and channels
     byte for byte those of gpsacq_track on the reference's bits;
  d. gpsacq_iq8_accumulate_sums (k_iq_sums) against Python integers: constant bytes, alternating rails, random; 1 .. 17 samples
     and one sample either side of the 2048 x 256 x 8 the grid covers in one stride; the same buffer in chunks of 70 001.

In b and c nothing can be masked, so those captures have no undecided sample (asserted in tests/test_iq_ref.py).  Every
comparison is equality.

Measured on an MI355X (pytest -s prints a line per case: samples, undecided, within 1e-3 of the threshold, wrong).  No case has
an undecided sample and none a wrong one:
    exhaustive, 12 captures of 1 048 576: no mixer 0 near the threshold; 0.62e6 @ 2.8e6 25 / 6 (uint8, mean removed / not) and
        22 / 4 (int8); 2.6e6 @ 10e6 17 / 12 and 14 / 8
    adversarial, 65 536 each (61 440 chosen + 4096 that complete the sums): next to zero 8938, 8835 (uint8; 0.618 @ 2.8, 2.618 @ 10)
        and 8907, 8913 (int8) near the threshold; next to the threshold 22 912, 22 715 and 22 827, 22 567
    quarter rate, 16 389 each (2.8 MHz with means (0, 0) and (3, -2), 10 MHz): 0 near the threshold -- r is one product or zero
    rails, 8160 each: low/high 13, mid/mid 1, high/low 14, mid/low 10 (uint8); 15, 1, 15, 6 (int8)
    lengths: at most 1 near the threshold
    fused search, 122 880 each: 31 800 (n0 = 0), 31 625 (int8, 2^33 + 12345), 27 047 (ragged end), 31 552 (2^40 + 12345)
    tracking, 83 997 samples: 21 595; 29 epochs on each of the 3 channels
The file takes 7 s, 1.7 s of it the engine; the longest test 0.8 s.
Mutation check (not kept): with the fast path's limit at 5e-6 instead of 5e-3, 7 of the 8 adversarial captures (1 to 9 samples
wrong), all four fused searches and the tracking test fail; without the second term of the 2 pi reduction the search at 2^40 fails
(at 2^33 the phase error, 5e-7, stays inside the fast path's margin, as it should).
"""
import ctypes

import numpy as np
import pytest

import iq_ref

pytestmark = pytest.mark.gpu
T0 = 2 ** 33 + 12344  # the byte grid of the 1-bit stream the tracking test runs on: its sample T0 + j is capture sample BIG + j


@pytest.fixture(scope="module")
def eng():
    import gpsacq
    with gpsacq.Engine(0.62e6, 2.8e6, 5000.0, device=0) as e:
        yield e


# ---- a. the stand-alone converter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(iq_ref.N_STANDALONE))
def test_converter_equals_reference_on_decided_samples(eng, k):
    cap = iq_ref.standalone_cases()[k]
    n, und, thr = cap.report()
    got = eng.iq8_to_bits(cap.raw, signed=cap.signed, remove_dc=cap.remove_dc, mix_hz=cap.mix_hz, fs=cap.fs)
    want = cap.bits()
    wrong = (iq_ref.unpack(got, n) != iq_ref.unpack(want, n)) & cap.decided()
    print(f"{cap.line()}, {int(wrong.sum())} wrong")
    assert und <= 1e-5 * n
    if "adversarial threshold" in cap.name:
        assert thr >= 100
    assert got.size == (n + 7) // 8
    assert not wrong.any(), (np.flatnonzero(wrong)[:8], cap.value()[wrong][:8])
    if n % 8:
        assert got[-1] >> (n % 8) == 0  # the bits past the end are zero


# ---- b. the conversion fused into the forward transform ----------------------------------------------------------------------------
TASKS = [(0, 0), (0, 17), (1, 5), (2, 31), (2, 9)]


@pytest.mark.parametrize("k", range(4))
def test_fused_search_equals_search_of_reference_bits(eng, k):
    cap = iq_ref.search_cases()[k]
    print(cap.line())
    assert cap.decided().all() and cap.n == 3 * 40960
    inp = eng.iq8_input(signed=cap.signed, remove_dc=True, mean=cap.mean, mix_hz=cap.mix_hz, fs=cap.fs, first_sample=cap.first,
                        total_samples=cap.total, multibit=0)
    want = cap.bits()
    c1, p1 = eng.search(want, tasks=TASKS)
    c2, p2 = eng.search_iq8(cap.raw, inp, tasks=TASKS)
    assert c1.tobytes() == c2.tobytes() and p1.tobytes() == p2.tobytes()
    if k == 0:  # what the equality is worth: one sample of block 1 the other way moves that block's cells and no other's
        flip = want.copy()
        flip[5120 + 1234] ^= 0x10
        c3, _ = eng.search(flip, tasks=TASKS)
        assert c3[2].tobytes() != c1[2].tobytes() and c3[:2].tobytes() == c1[:2].tobytes() and c3[3:].tobytes() == c1[3:].tobytes()


# ---- c. tracking, sign mode ----------------------------------------------------------------------------------------------------------
def _hit(eng, lo_shift, ca_shift):
    import gpsacq
    pk = np.zeros(1, gpsacq.PEAK_DTYPE)
    pk["snr"], pk["lo_shift"], pk["ca_shift"] = 100.0, lo_shift, ca_shift
    return pk[0]


def test_sign_mode_tracking_equals_tracking_of_reference_bits(eng):
    cap = iq_ref.track_case()
    print(cap.line())
    assert cap.decided().all() and cap.first == T0 + 1 and T0 % 8 == 0
    n, mean = cap.n, cap.mean
    inp = lambda off: eng.iq8_input(signed=cap.signed, remove_dc=True, mean=mean, mix_hz=cap.mix_hz, fs=cap.fs, first_sample=cap.first + off,
                                    total_samples=cap.total, multibit=0)
    p = eng.track_params()
    start = np.concatenate([eng.track_start(prn, _hit(eng, lo, ca), T0, params=p) for prn, lo, ca in ((3, 17, 100), (11, -40, 1999), (32, 0, 2799))])
    ref = start.copy()
    pr, rr, nr = eng.track(cap.bits(), ref, first_sample=T0, records=True, params=p)
    one = start.copy()
    po, ro, no = eng.track_iq8(cap.raw, inp(0), one, first_sample=T0, records=True, params=p, max_epochs=pr.shape[1])
    print("epochs per channel", nr.tolist())
    assert nr.min() >= 25  # (30 ms)
    assert np.array_equal(nr, no) and one.tobytes() == ref.tobytes()
    for c in range(start.size):
        assert po[c, :nr[c]].tobytes() == pr[c, :nr[c]].tobytes() and ro[c, :nr[c]].tobytes() == rr[c, :nr[c]].tobytes(), c
    # three unequal windows; each starts at the byte that holds the earliest channel's next sample: capture sample 1 mod 8
    pieces, recs, proms = start.copy(), [[] for _ in start], [[] for _ in start]
    for end in (n // 5 // 8 * 8, (3 * n) // 5 // 8 * 8, n):
        off = (int(pieces["next_sample"].min()) - T0) // 8 * 8
        assert (cap.first + off) % 8 == 1
        pw, r, ne = eng.track_iq8(cap.raw[2 * off:2 * end], inp(off), pieces, first_sample=T0 + off, records=True, params=p)
        for c in range(start.size):
            recs[c].append(r[c, :ne[c]])
            proms[c].append(pw[c, :ne[c]])
    assert pieces.tobytes() == ref.tobytes()
    for c in range(start.size):
        assert np.concatenate(recs[c]).tobytes() == rr[c, :nr[c]].tobytes() and np.concatenate(proms[c]).tobytes() == pr[c, :nr[c]].tobytes(), c


# ---- d. the integer sums -----------------------------------------------------------------------------------------------------------
GRID = 2048 * 256 * 8  # samples one stride of k_iq_sums' grid covers


def _patterns(n, rng):
    yield "0x00", np.zeros(2 * n, np.uint8)
    yield "0xFF", np.full(2 * n, 0xFF, np.uint8)
    yield "0x80", np.full(2 * n, 0x80, np.uint8)
    yield "rails 00/FF", np.resize(np.array([0x00, 0xFF, 0xFF, 0x00], np.uint8), 2 * n)
    yield "rails 7F/80", np.resize(np.array([0x7F, 0x80, 0x80, 0x7F], np.uint8), 2 * n)
    yield "random", rng.integers(0, 256, 2 * n, dtype=np.uint8)


def _device_sums(eng, raw, signed, start=(0, 0)):
    s = (ctypes.c_int64 * 2)(*start)  # it adds to what is there
    rc = eng._lib.gpsacq_iq8_accumulate_sums(eng._h, raw.ctypes.data_as(ctypes.c_void_p), raw.size // 2, 1 if signed else 0, s)
    assert rc == 0
    return s[0] - start[0], s[1] - start[1]


@pytest.mark.parametrize("lengths", [tuple(range(1, 18)), (GRID - 1,), (GRID,), (GRID + 1,)], ids=["1-17", "grid-1", "grid", "grid+1"])
def test_integer_sums(eng, lengths):
    rng = np.random.default_rng(len(lengths) + lengths[0])
    for n in lengths:
        for name, raw in _patterns(n, rng):
            for signed in (False, True):
                want = iq_ref.sums(raw, signed)
                assert _device_sums(eng, raw, signed, (-7, 1 << 40)) == want, (n, name, signed)
                assert eng.iq8_mean(raw, signed=signed) == (want[0] / n, want[1] / n)
    print(f"lengths {lengths[0]}..{lengths[-1]}: 6 patterns x 2 formats equal")


def test_integer_sums_in_ragged_chunks(eng):
    rng = np.random.default_rng(9)
    n = GRID + 1
    for name, raw in list(_patterns(n, rng))[3:]:
        for signed in (False, True):
            want = iq_ref.means(raw, signed)
            assert eng.iq8_mean(raw, signed=signed, chunk_samples=70001) == want, (name, signed)
