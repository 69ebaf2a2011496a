"""The synthetic capture generators on the GPU (k_generate, k_generate_iq8 of csrc/gen_kernels.hip through Engine.generate*,
Engine.generate_iq8*) against tests/gen_ref.py, the numpy restatement of "THE GENERATOR'S LAW" of include/gpsacq.h, over the case
table of tests/gen_cases.py.

1-bit: outside the left-out mask every sample with |y_ref| > tau has bit (y_ref < 0), with no exception; inside tau anything goes.
8-bit: outside the mask every arm value whose v_ref lies further than scale * tau from a half-integer equals
clamp(rint(v_ref)) exactly; the others differ from it by at most 1.  tau, the mask and the shares of samples they may take are
fixed in gen_ref.py and tests/test_gen_ref.py, where ten wrong laws are shown to fail these comparisons.  The exact cases ("ties",
"iq-rint") must equal a prediction made by hand in every sample.

Measured on an MI355X: no disagreement outside the margins in any group, so there is no worst |y_ref| to quote.  Samples (1-bit) or
arm values (8-bit) compared / left out / inside the margin, and how many of the last differ from the reference's own rounding:
    lengths      143 273 /  0 /    103 / 0        iq-lengths      17 399 / 0 /    527 / 0
    starts       229 153 /  0 /    223 / 1        iq-rint         24 576 / 0 / 24 576 / 0  (all equal the hand prediction)
    sweep      8 622 634 / 24 / 28 094 / 0        iq-clamp       262 014 / 0 /    130 / 0
    ties          65 536 /  0 / 65 536 / 0  (hand) iq-sense       262 058 / 0 /     86 / 0
    nav          393 216 /  0 /      0 / 0        iq-noisy     1 015 833 / 0 / 32 743 / 2
    twelve        65 535 /  1 /      0 / 0
    noisy      1 309 864 /  0 /    856 / 0
Each test prints its own figures before it asserts (pytest -s)."""
import numpy as np
import pytest

import gen_cases
from gen_cases import case_id, cases, compare, hand, n_samples, report, samples

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def engines():
    import gpsacq
    with gpsacq.Engine(*gen_cases.RATE_A, 5000.0) as a, gpsacq.Engine(*gen_cases.RATE_B, 5000.0) as b:
        yield {gen_cases.RATE_A: a, gen_cases.RATE_B: b}


def generate(engines, c, **over):
    """the host form's output for case c (with fields overridden)"""
    c = dict(c, **over)
    eng = engines[(c["fc"], c["fs"])]
    if c["kind"] == "bits":
        return eng.generate(c["n"], c["sats"], noise_sigma=c["sigma"], seed=c["seed"], first_sample=c["first"], nav=c["nav"])
    return eng.generate_iq8(c["n"], c["sats"], if_hz=c["if_hz"], scale=c["scale"], signed=c["signed"], noise_sigma=c["sigma"], seed=c["seed"],
                            first_sample=c["first"], nav=c["nav"])


@pytest.mark.parametrize("group", gen_cases.GROUPS)
def test_against_the_reference(engines, group):
    """every case of the group: no decided value differs, no undecided 8-bit value is off by more than 1, exact cases are exact"""
    failed, total = [], dict(compared=0, left_out=0, in_margin=0, bad=0)
    for c in cases(group):
        out = generate(engines, c)
        assert out.size == (c["n"] if c["kind"] == "bits" else 2 * c["n"])
        got = samples(c, out)
        r = compare(c, got)
        print(report(c, r))
        for k in total:
            total[k] += r[k]
        if r["bad"] or r["off_by_more"]:
            failed.append(report(c, r))
        if c["exact"]:
            wrong = int((got != hand(c)).sum())
            print("%-34s %d of %d values differ from the hand prediction" % (case_id(c), wrong, got.size))
            if wrong:
                failed.append("%s: %d values differ from the hand prediction" % (case_id(c), wrong))
        if group == "iq-clamp":
            v = got.astype(np.int16) - (0 if c["signed"] else 128)
            print("%-34s values %d .. %d" % (case_id(c), v.min(), v.max()))
            assert v.min() == -127 and v.max() == 127       # both rails reached, -128 (byte 0 of uint8) never
    print("%s: %d cases, %d compared, %d left out, %d inside the margin, %d disagreements" % (
        group, len(cases(group)), total["compared"], total["left_out"], total["in_margin"], total["bad"]))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("group", [g for g in gen_cases.GROUPS if g.startswith("iq-")])
def test_uint8_is_int8_plus_128(engines, group):
    for c in cases(group):
        s8 = generate(engines, c, signed=True)
        u8 = generate(engines, c, signed=False)
        assert s8.dtype == np.int8 and u8.dtype == np.uint8
        assert (u8.astype(np.int16) == s8.astype(np.int16) + 128).all(), case_id(c)


def test_satellites_without_amplitude_leave_the_noise_alone(engines):
    """amplitude 0, or an empty list, gives the bytes of the noise-only capture: 1-bit and 8-bit, with and without nav"""
    c = cases("lengths")[-1]
    assert c["name"] == "two-8192"
    noise = generate(engines, c, sats=[])
    silent = [(prn, 0.0, dop, cp, th) for prn, amp, dop, cp, th in c["sats"]]
    assert (generate(engines, c, sats=silent) == noise).all()
    assert (generate(engines, c, sats=silent, nav=np.array([[1, -1, 1], [-1, -1, 1]], np.int8)) == noise).all()
    assert (generate(engines, c) != noise).any()
    assert (noise == generate(engines, cases("lengths")[-2], seed=c["seed"])).all()
    q = cases("iq-noisy")[0]
    noise = generate(engines, q, sats=[], n=4099)
    assert (generate(engines, q, sats=[(prn, 0.0, dop, cp, th) for prn, amp, dop, cp, th in q["sats"]], n=4099) == noise).all()
    assert (generate(engines, q, n=4099) != noise).any()


DEVICE_CASES = [c for c in gen_cases.CASES if case_id(c) in (
    "lengths/two-1", "lengths/two-257", "starts/first-4294967288", "nav/boundary-3", "iq-lengths/n-1", "iq-lengths/n-257",
    "iq-lengths/first-2^32-3", "iq-noisy/nav")]


@pytest.mark.parametrize("c", DEVICE_CASES, ids=case_id)
def test_device_forms_write_the_same_bytes_and_nothing_more(engines, c):
    """the *_device forms with sync = 0, then a synchronise: the host form's bytes, and the byte (1-bit) or sample (8-bit) after
    them keeps its 0xA5"""
    import torch
    eng = engines[(c["fc"], c["fs"])]
    host = generate(engines, c).view(np.uint8)
    extra = 1 if c["kind"] == "bits" else 2
    d = torch.full((host.size + extra,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if c["kind"] == "bits":
        eng.generate_device(d.data_ptr(), c["n"], c["sats"], noise_sigma=c["sigma"], seed=c["seed"], sync=False, first_sample=c["first"], nav=c["nav"])
    else:
        eng.generate_iq8_device(d.data_ptr(), c["n"], c["sats"], if_hz=c["if_hz"], scale=c["scale"], signed=c["signed"], noise_sigma=c["sigma"],
                                seed=c["seed"], first_sample=c["first"], nav=c["nav"], sync=False)
    eng.synchronize()
    got = d.cpu().numpy()
    print("%-34s %d bytes, tail %s" % (case_id(c), host.size, got[host.size:].tolist()))
    assert (got[:host.size] == host).all()
    assert (got[host.size:] == FILL).all()
    assert n_samples(c) == (8 if c["kind"] == "bits" else 1) * c["n"]
