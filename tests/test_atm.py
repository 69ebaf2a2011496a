"""Atmosphere-corrected fixes, host side (include/gpsacq.h, "Atmosphere, elevation mask and DOP"): the page-18 decode
(gpsacq_iono_load) against tests/atm_ref.py's encoder, the parameters, the struct sizes -- and the reference itself, the yardstick of
tests/test_gpu_atm.py, against its own truth maker.  Needs the library, no GPU."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import atm_ref
import nav_ref
from nav_helpers import geometry

pytestmark = pytest.mark.usefixtures("hip_artifacts")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_CODES = (-128, -1, 0, 127)


def _records(words_list, tows, sf_id=4):
    import gpsacq
    sf = np.zeros(len(words_list), gpsacq.SUBFRAME_DTYPE)
    for k, w in enumerate(words_list):
        sf["words"][k], sf["id"][k], sf["tow"][k] = w, sf_id, tows[k]
    return sf


def _assert_exact(io, alpha_codes, beta_codes, tow):
    a, b = atm_ref.coefficients(alpha_codes, beta_codes)
    assert io["valid"][0] == 1 and io["tow"][0] == tow
    assert io["alpha"][0].tobytes() == np.array(a).tobytes(), (io["alpha"][0], a)
    assert io["beta"][0].tobytes() == np.array(b).tobytes(), (io["beta"][0], b)


@pytest.fixture(scope="module")
def pages():
    """200 random pages: eight signed codes each; the first rows put -128, -1, 0 and 127 into every field"""
    rng = np.random.default_rng(18)
    codes = rng.integers(-128, 128, (200, 8))
    for k, c in enumerate(EDGE_CODES):
        codes[k, :] = c
        codes[4 + k, :] = np.roll(EDGE_CODES, k).repeat(2)
    for f in range(8):
        assert set(EDGE_CODES) <= set(codes[:, f])
    return codes


def test_struct_sizes(tmp_path):
    import gpsacq
    sizes = (gpsacq.IONO_DTYPE.itemsize, gpsacq.ATM_PARAMS_DTYPE.itemsize, gpsacq.FIX_DOP_DTYPE.itemsize, gpsacq.SAT_VIEW_DTYPE.itemsize)
    src = tmp_path / "sizes.c"
    src.write_text('#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_iono) == %d, "iono");\n'
                   '_Static_assert(sizeof(gpsacq_atm_params) == %d, "params");\n'
                   '_Static_assert(sizeof(gpsacq_fix_dop) == %d, "dop");\n'
                   '_Static_assert(sizeof(gpsacq_sat_view) == %d, "view");\n' % sizes)
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert sizes == (72, 80, 48, 32)
    for dt in (gpsacq.IONO_DTYPE, gpsacq.ATM_PARAMS_DTYPE, gpsacq.FIX_DOP_DTYPE, gpsacq.SAT_VIEW_DTYPE):
        assert dt.itemsize == sum(dt[n].itemsize for n in dt.names)
    assert (gpsacq.ATM_IONO, gpsacq.ATM_TROPO, gpsacq.ATM_ROUNDS) == (1, 2, 3) == (atm_ref.ATM_IONO, atm_ref.ATM_TROPO, atm_ref.ROUNDS)


def test_decode_200_random_pages_exact(pages):
    import gpsacq
    rng = np.random.default_rng(19)
    for k, codes in enumerate(pages):
        tow = int(rng.integers(0, 100800))
        words = atm_ref.page18_words(codes[:4], codes[4:], tow, rng)
        io = gpsacq.iono(_records([words], [tow]))
        _assert_exact(io, codes[:4], codes[4:], tow)


def test_decode_through_bit_stream_both_polarities(pages):
    """page -> parity encoder -> 0/1 stream (upright and inverted, so with both values of D30* in front of every word) ->
    gpsacq_nav_subframes -> gpsacq_iono_load"""
    import gpsacq
    eph = geometry()["ephs"][0]
    for k, codes in enumerate(pages[:40]):
        tow0 = 2000 + 5 * k
        bits = atm_ref.frame_bits(eph, tow0, atm_ref.page18_words(codes[:4], codes[4:], tow0 + 3, np.random.default_rng(k)), seed=k)
        for invert in (False, True):
            sf, nfail = gpsacq.nav_subframes(1 - bits if invert else bits)
            assert nfail == 0 and list(sf["id"]) == [1, 2, 3, 4, 5] and bool(sf["inverted"].all()) == invert
            _assert_exact(gpsacq.iono(sf), codes[:4], codes[4:], tow0 + 3)
            # the ephemeris of the same stream is untouched by the new decoder, and the other way round
            assert gpsacq.ephemeris_valid(gpsacq.ephemeris(sf, 1)[0])
            if k < 4:  # and from the prompt arm of a channel: 20 epochs per bit, 1 = negative I, through gpsacq_nav_bits
                stream = 1 - bits if invert else bits
                ip = np.repeat(np.where(stream == 1, -900, 900), 20).astype(np.int32)
                got, epoch0 = gpsacq.nav_bits(np.concatenate([np.full(13, ip[0], np.int32), ip]))
                assert epoch0 % 20 == 13 and got.size >= 1500
                sf2, nfail = gpsacq.nav_subframes(got)
                assert nfail == 0 and 4 in sf2["id"]
                _assert_exact(gpsacq.iono(sf2), codes[:4], codes[4:], tow0 + 3)


def test_other_pages_and_subframes_leave_the_record_untouched(golden_dir):
    import gpsacq
    rng = np.random.default_rng(20)
    before = gpsacq.iono(_records([atm_ref.page18_words((1, 2, 3, 4), (5, 6, 7, 8), 77, rng)], [77]))
    assert before["valid"][0] == 1
    others = []
    for byte in (0x79, 0x38, 0x7F, 0x00, 0x78 ^ 0x80, 0x78 ^ 0x01):  # other page IDs and other data IDs
        others.append(atm_ref.page18_words((9,) * 4, (9,) * 4, 5, rng, page_byte=byte))
    for sf_id in (1, 2, 3, 5, 0, 6, 7):  # the page byte in place, but not subframe 4
        others.append(atm_ref.page18_words((9,) * 4, (9,) * 4, 5, rng, sf_id=sf_id))
    sf = _records(others, [5] * len(others))
    assert gpsacq.iono(sf, io=before[0]).tobytes() == before.tobytes()
    fresh = gpsacq.iono(sf)
    assert fresh["valid"][0] == 0 and not fresh.view(np.uint8).any()
    assert gpsacq.iono(sf[:0]).tobytes() == bytes(72)
    # the 2011 capture: its two subframe-4 pages are pages 63 and 57
    d = json.load(open(os.path.join(golden_dir, "holme_nav_2011.json")))
    real, nfail = gpsacq.nav_subframes(np.array([int(c) for c in "".join(d["bits"])], np.uint8))
    assert nfail == 0 and list(real["id"]).count(4) == 2
    assert sorted(int(w[2]) >> 16 & 0x3F for w in real["words"][real["id"] == 4]) == [57, 63]
    io = gpsacq.iono(real)
    assert io["valid"][0] == 0 and io.tobytes() == bytes(72)


def test_a_later_page_replaces_an_earlier_one():
    import gpsacq
    rng = np.random.default_rng(21)
    first = atm_ref.page18_words((10, 20, 30, 40), (50, 60, 70, 80), 100, rng)
    other = atm_ref.page18_words((9,) * 4, (9,) * 4, 101, rng, page_byte=0x79)
    second = atm_ref.page18_words((-10, -20, -30, -40), (-50, -60, -70, -80), 102, rng)
    _assert_exact(gpsacq.iono(_records([first, other, second], [100, 101, 102])), (-10, -20, -30, -40), (-50, -60, -70, -80), 102)
    _assert_exact(gpsacq.iono(_records([second, other, first], [102, 101, 100])), (10, 20, 30, 40), (50, 60, 70, 80), 100)
    # carried on from an earlier record
    io = gpsacq.iono(_records([first], [100]))
    _assert_exact(gpsacq.iono(_records([other, second], [101, 102]), io=io[0]), (-10, -20, -30, -40), (-50, -60, -70, -80), 102)


def test_parameters_defaults_and_errors():
    import gpsacq
    lib = gpsacq.load_library()
    p = gpsacq.atm_params()
    assert p["flags"][0] == 3 and p["reserved"][0] == 0 and not p["alpha"].any() and not p["beta"].any()
    assert abs(p["elev_mask"][0] - math.radians(5.0)) < 1e-16
    io = gpsacq.iono(_records([atm_ref.page18_words(atm_ref.ALPHA_CODES, atm_ref.BETA_CODES, 7)], [7]))
    p = gpsacq.atm_params(io[0], elev_mask=0.3, flags=1)
    a, b = atm_ref.coefficients()
    assert list(p["alpha"][0]) == a and list(p["beta"][0]) == b and p["elev_mask"][0] == 0.3 and p["flags"][0] == 1
    io["valid"] = 0  # not valid: zeros
    assert not gpsacq.atm_params(io[0])["alpha"].any()
    assert lib.gpsacq_atm_default_params(None, None) == 1
    assert lib.gpsacq_iono_load(None, None, 0) == 1
    rec = np.zeros(1, gpsacq.IONO_DTYPE)
    assert lib.gpsacq_iono_load(rec.ctypes.data_as(ctypes.c_void_p), None, 1) == 1
    assert lib.gpsacq_iono_load(rec.ctypes.data_as(ctypes.c_void_p), None, -1) == 1


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_zenith_delay_at_14h_local_time_by_hand():
    """a satellite straight up, at the local time the cosine peaks: x = 0, F = 1 + 16 * 0.03^3, psi = 0.0137 / 0.61 - 0.022"""
    p = atm_ref.params()
    lat, lon = math.radians(30.0), math.radians(20.0)
    psi = 0.0137 / (0.5 + 0.11) - 0.022
    phi_i = lat / math.pi + psi  # az = 0 at the zenith
    lam_i = lon / math.pi
    phi_m = phi_i + 0.064 * math.cos((lam_i - 1.617) * math.pi)
    tow = 3 * 86400 + 50400.0 - 4.32e4 * lam_i  # local time 14:00 at the pierce point
    amp = sum(a * phi_m ** n for n, a in enumerate(p["alpha"]))
    assert amp > 1e-8  # the coefficients make the ionosphere matter: 3 m at the zenith
    by_hand = nav_ref.C * (1 + 16 * 0.03 ** 3) * (5e-9 + amp)
    got = float(atm_ref.klobuchar(0.0, math.pi / 2, lat, lon, tow, p))
    print("zenith at 14 h: %.6f m by hand, %.6f m" % (by_hand, got))
    assert abs(got - by_hand) < 1e-9 and got > 3.0
    # twelve hours later: the night floor
    assert abs(float(atm_ref.klobuchar(0.0, math.pi / 2, lat, lon, tow + 43200, p)) - nav_ref.C * (1 + 16 * 0.03 ** 3) * 5e-9) < 1e-12
    # and a standard-atmosphere zenith troposphere of 2.3 .. 2.5 m at sea level
    assert 2.3 < float(atm_ref.saastamoinen(math.pi / 2, lat, 0.0, p)) < 2.5


@pytest.mark.parametrize("which", ["north", "south"])
def test_reference_recovers_truth_through_the_atmosphere(which):
    """atm_ref alone: corrected fixes on truth_tx_atm observations land within 1e-6 m of the receiver (the model's own residue
    after three rounds, re-measured here), the plain nav_ref.fix on the same observations is metres off"""
    geo = geometry(which)
    p = atm_ref.params(elev_mask=-math.pi / 2)  # the mask has its own tests: here every chosen satellite counts
    ref_ms = (geo["ref_ms"] + np.array([0, 1, 40000], np.int64)) % nav_ref.WEEK_MS
    t_rx = np.array([0.137e-3, 0.55e-3, 0.9e-3])
    ms, frac = atm_ref.truth_times(geo["ephs"], geo["rx"], ref_ms, t_rx, p)
    for sats in (5, 8, 12):
        sel = geo["subsets"][sats]  # 12: all of them, those below the horizon (no delay: el <= 0) included
        worst, plain_worst, delays = 0.0, 1e9, []
        for k in range(len(t_rx)):
            out = atm_ref.fix_atm(geo["ephs"], sel, ms[k, sel], frac[k, sel], np.ones(len(sel)), p)
            assert out["status"] == 0 and out["n_masked"] == 0 and len(out["stages"]) == 4
            worst = max(worst, np.linalg.norm(out["xyz"] - geo["rx"]))
            dt = float(nav_ref.fold_ms(out["rx_ms"] - int(ref_ms[k]))) * 1e-3 + out["rx_frac"] - t_rx[k]
            assert abs(dt) < 1e-12
            plain = nav_ref.fix(geo["ephs"], sel, ms[k, sel], frac[k, sel], np.ones(len(sel)))
            plain_worst = min(plain_worst, np.linalg.norm(plain["xyz"] - geo["rx"]))
            delays.append(out["delay"])
        print("%s %d satellites: corrected %.3g m, plain %.3g m from the receiver; delays %.2f .. %.2f m" %
              (which, len(sel), worst, plain_worst, np.min(delays), np.max(delays)))
        assert worst < 1e-6 and plain_worst > 5.0
