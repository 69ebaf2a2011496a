"""Ephemeris decode on the host (gpsacq_ephemeris_load, gpsacq_ephemeris_valid) against tests/nav_ref.py's direct slice of the
ICD's bit numbers: the ten subframes a real receiver printed in 2011, and the synthetic constellation through encoder -> bit
stream -> gpsacq_nav_subframes -> load.  Needs the library, no GPU."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import nav_ref
from nav_helpers import assert_fields_exact, geometry

pytestmark = pytest.mark.usefixtures("hip_artifacts")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def holme_bits(golden_dir):
    d = json.load(open(os.path.join(golden_dir, "holme_nav_2011.json")))
    bits = np.array([int(c) for c in "".join(d["bits"])], np.uint8)
    assert bits.size == 3000
    return bits


@pytest.fixture(scope="module")
def constellation():
    return nav_ref.make_constellation(nav_ref.ecef_of(*nav_ref.RX_LLA))


def test_nav_struct_sizes(tmp_path):
    """the binding's records match the C structs (checked by the C compiler).  gpsacq_fix as include/gpsacq.h declares it --
    four int32 and eight doubles -- is 80 bytes; gpsacq_ephemeris, ten 32-bit fields and nineteen doubles, 192."""
    import gpsacq
    sizes = (gpsacq.OBS_DTYPE.itemsize, gpsacq.SAT_STATE_DTYPE.itemsize, gpsacq.FIX_DTYPE.itemsize, gpsacq.EPHEMERIS_DTYPE.itemsize)
    src = tmp_path / "sizes.c"
    src.write_text('#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_obs) == %d, "obs");\n'
                   '_Static_assert(sizeof(gpsacq_sat_state) == %d, "state");\n'
                   '_Static_assert(sizeof(gpsacq_fix) == %d, "fix");\n'
                   '_Static_assert(sizeof(gpsacq_ephemeris) == %d, "ephemeris");\n' % sizes)
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert sizes == (32, 32, 4 * 4 + 8 * 8, 10 * 4 + 19 * 8) == (32, 32, 80, 192)
    for dt in (gpsacq.OBS_DTYPE, gpsacq.SAT_STATE_DTYPE, gpsacq.FIX_DTYPE, gpsacq.EPHEMERIS_DTYPE):
        assert dt.itemsize == sum(dt[n].itemsize for n in dt.names)  # no padding anywhere


def test_2011_subframes_give_a_valid_ephemeris(holme_bits):
    import gpsacq
    sf, nfail = gpsacq.nav_subframes(holme_bits)
    assert nfail == 0 and len(sf) == 10
    eph = gpsacq.ephemeris(sf, 1)
    assert gpsacq.ephemeris_valid(eph[0]) and eph["have"][0] == 7 and eph["prn"][0] == 1
    ref, have = nav_ref.decode_subframes([holme_bits[300 * k:300 * k + 300] for k in range(10)])
    assert nav_ref.ephemeris_valid(ref, have)
    assert_fields_exact(eph, ref)
    assert eph["tow"][0] == ref["tow"] == 41878  # the last of subframes 1-3 in the stream: the second subframe 3
    assert eph["week"][0] == 597  # 1 Feb 2011 = week 1621 = 597 mod 1024
    assert abs(int(eph["t_oe"][0]) - 6 * int(eph["tow"][0])) < 4 * 3600
    assert 5150 < eph["sqrt_a"][0] < 5157 and eph["e"][0] < 0.03 and 0.9 < eph["i_0"][0] < 1.0
    # subframes 1 and 2 alone: not valid; the third, loaded into the same record later, completes it
    part = gpsacq.ephemeris(sf[:2], 1)
    assert part["have"][0] == 3 and not gpsacq.ephemeris_valid(part[0])
    assert gpsacq.ephemeris_valid(gpsacq.ephemeris(sf[2:3], 1, eph=part[0])[0])
    # subframes 4 and 5 change nothing
    assert gpsacq.ephemeris(sf[3:5], 1).tobytes() == gpsacq.ephemeris(sf[:0], 1).tobytes()


def _round_trip(eph, tow0=64900, invert=False, seed=7):
    import gpsacq
    bits = nav_ref.encode_stream(eph, tow0, ids=(1, 2, 3, 4, 5), seed=seed)
    if invert:
        bits = 1 - bits
    sf, nfail = gpsacq.nav_subframes(bits)
    assert nfail == 0 and list(sf["id"]) == [1, 2, 3, 4, 5] and bool(sf["inverted"].all()) == invert
    rec = gpsacq.ephemeris(sf, eph.get("prn", 1))
    assert rec["tow"][0] == tow0 + 2
    return rec


def test_round_trip_of_the_constellation(constellation):
    import gpsacq
    assert len(constellation) == 12
    for k, eph in enumerate(constellation):
        rec = _round_trip(eph, seed=k)
        assert gpsacq.ephemeris_valid(rec[0]) and rec["prn"][0] == k + 1
        assert_fields_exact(rec, eph)
        # and the reference's own decoder reads the same stream the same way
        bits = nav_ref.encode_stream(eph, 64900, seed=k)
        ref, have = nav_ref.decode_subframes([bits[300 * j:300 * j + 300] for j in range(5)])
        assert have == 7 and all(ref[n] == eph[n] for n in nav_ref.FIELDS)


def test_round_trip_negative_in_every_signed_field(constellation):
    import gpsacq
    eph = dict(constellation[0])
    for name in nav_ref.SIGNED_FIELDS:
        eph[name] = -abs(eph[name]) if eph[name] != 0 else nav_ref.value_of(name, -3)
    eph["a_f0"] = nav_ref.value_of("a_f0", -(1 << 21))  # the most negative code of the 22-bit field
    eph["idot"] = nav_ref.value_of("idot", -(1 << 13))  # and of the 14-bit one
    eph = nav_ref.quantise(eph)
    assert all(eph[name] < 0 for name in nav_ref.SIGNED_FIELDS)
    rec = _round_trip(eph)
    assert gpsacq.ephemeris_valid(rec[0])
    assert_fields_exact(rec, eph)


def test_iode_mismatch_is_not_valid(constellation):
    import gpsacq
    eph = dict(constellation[1], iode3=constellation[1]["iode2"] + 1)
    rec = _round_trip(eph)
    assert_fields_exact(rec, eph)
    assert rec["have"][0] == 7 and not gpsacq.ephemeris_valid(rec[0])
    # IODC: only its eight low bits are compared (the constellation's IODCs have bit 8 set); a zero issue number is not valid
    assert constellation[1]["iodc"] > 255
    zero = dict(constellation[1], iodc=0x100, iode2=0, iode3=0)
    assert not gpsacq.ephemeris_valid(_round_trip(zero)[0])


def test_round_trip_inverted_polarity(constellation):
    import gpsacq
    rec = _round_trip(constellation[2], invert=True)
    assert gpsacq.ephemeris_valid(rec[0])
    assert_fields_exact(rec, constellation[2])


def test_every_subset_the_fix_tests_use_has_pdop_below_6():
    """The figures test_gpu_fix.py's tolerances rest on (its docstring quotes them)."""
    for which in ("north", "south", "rollover"):
        geo = geometry(which)
        assert sum(e > 0 for e in geo["elevation"]) >= 8
        for name, sel in geo["subsets"].items():
            p = nav_ref.pdop(geo["rx"], geo["sat_xyz"][sel])
            print(which, name, sel, "PDOP %.2f" % p)
            assert p < 6.0, (which, name, p)
