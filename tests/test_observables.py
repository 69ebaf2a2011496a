"""Observables on the host: the model of include/gpsacq.h ("Observables") checked against itself two independent ways
(tests/obs_ref.py's backward recursion against its forward simulator; the exact slope of the transmit time), and
gpsacq_time_tag_from_subframe by hand.  Needs the library, no GPU."""
import ctypes
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import obs_ref

pytestmark = pytest.mark.usefixtures("hip_artifacts")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gpsacq_time_tag_from_subframe", "gpsacq_observables", "gpsacq_observables_device", "gpsacq_fix_track_device",
               "gpsacq_observables_last_ms")


def test_struct_sizes_and_exports(tmp_path):
    import gpsacq
    src = tmp_path / "sizes.c"
    src.write_text('#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_time_tag) == %d, "tag");\n'
                   '_Static_assert(sizeof(gpsacq_obs) == %d, "obs");\n'
                   '_Static_assert(sizeof(gpsacq_track_record) == 40 && sizeof(gpsacq_track_chan) == 160, "tracking structs keep their size");\n'
                   '_Static_assert(sizeof(gpsacq_subframe) == 56 && sizeof(gpsacq_fix) == 80 && sizeof(gpsacq_ephemeris) == 192, "nav structs");\n'
                   % (gpsacq.TIME_TAG_DTYPE.itemsize, gpsacq.OBS_DTYPE.itemsize))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert (gpsacq.TIME_TAG_DTYPE.itemsize, gpsacq.OBS_DTYPE.itemsize) == (16, 32)
    assert gpsacq.TIME_TAG_DTYPE.names == ("epoch", "ms", "eph", "valid")
    lib = gpsacq.load_library()
    for name in NEW_SYMBOLS:
        assert name in gpsacq.EXPORTS and hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", gpsacq.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert " T %s\n" % name in out, name
    for name in ("observables", "observables_device", "fix_track_device", "observables_last_ms"):
        assert callable(getattr(gpsacq.Engine, name))


@pytest.mark.parametrize("spm,n", [(2800, 1), (2800, 300), (5456, 1000), (16368, 257)])
def test_backward_recursion_reproduces_the_forward_simulator(spm, n):
    rec, ch, walk = obs_ref.fabricate(spm + n, n, spm)
    pos = obs_ref.code_positions(rec["sample"], rec["ca_rate"], ch["next_sample"][0], ch["ca_pos"][0])
    assert pos == walk
    assert all(0 <= p < obs_ref.PERIOD for p in pos)
    assert len(set(rec["ca_rate"])) > min(n, 2) - 1  # the rate did move
    # and every sample of an epoch keeps the prompt position inside the code period (the model's n = ceil(...))
    for t in (0, n // 2, n - 1):
        end = int(rec["sample"][t + 1]) if t + 1 < n else int(ch["next_sample"][0])
        for R in (int(rec["sample"][t]), end - 1):
            tt, P = obs_ref.position_at(rec["sample"], rec["ca_rate"], ch["next_sample"][0], pos, R)
            assert tt == t and P < obs_ref.PERIOD
    assert obs_ref.position_at(rec["sample"], rec["ca_rate"], ch["next_sample"][0], pos, int(rec["sample"][0]) - 1) is None
    assert obs_ref.position_at(rec["sample"], rec["ca_rate"], ch["next_sample"][0], pos, int(ch["next_sample"][0])) is None


@pytest.mark.parametrize("spm", [2800, 5456])
def test_exact_slope_at_constant_rate(spm):
    """at constant ca_rate the transmit time is a straight line in the receive sample, exactly: tx(R) - tx(R0) =
    (R - R0) ca_rate / (2^32 1023) ms as fractions, before the final division"""
    n = 200
    rec, ch, _ = obs_ref.fabricate(5, n, spm, rate_span_hz=0.0)
    rate = int(rec["ca_rate"][0])
    assert (rec["ca_rate"] == rate).all()
    smp, nxt = rec["sample"], int(ch["next_sample"][0])
    pos = obs_ref.code_positions(smp, rec["ca_rate"], nxt, ch["ca_pos"][0])

    def tx(R):  # milliseconds since the start of record 0's epoch
        t, P = obs_ref.position_at(smp, rec["ca_rate"], nxt, pos, R)
        return t + Fraction(P, obs_ref.PERIOD)

    R0 = int(smp[0])
    for R in (R0 + 1, int(smp[1]) - 1, int(smp[1]), int(smp[100]) + 17, nxt - 1):
        assert tx(R) - tx(R0) == Fraction((R - R0) * rate, obs_ref.PERIOD), R


def _tag(tow, bit_offset, bit_epoch0, eph_index, sf_id=1):
    import gpsacq
    sf = np.zeros(1, gpsacq.SUBFRAME_DTYPE)
    sf["tow"], sf["bit_offset"], sf["id"] = tow, bit_offset, sf_id
    t = gpsacq.time_tag(sf[0], bit_epoch0, eph_index)
    assert t.dtype == gpsacq.TIME_TAG_DTYPE and t.shape == (1,)
    return tuple(int(t[k][0]) for k in t.dtype.names)


def test_time_tag_by_hand():
    assert _tag(1, 0, 0, 0) == (0, 0, 0, 1)
    assert _tag(0, 0, 0, 3) == (0, 604_794_000, 3, 1)
    assert _tag(100799, 0, 0, 11) == (0, 604_788_000, 11, 1)
    assert _tag(2, 299, 17, 5) == (17 + 20 * 299, 6000, 5, 1)
    assert _tag(41878, 0, 17, 0) == (17, 41877 * 6000, 0, 1)
    assert _tag(41878, 299, 0, 0) == (5980, 41877 * 6000, 0, 1)
    for tow in (0, 1, 2, 50400, 100799):
        for off in (0, 299):
            for e0 in (0, 17):
                assert _tag(tow, off, e0, 7) == obs_ref.time_tag(tow, off, e0, 7)


def test_time_tags_of_the_2011_subframes_are_6000_ms_apart(golden_dir):
    import gpsacq
    d = json.load(open(os.path.join(golden_dir, "holme_nav_2011.json")))
    bits = np.array([int(c) for c in "".join(d["bits"])], np.uint8)
    sf, nfail = gpsacq.nav_subframes(bits)
    assert nfail == 0 and len(sf) == 10
    tags = np.concatenate([gpsacq.time_tag(s, 1234, 2) for s in sf])
    assert (np.diff(tags["ms"]) == 6000).all() and (np.diff(tags["epoch"]) == 6000).all()
    assert tags["epoch"][0] == 1234 + 20 * sf["bit_offset"][0] and tags["ms"][0] == (int(sf["tow"][0]) - 1) * 6000
    assert (tags["eph"] == 2).all() and (tags["valid"] == 1).all()
    # every tag of a channel names the same line: ms - epoch is one number
    assert len(set(tags["ms"] - tags["epoch"])) == 1


def test_time_tag_errors():
    import gpsacq
    lib = gpsacq.load_library()
    sf = np.zeros(1, gpsacq.SUBFRAME_DTYPE)
    tag = np.full(1, 0x5A5A5A5A, np.int32).repeat(4).view(gpsacq.TIME_TAG_DTYPE)
    before = tag.tobytes()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for tow in (-1, 100800, 1 << 17):
        sf["tow"] = tow
        assert lib.gpsacq_time_tag_from_subframe(p(sf), 0, 0, p(tag)) == 1
        assert b"TOW" in lib.gpsacq_last_error()
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            gpsacq.time_tag(sf[0], 0, 0)
        assert ei.value.code == 1
    sf["tow"] = 5
    assert lib.gpsacq_time_tag_from_subframe(None, 0, 0, p(tag)) == 1
    assert lib.gpsacq_time_tag_from_subframe(p(sf), 0, 0, None) == 1
    assert tag.tobytes() == before
    assert lib.gpsacq_time_tag_from_subframe(p(sf), 0, 0, p(tag)) == 0 and tag["ms"][0] == 24000


def test_observables_argument_errors_need_no_device():
    """every argument error is found before the engine is touched: a NULL engine among them"""
    import gpsacq
    lib = gpsacq.load_library()
    rec, ch, _ = obs_ref.fabricate(1, 8, 2800)
    ne = np.array([8], np.int32)
    tag = np.zeros(1, gpsacq.TIME_TAG_DTYPE)
    obs = np.full(4 * 32, 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpsacq_observables(None, p(rec), 8, p(ne), p(ch), p(tag), 1, 0, 1, 4, p(obs)) == 1
    assert lib.gpsacq_observables_device(None, p(rec), 8, p(ne), p(ch), p(tag), 1, 0, 1, 4, p(obs), 1) == 1
    assert lib.gpsacq_fix_track_device(None, None, 0, p(rec), 8, p(ne), p(ch), p(tag), 1, 0, 1, 4, None, p(obs), 1) == 1
    assert lib.gpsacq_observables_last_ms(None, None, None) == 1
    assert (obs == 0xA5).all()
