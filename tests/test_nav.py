"""NAV data decoding on the host (gpsacq_nav_subframes, gpsacq_nav_bits): the ten subframes a real receiver printed in
2011 ("Homemade GPS Receiver", section "NAV data"), inverted streams, single-bit errors, synthetic subframes and bit sync.
Needs the library, no GPU."""
import json
import os

import numpy as np
import pytest

from track_helpers import encode_subframe, make_subframe_words, nav_stream

pytestmark = pytest.mark.usefixtures("hip_artifacts")


@pytest.fixture(scope="module")
def holme(golden_dir):
    d = json.load(open(os.path.join(golden_dir, "holme_nav_2011.json")))
    bits = np.array([int(c) for c in "".join(d["bits"])], np.uint8)
    assert bits.size == 3000
    return bits, d["ids"], d["tows"]


def test_2011_subframes_decode(holme):
    import gpsacq
    bits, ids, tows = holme
    assert ids == [1, 2, 3, 4, 5] * 2 and tows == list(range(41871, 41881))
    sf, nfail = gpsacq.nav_subframes(bits)
    assert nfail == 0
    assert list(sf["id"]) == ids and list(sf["tow"]) == tows
    assert list(sf["bit_offset"]) == list(range(0, 3000, 300)) and not sf["inverted"].any()
    assert all(w >> 16 == 0x8B for w in sf["words"][:, 0])  # TLM preamble, decoded


def test_2011_subframes_inverted(holme):
    import gpsacq
    bits, ids, tows = holme
    up, _ = gpsacq.nav_subframes(bits)
    sf, nfail = gpsacq.nav_subframes(1 - bits)
    assert nfail == 0 and list(sf["id"]) == ids and list(sf["tow"]) == tows
    assert sf["inverted"].all()
    assert np.array_equal(sf["words"], up["words"])


def test_2011_single_bit_errors_are_parity_failures(holme):
    import gpsacq
    bits, ids, _ = holme
    rng = np.random.default_rng(5)
    for s in range(10):
        for w in range(10):
            k = int(rng.integers(8 if w == 0 else 0, 30))  # a bit of word w of subframe s (not the preamble itself)
            b = bits.copy()
            b[300 * s + 30 * w + k] ^= 1
            sf, nfail = gpsacq.nav_subframes(b)
            assert nfail >= 1, (s, w, k)
            assert 300 * s not in [int(o) for o in sf["bit_offset"]] and len(sf) <= 9


def test_synthetic_subframes_round_trip():
    import gpsacq
    bits, meta = nav_stream(100000, 12, seed=3)
    pre = np.random.default_rng(0).integers(0, 2, 137).astype(np.uint8)  # junk before the first preamble
    sf, nfail = gpsacq.nav_subframes(np.concatenate([pre, bits]))
    found = [(int(a), int(b)) for a, b in zip(sf["id"], sf["tow"])]
    assert found[-12:] == meta
    assert list(sf["bit_offset"][-12:]) == [137 + 300 * k for k in range(12)]
    # the payload words come back
    rng = np.random.default_rng(9)
    words = make_subframe_words(4321, 3, rng)
    b, _, _ = encode_subframe(words)
    sf, nfail = gpsacq.nav_subframes(np.array(b, np.uint8))
    assert nfail == 0 and len(sf) == 1 and sf["tow"][0] == 4321 and sf["id"][0] == 3
    assert list(sf["words"][0][[0, 2, 3, 4, 5, 6, 7, 8]]) == [words[i] for i in (0, 2, 3, 4, 5, 6, 7, 8)]


def _ip_sequence(nav, offset, amp, noise, rng, n_epochs):
    """prompt I of epochs 0..n-1: bit k covers epochs offset + 20 k .. offset + 20 k + 19 (epochs before offset: bit -1)"""
    e = np.arange(n_epochs)
    k = np.floor_divide(e - offset, 20)
    s = np.where(nav[np.mod(k, nav.size)] > 0, 1.0, -1.0)
    return np.round(amp * s + noise * rng.standard_normal(n_epochs)).astype(np.int32)


@pytest.mark.parametrize("offset", [0, 7, 13, 19])
def test_bit_sync(offset):
    import gpsacq
    rng = np.random.default_rng(offset)
    nav = rng.integers(0, 2, 60).astype(np.int8) * 2 - 1
    ip = _ip_sequence(nav, offset, 400, 120, rng, 1200)
    bits, e0 = gpsacq.nav_bits(ip, first_epoch=0, sync_epochs=1000)
    assert e0 == offset
    want = (nav[(np.arange(bits.size))] < 0).astype(np.uint8)
    assert np.array_equal(bits, want)
    # the same stream seen from a later first epoch keeps the channel's bit boundaries
    bits2, e02 = gpsacq.nav_bits(ip[45:], first_epoch=45, sync_epochs=0)
    assert (e02 - offset) % 20 == 0 and e02 >= 45


def test_bit_sync_none():
    import gpsacq
    rng = np.random.default_rng(1)
    bits, e0 = gpsacq.nav_bits(np.round(300 * rng.standard_normal(2000)).astype(np.int32))
    assert e0 == -1 and bits.size == 0
    bits, e0 = gpsacq.nav_bits(np.full(500, 300, np.int32))  # no sign change at all
    assert e0 == -1 and bits.size == 0


def test_track_struct_sizes(tmp_path):
    """the binding's records match the C structs of include/gpsacq.h (checked by the C compiler itself)"""
    import ctypes
    import subprocess
    import gpsacq
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_track_chan) == %d, "chan");\n'
                   '_Static_assert(sizeof(gpsacq_track_params) == %d, "params");\n'
                   '_Static_assert(sizeof(gpsacq_track_record) == %d, "record");\n'
                   '_Static_assert(sizeof(gpsacq_subframe) == %d, "subframe");\n'
                   % (gpsacq.TRACK_CHAN_DTYPE.itemsize, ctypes.sizeof(gpsacq.TrackParams), gpsacq.TRACK_RECORD_DTYPE.itemsize,
                      gpsacq.SUBFRAME_DTYPE.itemsize))
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(root, "include"), str(src)], check=True)
    assert (gpsacq.TRACK_CHAN_DTYPE.itemsize, ctypes.sizeof(gpsacq.TrackParams), gpsacq.TRACK_RECORD_DTYPE.itemsize,
            gpsacq.SUBFRAME_DTYPE.itemsize) == (160, 72, 40, 56)
