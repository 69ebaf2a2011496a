#!/usr/bin/env python3
"""The noise floor of the aided search, measured on the CPU: where gpsacq_aided_default_params' ratio_min comes from
(include/gpsacq.h, "Aided acquisition", DEFAULT RATIO_MIN).

The scene is tools/snapshot_bench.py's: the northern receiver's eight satellites at amplitude 0.2, noise sigma 1, fs = 5.456 MHz,
made sample by sample with tests/gen_ref.py.  tests/aided_ref.py searches it for PRNs that are NOT in it, with the defaults
(16 blocks, W = 16, K = 1): every draw is one (window start, lo_center, absent PRN, ca_center), and its figure is the record's
ratio = best / floor over its 99 hypotheses.  C/A cross-correlation with the eight strong satellites is part of what is measured.
Prints one JSON line: the draw count, the largest ratio, and the default it gives (largest + a quarter of its excess over 1).

    python tools/aided_floor.py [--windows 8] [--centers 6] [--procs 8] [--coherent] [--iq8]

--coherent: the same draws for gpsacq_aided_coh_search ("Coherent aided acquisition", DEFAULT RATIO_MIN) with its defaults (20 ms
sums, 7 fine Dopplers 25/1024 cycle per segment apart, 20 bit edges: 13 860 hypotheses a draw), by tests/aided_coh_ref.py, on the
same scene with random navigation bits on its eight satellites (16 per satellite, repeated).

--iq8: the same draws for the multi-bit path of gpsacq_aided_search_iq8 ("Aided acquisition on an 8-bit IQ capture", DEFAULT
RATIO_MIN), by tests/aided_iq_ref.py against its measured floor: the same satellites written as an 8-bit IQ capture with
tests/gen_ref.py's generator as tools/snapshot_bench.py --iq8 has it (int8, scale 16, sigma 1, IF 0.4 MHz, the mean not removed,
GPSACQ_SAMPLES_REAL with mix_hz = fc - IF).

--iq8 --coherent: the same draws for the multi-bit path of gpsacq_aided_coh_search_iq8 ("Coherent aided acquisition on an 8-bit IQ
capture", DEFAULT RATIO_MIN) with --coherent's defaults, by tests/aided_coh_iq_ref.py's quick spellings against the measured
floor: --iq8's capture with --coherent's navigation bits.
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, FC, SPM, BLOCK_BYTES = 5.456e6, 4.092e6, 5456, 5120
BLOCKS, W, K = 16, 16, 1
KMAX = 36  # the reference grid of +-5 kHz in bins of fs / 40000

_scene = {}


def scene(n_blocks, seed):
    """the capture as 0/1 samples, and the PRNs in it"""
    import numpy as np

    import gen_ref
    from coarse_helpers import synth_sats
    from nav_helpers import geometry
    geo = geometry("north")
    sel = geo["subsets"][8]
    sats, _ = synth_sats(geo, sel, geo["ref_ms"] + 4321, 0.6180e-3, 0, FS, 0.2)
    n = n_blocks * BLOCK_BYTES * 8
    y = np.concatenate([gen_ref.LAW.bits(FC, FS, sats, 1.0, seed, a, min(gen_ref.MAX_SAMPLES, n - a))["y"] for a in range(0, n, gen_ref.MAX_SAMPLES)])
    return (y < 0.0).astype(np.uint8), [s[0] for s in sats]


def work(job):
    """every (absent PRN, ca_center) of one (window start, lo_center): the carriers are made once"""
    import numpy as np

    import aided_ref
    block, lo_center, prns, centers, n_blocks, seed = job
    if "s01" not in _scene:
        _scene["s01"], _ = scene(n_blocks, seed)
    s01 = _scene["s01"]
    o = block * BLOCK_BYTES * 8
    segments = BLOCKS * 40000 // SPM
    rates, carriers = [], []
    j = np.arange(segments * SPM, dtype=np.int64)
    for d in range(2 * K + 1):
        ok, lo_rate, ca_rate = aided_ref.nco_words(lo_center - K + d, FC, FS)
        assert ok and abs(lo_center - K + d) <= KMAX
        rates.append((True, lo_rate, ca_rate))
        carriers.append(aided_ref.carrier_pm((j * lo_rate) % aided_ref.TWO32))
    floor = aided_ref.LAW.floor_of(SPM, segments)
    out = []
    for prn in prns:
        for ca in centers:
            pw = aided_ref.LAW.powers_stream(s01, o, segments, SPM, prn, aided_ref.LAW.base_of(ca, W, SPM), 2 * W + 1, rates, carriers)
            out.append(max(max(r) for r in pw) / floor)
    return out


COH = dict(min_segments=20, coh_ms=20, fine_half=3, fine_step=25)  # gpsacq_aided_coh_default_params beside BLOCKS, W, K
NAV_BITS, NAV_SEED = 16, 5


def scene_nav(n_blocks, seed):
    """scene() with random navigation bits, NAV_BITS per satellite (repeated), on the eight satellites"""
    import numpy as np

    import gen_ref
    from coarse_helpers import synth_sats
    from nav_helpers import geometry
    geo = geometry("north")
    sel = geo["subsets"][8]
    sats, _ = synth_sats(geo, sel, geo["ref_ms"] + 4321, 0.6180e-3, 0, FS, 0.2)
    nav = (1 - 2 * np.random.default_rng(NAV_SEED).integers(0, 2, (len(sats), NAV_BITS))).astype(np.int8)
    n = n_blocks * BLOCK_BYTES * 8
    y = np.concatenate([gen_ref.LAW.bits(FC, FS, sats, 1.0, seed, a, min(gen_ref.MAX_SAMPLES, n - a), nav=nav)["y"]
                        for a in range(0, n, gen_ref.MAX_SAMPLES)])
    return (y < 0.0).astype(np.uint8), [s[0] for s in sats]


def work_coherent(job):
    """work() for gpsacq_aided_coh_search with its defaults: tests/aided_coh_ref.py on the scene with navigation bits"""
    import numpy as np

    import aided_coh_ref
    import aided_ref
    block, lo_center, prns, centers, n_blocks, seed = job
    if "nav01" not in _scene:
        _scene["nav01"], _ = scene_nav(n_blocks, seed)
    s01 = _scene["nav01"]
    o = block * BLOCK_BYTES * 8
    segments = BLOCKS * 40000 // SPM
    rates, carriers = [], []
    j = np.arange(segments * SPM, dtype=np.int64)
    for d in range(2 * K + 1):
        ok, lo_rate, ca_rate = aided_ref.nco_words(lo_center - K + d, FC, FS)
        assert ok and abs(lo_center - K + d) <= KMAX
        rates.append((True, lo_rate, ca_rate))
        carriers.append(aided_ref.carrier_pm((j * lo_rate) % aided_ref.TWO32))
    floor = 2 * SPM * segments
    out = []
    for prn in prns:
        for ca in centers:
            z = aided_coh_ref.segment_sums(s01, o, segments, SPM, prn, (ca - W) % SPM, 2 * W + 1, rates, carriers)
            best = max(int(np.array(aided_coh_ref.LAW.powers(zi, zq, COH["fine_half"], COH["fine_step"], COH["coh_ms"]), dtype=np.uint64).max())
                       for zi, zq in z)
            out.append(best / floor)
    return out


IF_HZ, SCALE = 0.4e6, 16.0  # tools/snapshot_bench.py --iq8


def scene_iq8(n_blocks, seed, with_nav=False):
    """scene() as interleaved int8 I, Q bytes; with_nav: scene_nav()'s navigation bits on the eight satellites"""
    import numpy as np

    import gen_ref
    from coarse_helpers import synth_sats
    from nav_helpers import geometry
    geo = geometry("north")
    sel = geo["subsets"][8]
    sats, _ = synth_sats(geo, sel, geo["ref_ms"] + 4321, 0.6180e-3, 0, FS, 0.2)
    nav = (1 - 2 * np.random.default_rng(NAV_SEED).integers(0, 2, (len(sats), NAV_BITS))).astype(np.int8) if with_nav else None
    n = n_blocks * BLOCK_BYTES * 8
    return np.concatenate([gen_ref.LAW.quantise(gen_ref.LAW.iq8(FS, sats, IF_HZ, SCALE, 1.0, seed, a, min(gen_ref.MAX_SAMPLES, n - a), nav=nav)["v"],
                                                True).ravel() for a in range(0, n, gen_ref.MAX_SAMPLES)])


def work_iq8(job):
    """work() for the multi-bit path of gpsacq_aided_search_iq8: tests/aided_iq_ref.py's quick spelling and its floor law"""
    import aided_iq_ref
    import refine_iq_ref
    block, lo_center, prns, centers, n_blocks, seed = job
    if "iq" not in _scene:
        _scene["iq"] = refine_iq_ref.samples(scene_iq8(n_blocks, seed), True)
    vi, vq = _scene["iq"]
    o = block * BLOCK_BYTES * 8
    segments = BLOCKS * 40000 // SPM
    law = aided_iq_ref.LAW
    rates = [aided_iq_ref.nco_words(lo_center - K + d, FC, FS, FC - IF_HZ, aided_iq_ref.REAL, KMAX) for d in range(2 * K + 1)]
    assert all(r[0] for r in rates)
    floor = law.floor_of(vi, vq, o, segments, SPM)
    out = []
    for prn in prns:
        for ca in centers:
            pw = law.powers_stream(vi, vq, o, segments, SPM, prn, law.base_of(ca, W, SPM), 2 * W + 1, rates)
            out.append(max(max(r) for r in pw) / floor)
    return out


def work_iq8_coherent(job):
    """work_iq8() for the multi-bit path of gpsacq_aided_coh_search_iq8 with its defaults: tests/aided_coh_iq_ref.py's quick
    spellings on the capture with navigation bits, against the measured floor"""
    import aided_coh_iq_ref
    import aided_iq_ref
    import refine_iq_ref
    block, lo_center, prns, centers, n_blocks, seed = job
    if "iqnav" not in _scene:
        _scene["iqnav"] = refine_iq_ref.samples(scene_iq8(n_blocks, seed, True), True)
    vi, vq = _scene["iqnav"]
    o = block * BLOCK_BYTES * 8
    segments = BLOCKS * 40000 // SPM
    law = aided_coh_iq_ref.LAW
    rates = [aided_iq_ref.nco_words(lo_center - K + d, FC, FS, FC - IF_HZ, aided_iq_ref.REAL, KMAX) for d in range(2 * K + 1)]
    assert all(r[0] for r in rates)
    floor = law.floor_of(vi, vq, o, segments, SPM)
    out = []
    for prn in prns:
        for ca in centers:
            z = law.segment_sums_stream(vi, vq, o, segments, SPM, prn, law.base_of(ca, W, SPM), 2 * W + 1, rates)
            best = max(max(max(max(row) for row in rows) for rows in law.powers_quick(zi, zq, COH["fine_half"], COH["fine_step"], COH["coh_ms"]))
                       for zi, zq in z)
            out.append(best / floor)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coherent", action="store_true", help="the floor of gpsacq_aided_coh_search (20 ms sums, 7 fine Dopplers, 20 edges) "
                    "on the scene with navigation bits")
    ap.add_argument("--iq8", action="store_true", help="the floor of the multi-bit path of gpsacq_aided_search_iq8 on the scene as an 8-bit IQ capture")
    ap.add_argument("--windows", type=int, default=8, help="window starts: blocks 0 .. windows - 1")
    ap.add_argument("--centers", type=int, default=6, help="lo_center values, spread over the grid")
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=77)
    a = ap.parse_args()
    import numpy as np
    n_blocks = a.windows + BLOCKS - 1
    _, present = scene(1, a.seed)
    absent = [p for p in range(1, 33) if p not in present]
    los = np.linspace(-KMAX + K, KMAX - K, a.centers).round().astype(int).tolist()
    rng = np.random.default_rng(a.seed)
    jobs = [(b, lo, absent, rng.integers(0, SPM, 2).tolist(), n_blocks, a.seed) for b in range(a.windows) for lo in los]
    with multiprocessing.Pool(a.procs) as pool:
        ratios = np.array([r for rows in pool.map(work_iq8_coherent if a.coherent and a.iq8 else work_coherent if a.coherent else work_iq8 if a.iq8 else work, jobs) for r in rows])
    worst = float(ratios.max())
    extra = dict(COH, coherent=True, nav_bits=NAV_BITS, nav_seed=NAV_SEED) if a.coherent else {}
    if a.iq8:
        extra.update(iq8=True, if_hz=IF_HZ, scale=SCALE)
    print(json.dumps({"draws": int(ratios.size), "absent_prns": len(absent), "windows": a.windows, "lo_centers": los, "blocks": BLOCKS, "W": W, "K": K,
                      **extra, "ratio_max": round(worst, 4), "ratio_median": round(float(np.median(ratios)), 4),
                      "ratio_p999": round(float(np.percentile(ratios, 99.9)), 4), "ratio_min_default": round(worst + 0.25 * (worst - 1.0), 4)}))


if __name__ == "__main__":
    main()
