#!/usr/bin/env python3
"""The gate of the snapshot signal quality on an 8-bit IQ capture, measured on the CPU: where
gpsacq_snap_quality_default_params_iq8's cn0_min_lin comes from (include/gpsacq.h, "Snapshot signal quality on an 8-bit IQ capture",
PARAMETERS).

The scene is tools/aided_floor.py --iq8's: the northern receiver's eight satellites at amplitude 0.2, noise sigma 1, fs = 5.456 MHz,
written as an 8-bit IQ capture (int8, scale 16, IF 0.4 MHz, the mean not removed) by tests/gen_ref.py.  Every draw is ONE hypothesis
of a PRN that is NOT in the capture: a window start, a Doppler bin, an absent PRN and a random code phase; its figure is
    lin = (prompt - floor) / floor * fs / spm        (0 where prompt <= floor)
with the prompt power of tests/refine_iq_ref.py's law (16 blocks, GPSACQ_SAMPLES_REAL, mix_hz = fc - IF) and the measured floor of
tests/snapq_iq_ref.py over the same window.  C/A cross-correlation with the eight strong satellites is part of what is measured.
Prints one JSON line: the draw count, the largest lin, and the default it gives (the larger of 500.0 and the largest plus a quarter
of it).

    python tools/snap_quality_floor.py [--windows 8] [--centers 6] [--phases 2] [--procs 8]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import aided_floor as af  # noqa: E402  (the scene and its constants)

_scene = {}


def work(job):
    """every (absent PRN, code phase) of one (window start, bin): the carrier-wiped series is made once"""
    import numpy as np

    import refine_iq_ref
    import snapq_iq_ref
    import track_ref
    block, lo_shift, prns, shifts, n_blocks, seed = job
    if "iq" not in _scene:
        _scene["iq"] = refine_iq_ref.samples(af.scene_iq8(n_blocks, seed), True)
    vi, vq = _scene["iq"]
    spm = af.SPM
    o = block * af.BLOCK_BYTES * 8
    segments = af.BLOCKS * 40000 // spm
    n = segments * spm
    law = refine_iq_ref.LAW
    ok, lo_rate, ca_rate, _, _ = refine_iq_ref.nco_words(lo_shift, af.FC, af.FS, af.FC - af.IF_HZ, refine_iq_ref.REAL)
    assert ok
    j = np.arange(n, dtype=np.int64)
    C, S = law.carrier((j * lo_rate) % refine_iq_ref.TWO32)
    re_, im_ = law.arms(vi[o:o + n], vq[o:o + n], C, S)
    floor = snapq_iq_ref.LAW.floor_of_window(vi, vq, o, n)
    out = []
    for prn in prns:
        c = track_ref.chips(prn)
        for ca in shifts:
            P = ((ca * ca_rate) % refine_iq_ref.FULL + j * ca_rate) % refine_iq_ref.FULL
            h = 1 - 2 * c[(P // refine_iq_ref.TWO32) % 1023].astype(np.int64)
            I = (h * re_).reshape(segments, spm).sum(axis=1).tolist()
            Q = (h * im_).reshape(segments, spm).sum(axis=1).tolist()
            prompt = sum(a * a + b * b for a, b in zip(I, Q))
            out.append((prompt - floor) / floor * af.FS / spm if prompt > floor else 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8, help="window starts: blocks 0 .. windows - 1")
    ap.add_argument("--centers", type=int, default=6, help="Doppler bins, spread over the grid")
    ap.add_argument("--phases", type=int, default=2, help="random code phases per (window, bin), shared by its absent PRNs")
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=77)
    a = ap.parse_args()
    import numpy as np
    n_blocks = a.windows + af.BLOCKS - 1
    _, present = af.scene(1, a.seed)
    absent = [p for p in range(1, 33) if p not in present]
    los = np.linspace(-af.KMAX, af.KMAX, a.centers).round().astype(int).tolist()
    rng = np.random.default_rng(a.seed)
    jobs = [(b, lo, absent, rng.integers(0, af.SPM, a.phases).tolist(), n_blocks, a.seed) for b in range(a.windows) for lo in los]
    with multiprocessing.Pool(a.procs) as pool:
        lin = np.array([r for rows in pool.map(work, jobs) for r in rows])
    worst = float(lin.max())
    print(json.dumps({"draws": int(lin.size), "absent_prns": len(absent), "windows": a.windows, "bins": los, "blocks": af.BLOCKS, "if_hz": af.IF_HZ,
                      "scale": af.SCALE, "lin_max_hz": round(worst, 2), "lin_median_hz": round(float(np.median(lin)), 2),
                      "lin_p999_hz": round(float(np.percentile(lin, 99.9)), 2), "cn0_min_lin_default": round(max(500.0, worst + 0.25 * worst), 1)}))


if __name__ == "__main__":
    main()
