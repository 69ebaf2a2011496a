#!/usr/bin/env python3
"""Tracking-channel benchmark (gpsacq_track_device): a Nottingham-size capture made on the device (fs 5.456 MHz, IF 4.092 MHz,
81.8 s = 446 M samples) with 32 satellites carrying parity-valid NAV subframes, amplitudes 0.08-0.2 at sigma = 1; the first run
is searched, a channel started for every hit with SNR > 25, everything tracked in ONE call, the subframes decoded and checked.
Prints one JSON line: wall time of the tracking call, epochs per second summed over channels, real-time factor, subframes found
and wrong, parity failures, and (unless --no-prof) the k_track time of a `rocprofv3 --kernel-trace --stats` run of this same
script in a child process.

    python tools/track_bench.py [--secs 81.8] [--no-prof]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(secs):
    import ctypes

    import numpy as np
    import torch

    import gpsacq
    from track_helpers import nav_stream

    fs, fc = 5.456e6, 4.092e6
    rng = np.random.default_rng(2024)
    sats, navs, metas = [], [], []
    for prn in range(1, 33):
        sats.append((prn, float(rng.uniform(0.08, 0.2)), float(rng.uniform(-4500, 4500)), float(rng.uniform(0, 5456)), float(rng.uniform(0, 1))))
        b, meta = nav_stream(1000 * prn, 15, seed=prn)  # 15 subframes = 90 s, longer than the capture; TOW < 2^17
        navs.append(np.where(b > 0, -1, 1).astype(np.int8))
        metas.append(meta)
    nav = np.ascontiguousarray(np.array(navs))
    n_bytes = int(secs * fs) // 8
    eng = gpsacq.Engine(fc, fs, 5000.0, device=0)
    d_bits = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0")
    arr = eng._sats(sats)
    t0 = time.time()
    rc = eng._lib.gpsacq_generate_nav_range_device(eng._h, d_bits.data_ptr(), n_bytes, 0, arr, len(sats), nav.ctypes.data_as(ctypes.c_void_p),
                                                   nav.shape[1], ctypes.c_float(1.0), 7, 1)
    gpsacq._check(eng._lib, rc)
    gen_s = time.time() - t0
    head = d_bits[:32 * gpsacq.BLOCK_BYTES].cpu().numpy()
    _, peaks = eng.search(head, want_cells=False)
    chans = [eng.track_start(b % 32 + 1, peaks[b], b * gpsacq.BLOCK_BYTES * 8) for b in range(32) if peaks["snr"][b] > 25]
    ch = np.concatenate(chans)
    max_epochs = int(secs * 1000) + 10
    d_prompt = torch.zeros((ch.size, max_epochs, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.time()
    ne = eng.track_device(d_bits.data_ptr(), n_bytes, ch, 0, max_epochs, d_prompt.data_ptr(), None)
    wall = time.time() - t0
    prompt = d_prompt.cpu().numpy()
    found = wrong = pfail = 0
    for c in range(ch.size):
        prn = int(ch["prn"][c])
        n = int(ne[c])
        bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=int(ch["epoch"][c]) - n + 1000)
        sf, _ = gpsacq.nav_subframes(bits)
        if len(sf):  # parity failures counted from the first subframe on (before it, payload bits can mimic a preamble)
            sf, nf = gpsacq.nav_subframes(bits[int(sf["bit_offset"][0]):])
            pfail += nf
        for a, t in zip(sf["id"], sf["tow"]):
            found += 1
            wrong += (int(a), int(t)) not in metas[prn - 1]
    epochs = int(ne.sum())
    out = {"metric": "track", "secs": secs, "samples": n_bytes * 8, "channels": int(ch.size), "lost": int((ch["status"] != 0).sum()),
           "epochs": epochs, "track_wall_s": round(wall, 4), "epochs_per_s": round(epochs / wall, 1), "realtime_x": round(secs / wall, 1),
           "subframes": found, "subframes_wrong": wrong, "parity_failures": pfail, "generate_s": round(gen_s, 3),
           "device": eng.device_name}
    eng.close()
    return out


def kernel_time(secs):
    """k_track's time from a rocprofv3 --kernel-trace --stats run of this script (child process, --no-prof)."""
    d = tempfile.mkdtemp(prefix="track_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--secs", str(secs), "--no-prof"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"prof_error": r.returncode}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_track" in row.get("Name", ""):
                return {"kernel_ms": round(float(row["TotalDurationNs"]) / 1e6, 3), "kernel_calls": int(row["Calls"])}
    return {"prof_error": "no k_track row"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--secs", type=float, default=81.8)
    ap.add_argument("--no-prof", action="store_true")
    a = ap.parse_args()
    out = run(a.secs)
    if not a.no_prof:
        out.update(kernel_time(a.secs))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
