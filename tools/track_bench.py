#!/usr/bin/env python3
"""Tracking-channel benchmark (gpsacq_track_device): a Nottingham-size capture made on the device (fs 5.456 MHz, IF 4.092 MHz,
81.8 s = 446 M samples) with 32 satellites carrying parity-valid NAV subframes, amplitudes 0.08-0.2 at sigma = 1; the first run
is searched, a channel started for every hit with SNR > 25, everything tracked in ONE call, the subframes decoded and checked.
Prints one JSON line: wall time of the tracking call, epochs per second summed over channels, real-time factor, subframes found
and wrong, parity failures, and (unless --no-prof) the k_track time of a `rocprofv3 --kernel-trace --stats` run of this same
script in a child process.

--input iq8: the same satellites as an 8-bit complex capture from gpsacq_generate_iq8_range (uint8, residual IF 250 kHz, scale 16;
the generator is zero-mean, so the mean handed over is 0), searched with gpsacq_search_iq8 (mixer fc - 250 kHz) and tracked with
gpsacq_track_iq8: in sign mode (the converter + k_track; "convert_ms" and "track_kernel_ms" are the two device times of the
call) or, with --multibit, by the multi-bit complex channels (k_track_iq).  The line carries an "input" field.

    python tools/track_bench.py [--secs 81.8] [--no-prof] [--input bits|iq8] [--multibit]
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


IF_HZ, SCALE = 250e3, 16.0


def run(secs, input_kind="bits", multibit=False):
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
    if input_kind == "iq8":
        return run_iq8(eng, secs, n_bytes * 8, sats, nav, metas, multibit)
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
    out = report(secs, n_bytes * 8, ch, ne, d_prompt.cpu().numpy(), metas, wall, gen_s, eng.device_name)
    out["input"] = "bits"
    eng.close()
    return out


def run_iq8(eng, secs, n_samples, sats, nav, metas, multibit):
    import numpy as np
    import torch

    import gpsacq

    d_iq = torch.empty(2 * n_samples, dtype=torch.uint8, device="cuda:0")
    t0 = time.time()
    eng.generate_iq8_device(d_iq.data_ptr(), n_samples, sats, if_hz=IF_HZ, scale=SCALE, signed=False, seed=7, nav=nav)
    gen_s = time.time() - t0
    head = d_iq[:32 * 16 * gpsacq.BLOCK_BYTES].cpu().numpy()
    inp = eng.iq8_input(signed=False, remove_dc=True, mean=(0.0, 0.0), mix_hz=eng.fc - IF_HZ, fs=eng.fs, total_samples=n_samples,
                        multibit=1 if multibit else 0)
    _, peaks = eng.search_iq8(head, inp, want_cells=False)
    params = eng.track_params_iq8(eng.iq8_rms(head, inp)) if multibit else eng.track_params()
    chans = [eng.track_start_iq8(inp, b % 32 + 1, peaks[b], b * gpsacq.BLOCK_BYTES * 8, params=params) for b in range(32) if peaks["snr"][b] > 25]
    ch = np.concatenate(chans)
    max_epochs = int(secs * 1000) + 10
    d_prompt = torch.zeros((ch.size, max_epochs, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.time()
    ne = eng.track_iq8_device(d_iq.data_ptr(), n_samples, inp, ch, 0, max_epochs, d_prompt.data_ptr(), None, params=params)
    wall = time.time() - t0
    out = report(secs, n_samples, ch, ne, d_prompt.cpu().numpy(), metas, wall, gen_s, eng.device_name)
    out["input"] = "iq8_multibit" if multibit else "iq8_sign"
    conv_ms, track_ms = eng.track_iq8_last_ms()
    out["convert_ms"], out["track_kernel_ms"] = round(conv_ms, 3), round(track_ms, 3)
    eng.close()
    return out


def report(secs, n_samples, ch, ne, prompt, metas, wall, gen_s, device_name):
    import gpsacq
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
    return {"metric": "track", "secs": secs, "samples": n_samples, "channels": int(ch.size), "lost": int((ch["status"] != 0).sum()),
           "epochs": epochs, "track_wall_s": round(wall, 4), "epochs_per_s": round(epochs / wall, 1), "realtime_x": round(secs / wall, 1),
           "subframes": found, "subframes_wrong": wrong, "parity_failures": pfail, "generate_s": round(gen_s, 3),
           "device": device_name}


def kernel_time(secs, extra=()):
    """The channel kernel's time (k_track, or k_track_iq for multi-bit channels; and the converter's as convert_kernel_ms) from a
    rocprofv3 --kernel-trace --stats run of this script (child process, --no-prof)."""
    d = tempfile.mkdtemp(prefix="track_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--secs", str(secs), "--no-prof", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"prof_error": r.returncode}
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if "k_track" in name:
                out.update({"kernel_ms": round(float(row["TotalDurationNs"]) / 1e6, 3), "kernel_calls": int(row["Calls"])})
            elif "k_iq_to_bits" in name:
                out["convert_kernel_ms"] = round(float(row["TotalDurationNs"]) / 1e6, 3)
    return out if "kernel_ms" in out else {"prof_error": "no k_track row"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--secs", type=float, default=81.8)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--input", choices=("bits", "iq8"), default="bits")
    ap.add_argument("--multibit", action="store_true", help="with --input iq8: multi-bit complex channels instead of the 1-bit ones")
    a = ap.parse_args()
    if a.multibit and a.input != "iq8":
        ap.error("--multibit needs --input iq8")
    out = run(a.secs, a.input, a.multibit)
    if not a.no_prof:
        out.update(kernel_time(a.secs, ["--input", a.input] + (["--multibit"] if a.multibit else [])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
