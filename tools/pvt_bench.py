#!/usr/bin/env python3
"""Capture-to-position benchmark: a synthetic 1-bit capture of five satellites with real navigation data (the constellation of
the tests, tests/nav_ref.py; device generator), searched, tracked, decoded on the host (NAV bits, subframes, ephemerides, time
tags), and then gpsacq_fix_track_device at every millisecond of the capture at which every channel has records -- records,
observations and fixes resident in device memory.  Prints one JSON line: the device time of the two observables kernels and of
the solver's two (HIP events on the engine's stream, best of --reps calls), fixes per second over the four, and the position
error against the generator's truth.

The generator runs every satellite at the Doppler it has at sample 19.5 s x fs, where its transmit times are the truth maker's;
away from that instant the truth is off by the range acceleration (metres over the capture), so the error is given at that
instant, and as median and maximum over the instants after the loops' first two seconds.

With --velocity the line also carries the velocity leg: gpsacq_pvt_track_device over the same instants (Doppler averaged over half
a second of samples), the device time of its four kernels from the same call as the others, and the speed of the stationary
receiver at 19.5 s and over the instants whose window lies inside the records.  Without the flag the line is unchanged.

With --smooth [--window M] the line also carries the smoothed leg: gpsacq_fix_smooth_track_device over the same instants (window M
instants, default 1000; the other parameters at their defaults), the device time of k_code_pos, k_carrier_acc and the four smoothing
kernels from one call, code_sigma_m per channel, and position scatter (about the mean) and error (of the mean), raw beside smoothed,
over the instants at which every channel's window is full.  Without the flag the line is unchanged.

With --quality the line also carries the signal-quality leg: gpsacq_fix_quality_track_device over the same instants (raw
observations, the default quality parameters), the device time of k_quality_acc and k_quality_out beside k_code_pos and k_observe
of the same call, the mean C/N0 per channel over the full windows and how many observations the gate took out.  Without the flag
the line is unchanged.

    python tools/pvt_bench.py [--seconds 20] [--reps 5] [--velocity] [--smooth [--window 1000]] [--quality]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, FC, SPM, L1 = 5.456e6, 4.092e6, 5456, 1575.42e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--velocity", action="store_true")
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    if a.seconds < 20.0:
        ap.error("subframes 1-3 are complete 19 s into the capture: --seconds must be at least 20")

    import numpy as np
    import torch

    import gpsacq
    import nav_ref
    from nav_helpers import geometry

    geo = geometry("north")
    ephs = [geo["ephs"][k] for k in geo["subsets"][5]]
    n_bytes = int(a.seconds * FS) // 8
    r_star = int(19.5 * FS)
    tow0 = 64898
    bit0_ms = (tow0 - 1) * 6000
    ref_ms, ref_frac = bit0_ms + 18_275, 0.3217e-3  # the receive time at r_star: bit 0 lies 1.3 s into the capture, past the 1000 epochs bit sync skips on a channel started from block 8
    sats, nav = [], []
    for j, eph in enumerate(ephs):
        t = nav_ref.truth_tx(eph, geo["rx"], ref_ms, np.array([ref_frac - 0.5, ref_frac, ref_frac + 0.5]))
        dop = L1 * ((t[2] - t[0]) - 1.0)
        cp = ((ref_ms - bit0_ms) + t[1] * 1e3) * FS / (1000.0 * (1.0 + dop / L1)) - r_star
        sats.append((int(eph["prn"]), 0.15 + 0.0125 * j, float(dop), float(cp), 0.1 + 0.17 * j))
        nav.append(1 - 2 * nav_ref.encode_stream(eph, tow0, ids=(1, 2, 3, 4, 5)).astype(np.int8))
    prns = [s[0] for s in sats]

    with gpsacq.Engine(FC, FS, 5000.0, device=0) as eng:
        d_bits = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda:0")
        d_peaks = torch.zeros(32 * gpsacq.PEAK_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.generate_device(d_bits.data_ptr(), n_bytes, sats, noise_sigma=1.0, seed=77, nav=np.array(nav))
        eng.search_device(d_bits.data_ptr(), 32, d_peaks.data_ptr())
        peaks = d_peaks.cpu().numpy().view(gpsacq.PEAK_DTYPE)
        chans = np.concatenate([eng.track_start(p, peaks[p - 1], (p - 1) * gpsacq.BLOCK_BYTES * 8) for p in prns])
        max_epochs = int(a.seconds * 1000) + 100
        d_prompt = torch.zeros(len(prns) * max_epochs * 2, dtype=torch.int32, device="cuda:0")
        d_rec = torch.zeros(len(prns) * max_epochs * gpsacq.TRACK_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ne = eng.track_device(d_bits.data_ptr(), n_bytes, chans, 0, max_epochs, d_prompt.data_ptr(), d_rec.data_ptr())
        prompt = d_prompt.cpu().numpy().reshape(len(prns), max_epochs, 2)
        tags, recs = [], []
        for c, prn in enumerate(prns):
            n = int(ne[c])
            bits, e0 = gpsacq.nav_bits(prompt[c, 1000:n, 0], first_epoch=int(chans["epoch"][c]) - n + 1000)
            sf, _ = gpsacq.nav_subframes(bits)
            if not len(sf):
                raise SystemExit("PRN %d: no subframe decoded" % prn)
            recs.append(gpsacq.ephemeris(sf, prn))
            tags.append(gpsacq.time_tag(sf[0], e0, c))
        tags, recs = np.concatenate(tags), np.concatenate(recs)
        # every millisecond (on r_star's grid) at which every channel has records
        records0 = d_rec.cpu().numpy().view(gpsacq.TRACK_RECORD_DTYPE).reshape(len(prns), max_epochs)[:, 0]
        lo, hi = int(records0["sample"].max()), int(chans["next_sample"].min())
        first = r_star - (r_star - lo) // SPM * SPM
        n_fix = (hi - 1 - first) // SPM + 1
        d_fix = torch.zeros(n_fix * gpsacq.FIX_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        best = None
        for _ in range(1 + a.reps):  # the first call also allocates the engine's scratch
            eng.fix_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_fix.data_ptr(), sync=True)
            ms = eng.observables_last_ms() + eng.fix_last_ms()
            if best is None or sum(ms) < sum(best):
                best = ms
        fix = d_fix.cpu().numpy().view(gpsacq.FIX_DTYPE)
        vbest = None
        if a.velocity:
            d_fix2 = torch.zeros_like(d_fix)
            d_vel = torch.zeros(n_fix * gpsacq.VEL_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(1 + a.reps):
                eng.pvt_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, int(0.5 * FS), d_fix2.data_ptr(),
                                     d_vel.data_ptr(), sync=True)
                ms = eng.observables_last_ms() + eng.fix_last_ms() + eng.velocity_last_ms()
                if vbest is None or sum(ms) < sum(vbest):
                    vbest = ms
            vel = d_vel.cpu().numpy().view(gpsacq.VEL_DTYPE)
            assert d_fix2.cpu().numpy().tobytes() == fix.tobytes()
        sbest = None
        if a.smooth:
            d_fix3 = torch.zeros_like(d_fix)
            d_info = torch.zeros(n_fix * len(prns) * gpsacq.SMOOTH_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(1 + a.reps):
                eng.fix_smooth_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_fix3.data_ptr(),
                                            d_info_ptr=d_info.data_ptr(), params=gpsacq.smooth_params(window=a.window), sync=True)
                ms = eng.observables_last_ms()[:1] + eng.velocity_last_ms()[:1] + eng.smooth_last_ms() + eng.fix_last_ms()
                if sbest is None or sum(ms) < sum(sbest):
                    sbest = ms
            sfix = d_fix3.cpu().numpy().view(gpsacq.FIX_DTYPE)
            sinfo = d_info.cpu().numpy().view(gpsacq.SMOOTH_INFO_DTYPE).reshape(n_fix, len(prns))
        qbest = None
        if a.quality:
            d_fix4 = torch.zeros_like(d_fix)
            d_qinfo = torch.zeros(n_fix * len(prns) * gpsacq.QUALITY_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(1 + a.reps):
                eng.fix_quality_track_device(recs, d_rec.data_ptr(), max_epochs, ne, chans, tags, first, SPM, n_fix, d_fix4.data_ptr(),
                                             d_info_ptr=d_qinfo.data_ptr(), sync=True)
                ms = eng.observables_last_ms() + eng.quality_last_ms() + eng.fix_last_ms()
                if qbest is None or sum(ms) < sum(qbest):
                    qbest = ms
            qfix = d_fix4.cpu().numpy().view(gpsacq.FIX_DTYPE)
            qinfo = d_qinfo.cpu().numpy().view(gpsacq.QUALITY_INFO_DTYPE).reshape(n_fix, len(prns))
        name = eng.device_name
    off = np.linalg.norm(np.stack([fix["x"], fix["y"], fix["z"]], 1) - geo["rx"], axis=1)
    ok = fix["status"] == 0
    row = (r_star - first) // SPM
    late = ok & (np.arange(n_fix) * SPM + first >= 2 * FS)
    out = {"bench": "pvt", "device": name, "seconds": a.seconds, "sats": len(prns), "epochs": int(ne.min()), "n_fix": int(n_fix),
                      "code_pos_ms": round(best[0], 4), "observe_ms": round(best[1], 4), "sat_state_ms": round(best[2], 4),
                      "fix_ms": round(best[3], 4), "kernel_ms": round(sum(best), 4), "fixes_per_s": round(n_fix / (sum(best) * 1e-3)),
                      "ok": int(ok.sum()), "valid_ephemerides": int(sum(gpsacq.ephemeris_valid(r) for r in recs)),
                      "position_error_at_19p5s_m": round(float(off[row]), 2), "position_error_median_m": round(float(np.median(off[late])), 2),
                      "position_error_max_m": round(float(off[late].max()), 2)}
    if a.velocity:
        vok = vel["status"] == 0
        speed = np.sqrt(vel["vx"] ** 2 + vel["vy"] ** 2 + vel["vz"] ** 2)
        vlate = vok & late
        names = ("code_pos_ms", "observe_ms", "sat_state_ms", "fix_ms", "carrier_acc_ms", "observe_rate_ms", "sat_state_rate_ms", "vel_ms")
        out["velocity"] = dict({k: round(v, 4) for k, v in zip(names, vbest)}, kernel_ms=round(sum(vbest), 4),
                               pvt_per_s=round(n_fix / (sum(vbest) * 1e-3)), ok=int(vok.sum()), avg_samples=int(0.5 * FS),
                               speed_at_19p5s_mps=round(float(speed[row]), 4), speed_median_mps=round(float(np.median(speed[vlate])), 4),
                               speed_max_mps=round(float(speed[vlate].max()), 4), drift_at_19p5s=float(vel["drift"][row]))
    if a.smooth:
        full = ((sinfo["flags"] & gpsacq.SMOOTH_FULL) != 0).all(axis=1) & ok & (sfix["status"] == 0)

        def scatter_and_error(f):
            xyz = np.stack([f["x"][full], f["y"][full], f["z"][full]], 1)
            return (round(float(np.sqrt(((xyz - xyz.mean(axis=0)) ** 2).sum(axis=1).mean())), 3),
                    round(float(np.linalg.norm(xyz.mean(axis=0) - geo["rx"])), 3))

        names = ("code_pos_ms", "carrier_acc_ms", "lock_acc_ms", "cmc_ms", "smooth_scan_ms", "smooth_out_ms", "sat_state_ms", "fix_ms")
        (s_raw, e_raw), (s_sm, e_sm) = (scatter_and_error(fix), scatter_and_error(sfix)) if full.any() else ((None, None), (None, None))
        out["smooth"] = dict({k: round(v, 4) for k, v in zip(names, sbest)}, kernel_ms=round(sum(sbest), 4), window=a.window,
                             full_instants=int(full.sum()), unlocked=int(((sinfo["flags"] & gpsacq.SMOOTH_UNLOCKED) != 0).sum()),
                             resets=int(((sinfo["flags"] & gpsacq.SMOOTH_RESET) != 0).sum()),
                             code_sigma_m=[round(float(v), 3) for v in gpsacq.code_sigma_m(sinfo)],
                             position_scatter_raw_m=s_raw, position_scatter_smoothed_m=s_sm,
                             position_error_raw_m=e_raw, position_error_smoothed_m=e_sm)
    if a.quality:
        names = ("code_pos_ms", "observe_ms", "quality_acc_ms", "quality_out_ms", "sat_state_ms", "fix_ms")
        qfull = (qinfo["flags"] & gpsacq.QUALITY_FULL) != 0
        qoff = np.linalg.norm(np.stack([qfix["x"], qfix["y"], qfix["z"]], 1) - geo["rx"], axis=1)
        qlate = (qfix["status"] == 0) & late
        out["quality"] = dict({k: round(v, 4) for k, v in zip(names, qbest)}, kernel_ms=round(sum(qbest), 4), ok=int((qfix["status"] == 0).sum()),
                              cn0_dbhz=[round(float(qinfo["cn0_dbhz"][qfull[:, c], c].mean()), 2) if qfull[:, c].any() else None
                                        for c in range(len(prns))],
                              gated=int(((qinfo["weight"] == 0) & (qinfo["epochs"] > 0)).sum()),
                              unlocked=int(((qinfo["flags"] & gpsacq.QUALITY_UNLOCKED) != 0).sum()),
                              position_error_median_m=round(float(np.median(qoff[qlate])), 2) if qlate.any() else None)
        out["quality_acc_ms"], out["quality_out_ms"] = round(qbest[2], 4), round(qbest[3], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
