#!/usr/bin/env python3
"""The weight law of the snapshot signal quality, measured on the CPU: where gpsacq_snap_quality_default_params' cn0_ref_lin comes
from, and what the weights are worth (include/gpsacq.h, "Snapshot signal quality", PARAMETERS and LIMITS OF THE MODEL).

Captures are made sample by sample with tests/gen_ref.py (16 blocks at fs = 5.456 MHz, noise sigma 1), every peak is placed at the
whole sample and the Doppler bin nearest to the generator's law, tests/refine_ref.py gives the fine records with the defaults and
tests/snapq_ref.py their C/N0 and weights; the range error of a fine code phase is taken against the generator's law.

  --scene law    (default) six satellites at amplitude 0.2 and one each at 0.1, 0.07, 0.05, 0.04 and 0.03, random Dopplers within
                 +-4.5 kHz and random code phases per capture (tests/snapq_ref.py, law_capture): the table of S = sig / noise, C/N0,
                 range error, the ideal weight var(0.2) / var and the weight the law gives, per amplitude.
  --scene bench  tools/snapshot_bench.py's eight satellites at amplitude 0.2, one window per capture seed: the level the strong
                 satellites read, which is what cn0_ref_lin is set to.

Prints the table and one JSON line with the proposed cn0_ref: the median C/N0 of the amplitude-0.2 satellites, rounded to 0.1 dB.

  --iq8          the same two scenes written as 8-bit IQ captures with tests/gen_ref.py's generator (int8, scale 16, sigma 1, IF
                 0.4 MHz, the mean not removed), tests/refine_iq_ref.py for the multi-bit fine records (GPSACQ_SAMPLES_REAL, mix_hz =
                 fc - IF) and tests/snapq_iq_ref.py for the measured floor: where gpsacq_snap_quality_default_params_iq8's
                 cn0_ref_lin comes from ("Snapshot signal quality on an 8-bit IQ capture", PARAMETERS).

    python tools/snap_quality_law.py [--scene law|bench] [--captures 60] [--procs 8] [--iq8]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, FC, SPM = 5.456e6, 4.092e6, 5456


def work_law(seed):
    import snapq_ref
    return snapq_ref.law_capture(seed)


def work_bench(seed):
    """the bench scene's eight satellites, 16 blocks from sample 0, noise seed `seed`"""
    import numpy as np

    import gen_ref
    import refine_ref
    import snapq_ref
    from coarse_helpers import synth_sats
    from nav_helpers import geometry
    geo = geometry("north")
    sats, _ = synth_sats(geo, geo["subsets"][8], geo["ref_ms"] + 4321, 0.6180e-3, 0, FS, 0.2)
    y = gen_ref.LAW.bits(FC, FS, sats, 1.0, seed, 0, 16 * 40960)["y"]
    bits = np.packbits((y < 0.0).astype(np.uint8), bitorder="little")
    peaks, truth = [], []
    for s in sats:
        chips = (s[3] * gen_ref.LAW.chips_per_sample(s[2], FS)) % 1023.0
        truth.append(chips / 1.023e6)
        peaks.append((100.0, int(round(s[2] / (FS / 40000))), int(round(chips / 1.023e6 * FS)) % SPM, 1.0))
    recs = refine_ref.refine(bits, 5120, [(0, s[0] - 1) for s in sats], peaks, SPM, FC, FS)
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    err = np.array([snapq_ref.C_MPS * wrap(r["tx_frac"] - t) for r, t in zip(recs, truth)])
    return np.full(len(sats), 0.2), recs, err


IF_HZ, SCALE = 0.4e6, 16.0  # tools/snapshot_bench.py --iq8


def iq8_records(sats, noise_seed, blocks=16):
    """the scene of `sats` as an 8-bit IQ capture of `blocks` blocks from sample 0: (fine records, floors, info, range errors)"""
    import numpy as np

    import gen_ref
    import refine_iq_ref
    import snapq_iq_ref
    import snapq_ref
    iq = gen_ref.LAW.quantise(gen_ref.LAW.iq8(FS, sats, IF_HZ, SCALE, 1.0, noise_seed, 0, blocks * 40960)["v"], True).ravel()
    peaks, truth = [], []
    for s in sats:
        chips = (s[3] * gen_ref.LAW.chips_per_sample(s[2], FS)) % 1023.0
        truth.append(chips / 1.023e6)
        peaks.append((100.0, int(round(s[2] / (FS / 40000))), int(round(chips / 1.023e6 * FS)) % SPM, 1.0))
    tasks = [(0, s[0] - 1) for s in sats]
    recs = refine_iq_ref.refine(iq, 81920, tasks, peaks, SPM, FC, FS, signed=True, mix_hz=FC - IF_HZ, blocks=blocks)
    _, info = snapq_iq_ref.quality(iq, 81920, tasks, recs, SPM, FS, signed=True)
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    err = np.array([snapq_ref.C_MPS * wrap(r["tx_frac"] - t) for r, t in zip(recs, truth)])
    return info, err


def work_law_iq8(seed):
    """snapq_ref.law_capture's scene (the same draws of Doppler, code phase and carrier phase) as an 8-bit IQ capture"""
    import numpy as np

    import snapq_ref as sq
    rng = np.random.default_rng(seed)
    n = len(sq.LAW_AMPLITUDES)
    dop, phase, carrier = rng.uniform(-4500.0, 4500.0, n), rng.uniform(0.0, sq.LAW_SPM, n), rng.uniform(0.0, 1.0, n)
    sats = [(sq.LAW_PRNS[k], sq.LAW_AMPLITUDES[k], float(dop[k]), float(phase[k]), float(carrier[k])) for k in range(n)]
    info, err = iq8_records(sats, 1000 + seed, sq.LAW_BLOCKS)
    return np.array(sq.LAW_AMPLITUDES), info, err


def work_bench_iq8(seed):
    """work_bench's eight satellites as an 8-bit IQ capture"""
    import numpy as np

    from coarse_helpers import synth_sats
    from nav_helpers import geometry
    geo = geometry("north")
    sats, _ = synth_sats(geo, geo["subsets"][8], geo["ref_ms"] + 4321, 0.6180e-3, 0, FS, 0.2)
    info, err = iq8_records(sats, seed)
    return np.full(len(sats), 0.2), info, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iq8", action="store_true", help="the scenes as 8-bit IQ captures, multi-bit records and the measured floor")
    ap.add_argument("--scene", choices=("law", "bench"), default="law")
    ap.add_argument("--captures", type=int, default=60)
    ap.add_argument("--procs", type=int, default=8)
    a = ap.parse_args()
    import numpy as np

    import snapq_ref
    with multiprocessing.Pool(a.procs) as pool:
        out = pool.map((work_law_iq8 if a.iq8 else work_law) if a.scene == "law" else (work_bench_iq8 if a.iq8 else work_bench), range(a.captures))
    amps, err = np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out])
    defaults = snapq_ref.DEFAULTS
    if a.iq8:
        import snapq_iq_ref
        info, defaults = np.concatenate([o[1] for o in out]), snapq_iq_ref.DEFAULTS
    else:
        info = snapq_ref.quality([r for o in out for r in o[1]], SPM, FS)
    rows = snapq_ref.law_table(amps, info, err)
    snapq_ref.law_print(rows)
    strong = info["cn0_dbhz"][amps == snapq_ref.LAW_STRONG]
    weak = amps < snapq_ref.LAW_STRONG
    pooled = float((info["weight"][weak] * err[weak] ** 2).mean() / (err[~weak] ** 2).mean()) if weak.any() else None
    print(json.dumps({**({"iq8": True} if a.iq8 else {}), "scene": a.scene, "captures": a.captures, "strong_records": int(strong.size), "cn0_strong_median_dbhz": round(float(np.median(strong)), 3),
                      "cn0_strong_min_dbhz": round(float(strong.min()), 3), "cn0_strong_max_dbhz": round(float(strong.max()), 3),
                      "range_rms_strong_m": round(float(np.sqrt((err[~weak] ** 2).mean())), 3), "weighted_over_strong_pooled": None if pooled is None else round(pooled, 4),
                      "cn0_ref_dbhz_proposed": round(float(np.median(strong)), 1),
                      "cn0_ref_dbhz_default": round(10 * float(np.log10(defaults["cn0_ref_lin"])), 1)}))


if __name__ == "__main__":
    main()
