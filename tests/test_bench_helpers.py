"""bench_extras.py's measurement helpers that need no GPU (bench.py re-exports what its own core uses): the sysfs clock / power
reader behind roofline.sclk_mhz, the sampler's statistics, the host half of the parity verdict, the key digest
(CPU suite; the GPU box runs them for real in tests/test_gpu_round5.py / test_gpu_round6.py)."""
import importlib.util
import os
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_extras_mod", os.path.join(ROOT, "bench_extras.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sysfs_clock_and_power_reader(tmp_path):
    b = _bench()
    card = tmp_path / "card0" / "device"
    (card / "hwmon" / "hwmon3").mkdir(parents=True)
    (card / "pp_dpm_sclk").write_text("0: 132Mhz \n1: 2214Mhz *\n")  # the format of an MI355X box (gpurun_out/r05a/sysfs.txt)
    (card / "hwmon" / "hwmon3" / "power1_average").write_text("1363000000\n")
    assert b.read_clock_power(str(card)) == {"sclk_mhz": 2214, "power_w": 1363.0}
    (card / "hwmon" / "hwmon3" / "power1_average").unlink()
    (card / "hwmon" / "hwmon3" / "power1_input").write_text("901500000\n")
    assert b.read_clock_power(str(card)) == {"sclk_mhz": 2214, "power_w": 901.5}
    (card / "pp_dpm_sclk").write_text("garbage\n")
    assert b.read_clock_power(str(card))["sclk_mhz"] is None
    assert b.read_clock_power(str(tmp_path / "nothing")) == {"sclk_mhz": None, "power_w": None}


def test_clock_sampler_statistics(tmp_path):
    """Medians over the readings taken between start() and stop(); the first one 10 ms in, so a leg of a few steps gets one."""
    b = _bench()
    card = tmp_path / "device"
    (card / "hwmon" / "hwmon0").mkdir(parents=True)
    (card / "pp_dpm_sclk").write_text("0: 132Mhz\n1: 2100Mhz *\n")
    (card / "hwmon" / "hwmon0" / "power1_average").write_text("1000000000\n")
    s = b.ClockSampler.__new__(b.ClockSampler)
    s.card, s.dev_index, s.period = str(card), 0, 0.02
    s.start()
    time.sleep(0.05)
    (card / "pp_dpm_sclk").write_text("0: 132Mhz\n1: 2200Mhz *\n")
    time.sleep(0.12)
    s.stop()
    st = s.stats()
    assert st["samples"] >= 4 and st["sclk_mhz_min_max"] == [2100, 2200] and 2100 <= st["sclk_mhz"] <= 2200 and st["power_w"] == 1000.0
    assert "sysfs" in st["source"]
    s.start()  # a leg shorter than the period still gets its reading
    time.sleep(0.03)
    s.stop()
    assert s.stats()["samples"] >= 1


def test_flops_and_peak_constants():
    b = _bench()
    assert abs(b.flops_per_cell(5456) - (6 * 40000 + 5 * 40000 * 15.287712379549449 + 5 * 5456)) < 1.0
    # 157.3 TFLOP/s = 256 CUs x 128 FMA lanes x 2 flop x 2.4 GHz: the clock frac_at_clock normalises to
    assert abs(256 * 128 * 2 * b.FP32_PEAK_CLOCK_MHZ * 1e6 / 1e12 - b.FP32_VALU_PEAK_TF) < 0.05


def test_compare_peaks_verdict_logic(monkeypatch):
    """The host half of cpu_baseline.parity_vs_gpu on the oracle alone (no GPU): the double-precision oracle's peaks stand in for the
    GPU's.  Equal results pass; a peak moved to another lag is an UNPROVEN mismatch (the bench run then exits 3); the same move is
    accepted as a tie only when the two candidates' double-precision SNRs agree to the tie tolerance (forced here by widening it);
    a result outside the search grid is never a tie."""
    import numpy as np
    from oracle_lib import Oracle
    b = _bench()
    cfg = b.CONFIGS[1]
    bits = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "synth_nott_fs5456.bin"), "rb").read()[:6 * 5120], dtype=np.uint8)
    _, cpu = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f32").bench_blocks(bits, 6)
    _, gpu = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f64").search(bits.tobytes())
    r, _, _ = b.compare_peaks(cfg, gpu, cpu, bits)
    assert r["blocks"] == 6 and r["ca_equal"] == 6 and r["lo_equal"] == 6 and r["n_unproven"] == 0 and r["snr_max_rel"] < 1e-4
    moved = gpu.copy()
    moved["ca_shift"][3] = (moved["ca_shift"][3] + 7) % 5456
    r, _, _ = b.compare_peaks(cfg, moved, cpu, bits)
    assert r["ca_equal"] == 5 and r["unproven_mismatches"] == [3] and r["proven_ties"] == 0
    monkeypatch.setattr(b, "PARITY_TIE_REL", 10.0)  # "anything is a tie": the proven-tie branch itself
    r, _, _ = b.compare_peaks(cfg, moved, cpu, bits)
    assert r["proven_ties"] == 1 and r["n_unproven"] == 0
    off_grid = gpu.copy()
    off_grid["lo_shift"][2] = 500
    r, _, _ = b.compare_peaks(cfg, off_grid, cpu, bits)
    assert r["unproven_mismatches"] == [2]


def test_non_finite_gpu_values_are_never_within_tolerance():
    """A GPU peak whose SNR is NaN but whose code phase and Doppler bin happen to match must fail the verdict (np.nanmax used to skip
    it: ADVICE r5)."""
    import numpy as np
    from oracle_lib import Oracle
    b = _bench()
    cfg = b.CONFIGS[1]
    bits = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "synth_nott_fs5456.bin"), "rb").read()[:4 * 5120], dtype=np.uint8)
    _, cpu = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f32").bench_blocks(bits, 4)
    _, gpu = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f64").search(bits.tobytes())
    bad = gpu.copy()
    bad["snr"][1] = np.nan
    r, _, _ = b.compare_peaks(cfg, bad, cpu, bits)
    assert r["ca_equal"] == 4 and r["non_finite_gpu_peaks"] == 1 and r["unproven_mismatches"] == [1]
    assert not (r["snr_max_rel"] <= b.PARITY_SNR_REL)
    bad["snr"][1] = np.inf
    r, _, _ = b.compare_peaks(cfg, bad, cpu, bits)
    assert r["n_unproven"] == 1 and not (r["snr_max_rel"] <= b.PARITY_SNR_REL)


def test_all_cores_oracle_pass_keeps_the_results_of_the_one_thread_port():
    """cpu_baseline_all_cores (oracle_search_omp): one OpenMP pass over a share of the capture -- block b of the share against PRN
    (first_block + b) % 32, the reference schedule -- returns the SAME peaks and cells as the oracle's plain per-block search (bit for
    bit: the same code, only dealt to threads), the blocks done are a prefix, and a pass whose time is up does nothing."""
    import numpy as np
    from oracle_lib import Oracle
    b = _bench()
    cfg = b.CONFIGS[1]
    bits = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "synth_nott_fs5456.bin"), "rb").read()[:10 * 5120], dtype=np.uint8)
    d, pk, cl, n = b.cpu_baseline_all_cores(cfg, bits, 73, 1000.0, cap_s=120.0, first_block=32 * 3)
    assert n == 10 and d["blocks"] == 10 and d["blocks_of_the_share"] == 10 and d["value"] > 0 and d["cores"] >= 1 and d["speedup_over_1_thread"] > 0
    oc, op = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f32").search(bits.tobytes(), [(i, (96 + i) % 32) for i in range(10)])
    for f in ("snr", "lo_shift", "ca_shift", "max_pwr"):
        assert np.array_equal(pk[f], op[f]), f
    for f in ("max_pwr", "max_i", "tot_pwr", "snr"):
        assert np.array_equal(cl[f], oc[f]), f
    d0, pk0, cl0, n0 = b.cpu_baseline_all_cores(cfg, bits, 73, None, cap_s=0.0)
    assert n0 == 0 and len(pk0) == 0 and cl0.shape == (0, 73) and d0["blocks"] == 0 and d0["speedup_over_1_thread"] is None


def test_compare_cells_verdict_logic():
    """Part (2) of parity_vs_gpu on the oracle alone (no GPU): the double-precision oracle's cells stand in for the GPU's, the float
    build's (the all-cores pass) are the checker's.  Equal results pass; a power 1.5e-5 off the float build goes to the double build
    and passes there; 6e-5 off fails; a lag moved to a weaker sample fails, moved to an exact tie passes as a proven tie; NaN, a
    non-positive power and a lag outside the scan fail outright; too many cells off the screen fail without being judged."""
    import numpy as np
    from oracle_lib import Oracle
    b = _bench()
    cfg = b.CONFIGS[1]
    nb = 3
    bits = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "synth_nott_fs5456.bin"), "rb").read()[:nb * 5120], dtype=np.uint8)
    _, cpu_pk, cpu_cl, _ = b.cpu_baseline_all_cores(cfg, bits, 73, None, cap_s=120.0)
    gcl, gpk = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f64").search(bits.tobytes())
    r = b.parity_vs_gpu(cfg, gpk, gcl, cpu_pk, cpu_cl, bits, first_block=0, share_blocks=nb)
    assert r["ok"] and r["whole_share"] and r["blocks"] == nb and r["cells"] == nb * 73 and r["cells_judged_in_double"] == 0 and r["pwr_max_rel"] < 5e-6, r
    assert b.parity_vs_gpu(cfg, gpk, gcl, cpu_pk, cpu_cl, bits, share_blocks=nb + 32)["whole_share"] is False

    def verdict(mutate):
        g = gcl.copy()
        mutate(g)
        return b.parity_vs_gpu(cfg, gpk, g, cpu_pk, cpu_cl, bits, share_blocks=nb)

    def scale(f, k):
        def m(g):
            g[f][1, 40] *= np.float32(1.0 + k)
        return m
    r = verdict(scale("tot_pwr", 1.5e-5))  # off the screen, inside the judge's tolerance
    assert r["ok"] and r["cells_judged_in_double"] == 1 and 1e-5 < r["pwr_max_rel_judged_in_double"] <= 2e-5, r
    r = verdict(scale("max_pwr", 6e-5))
    assert not r["ok"] and r["n_cell_power_mismatches"] == 1 and r["cell_power_mismatches"][0][:3] == [1, 40 - 36, "max_pwr"], r

    def move_lag(g):
        g["max_i"][2, 5] = (g["max_i"][2, 5] + 11) % 5456
    r = verdict(move_lag)
    assert not r["ok"] and r["cell_lag_mismatches"] == [[2, 5 - 36]] and r["cell_lag_ties"] == 0, r
    for bad in (np.nan, np.inf, 0.0, -1.0):
        def poison(g, bad=bad):
            g["tot_pwr"][0, 0] = bad
        r = verdict(poison)
        assert not r["ok"] and r["non_finite_or_non_positive_cell_powers"] == 1, (bad, r)

    def off_scan(g):
        g["max_i"][0, 72] = 5456
    r = verdict(off_scan)
    assert not r["ok"] and r["cell_lag_mismatches"] == [[0, 36]], r
    # an exact tie in the double-precision powers: the GPU may report either lag
    orc = Oracle(cfg["fc"], cfg["fs"], cfg["max_fo"], kind="f64")
    _, _, lag_powers = b.compare_peaks(cfg, gpk, cpu_pk, bits)
    calls = []

    def tied(block, sv, lo):
        pw = lag_powers(block, sv, lo).copy()
        pw[(int(np.argmax(pw)) + 11) % 5456] = pw.max()
        calls.append((sv, lo))
        return pw
    g = gcl.copy()
    move_lag(g)
    r = b.compare_cells(g, cpu_cl, bits, 0, orc, tied)
    assert r["ok"] and r["cell_lag_ties"] == 1 and calls == [(2, 5 - 36)], r
    # every cell 1e-4 off: nothing is judged one by one, the verdict is a failure
    g = gcl.copy()
    g["max_pwr"] *= np.float32(1.0001)
    r = b.compare_cells(g, cpu_cl, bits, 0, orc, lag_powers, max_recheck=50)
    assert not r["ok"] and r["too_many_cells_off_the_screen"] and r["cells_judged_in_double"] == nb * 73, r


def test_keys_digest_and_host_packing():
    """keys_digest: 16 hex digits of sha256 over the int64 keys; pack_keys_host: the packing of gpsacq_peak_keys_device /
    gpsacq.dist.pack_keys on PEAK records (integer MAX = higher SNR, ties to the lower Doppler bin, c/search_offline.cpp:196-198)."""
    import numpy as np
    import torch
    from gpsacq import dist as D
    b = _bench()
    pk = np.zeros(4, dtype=[("snr", "<f4"), ("lo_shift", "<i4"), ("ca_shift", "<i4"), ("max_pwr", "<f4")])
    pk["snr"], pk["lo_shift"], pk["ca_shift"] = [30.5, 30.5, 12.0, 0.0], [-3, 4, 0, 0], [100, 5455, 7, 0]
    keys = b.pack_keys_host(pk, 36)
    t = torch.from_numpy(np.stack([pk["snr"].view("<i4"), pk["lo_shift"], pk["ca_shift"], pk["max_pwr"].view("<i4")], axis=1).astype(np.int32))
    assert np.array_equal(keys, D.pack_keys(t, 36).numpy())
    assert keys[0] > keys[1] > keys[2] > keys[3]  # equal SNR: the lower Doppler bin wins
    d = b.keys_digest(keys)
    assert len(d) == 16 and d == b.keys_digest(keys.copy()) and d != b.keys_digest(keys[::-1])


def _bench_core():
    spec = importlib.util.spec_from_file_location("bench_core_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_times_the_steps_only_and_full_keeps_the_rest():
    """bench.py without --full: set-up, warm-up, the K timed steps and the line -- no side legs, live traffic, rocFFT baseline,
    in-process multi-GPU leg or front end (the CPU baseline and parity verdict need --full in main()); --full runs them as before;
    --bare is the timed steps alone either way."""
    b = _bench_core()
    p = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert p.steps == 7 and p.warmup == 2 and not p.full and p.dump_outputs is None
    assert (p.weak_blocks, p.soak_seconds, p.pk_fma_seconds) == (0, 0.0, 0.0)
    assert p.no_live_traffic and p.no_library_baseline and p.no_inproc_multi and p.no_e2e and not p.no_cpu_baseline
    f = b.parse_args(["--full", "--dump-outputs", "out"])
    assert f.full and f.dump_outputs == "out" and (f.weak_blocks, f.soak_seconds, f.pk_fma_seconds) == (4096, 6.0, 3.0)
    assert not (f.no_live_traffic or f.no_library_baseline or f.no_inproc_multi or f.no_e2e or f.no_cpu_baseline)
    fb = b.parse_args(["--full", "--bare"])
    assert fb.no_cpu_baseline and fb.no_e2e and fb.no_live_traffic and (fb.weak_blocks, fb.soak_seconds) == (0, 0.0)


def test_dump_outputs_writes_exact_float_arrays_and_samples_large_ones(tmp_path, monkeypatch):
    """bench.dump_outputs on host tensors shaped like a Leg's: the decoded merged keys, the last step's peaks (three buffers: the
    one step_no points at) and cells, as float32 / float64 .npy holding every value exactly; above the cell budget a seeded sample of
    whole tasks, the same rows in every run."""
    import types
    import numpy as np
    import torch
    from gpsacq import CELL_DTYPE, PEAK_DTYPE
    from gpsacq import dist as gdist
    b = _bench_core()
    rng = np.random.default_rng(5)
    n_tasks, ndop, kmax = 96, 73, 36
    pk = np.zeros(n_tasks, dtype=PEAK_DTYPE)
    pk["snr"] = rng.uniform(1, 200, n_tasks).astype(np.float32)
    pk["lo_shift"] = rng.integers(-kmax, kmax + 1, n_tasks)
    pk["ca_shift"] = rng.integers(0, 5456, n_tasks)
    pk["max_pwr"] = rng.uniform(1e3, 1e9, n_tasks).astype(np.float32)
    cells = np.zeros((n_tasks, ndop), dtype=CELL_DTYPE)
    for f in ("max_pwr", "tot_pwr", "snr"):
        cells[f] = rng.uniform(0, 1e9, cells.shape).astype(np.float32)
    cells["max_i"] = rng.integers(0, 5456, cells.shape)
    d_peaks = [torch.zeros((n_tasks, 4), dtype=torch.int32) for _ in range(3)]
    d_peaks[1] = torch.from_numpy(pk.view(np.int32).reshape(n_tasks, 4).copy())
    peaks_t = d_peaks[1]
    best = gdist.per_prn_best(gdist.pack_keys(peaks_t, kmax))
    leg = types.SimpleNamespace(torch=torch, dev=torch.device("cpu"), n_tasks=n_tasks, NBUF=3, step_no=5, d_peaks=d_peaks,
                                d_cells=torch.from_numpy(cells.view(np.int32).reshape(n_tasks, ndop, 4).copy()))
    names = b.dump_outputs(str(tmp_path / "a"), leg, best, kmax, gdist)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["peaks_snr"], pk["snr"]) and np.array_equal(got["peaks_ca_shift"], pk["ca_shift"].astype(np.float64))
    assert np.array_equal(got["peaks_lo_shift"], pk["lo_shift"].astype(np.float64)) and np.array_equal(got["peaks_max_pwr"], pk["max_pwr"])
    assert np.array_equal(got["cells_max_i"], cells["max_i"].astype(np.float64)) and np.array_equal(got["cells_tot_pwr"], cells["tot_pwr"])
    for sv in range(32):  # the merged keys, decoded: the best peak of each PRN (block t <-> PRN t % 32)
        i = sv + 32 * int(np.argmax(pk["snr"][sv::32]))
        assert got["keys_snr"][sv] == pk["snr"][i] and got["keys_ca_shift"][sv] == pk["ca_shift"][i] and got["keys_lo_shift"][sv] == pk["lo_shift"][i]
    assert "cells_index" not in got and got["cells_snr"].shape == (n_tasks, ndop)
    monkeypatch.setattr(b, "DUMP_CELLS_MAX", 10 * ndop)
    for d in ("b", "c"):
        names = b.dump_outputs(str(tmp_path / d), leg, best, kmax, gdist)
    idx = np.load(tmp_path / "b" / "cells_index.npy")
    assert idx.shape == (10,) and np.array_equal(idx, np.load(tmp_path / "c" / "cells_index.npy")) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "cells_max_pwr.npy"), cells["max_pwr"][idx.astype(np.int64)])
