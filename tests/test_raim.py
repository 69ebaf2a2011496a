"""Fix integrity on the CPU: the records and the chi-square thresholds of the library (host only), and the properties of
tests/raim_ref.py that the GPU tests (tests/test_gpu_raim.py) rely on when they compare the kernels with it."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import atm_ref
import raim_cases
import raim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes(tmp_path):
    import gpsacq
    sizes = (gpsacq.RAIM_PARAMS_DTYPE.itemsize, gpsacq.FIX_RAIM_DTYPE.itemsize)
    src = tmp_path / "sizes.c"
    src.write_text('#include "gpsacq.h"\n'
                   '_Static_assert(sizeof(gpsacq_raim_params) == %d, "params");\n'
                   '_Static_assert(sizeof(gpsacq_fix_raim) == %d, "raim");\n'
                   '_Static_assert(GPSACQ_RAIM_MAX_DOF == GPSACQ_FIX_MAX_SATS - 4, "dof");\n' % sizes)
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert sizes == (88, 40)
    for dt in (gpsacq.RAIM_PARAMS_DTYPE, gpsacq.FIX_RAIM_DTYPE):
        assert dt.itemsize == sum(dt[n].itemsize for n in dt.names)
    assert (gpsacq.RAIM_NONE, gpsacq.RAIM_UNCHECKED, gpsacq.RAIM_PASS, gpsacq.RAIM_EXCLUDED, gpsacq.RAIM_FAILED) == (0, 1, 2, 3, 4) == \
        (raim_ref.NONE, raim_ref.UNCHECKED, raim_ref.PASS, raim_ref.EXCLUDED, raim_ref.FAILED)
    assert gpsacq.RAIM_MAX_DOF == 8 == raim_ref.MAX_DOF
    for name in ("gpsacq_raim_default_params", "gpsacq_fix_raim_batch", "gpsacq_fix_raim_batch_device", "gpsacq_fix_raim_last_ms"):
        assert name in gpsacq.EXPORTS and getattr(gpsacq.load_library(), name)


def test_default_thresholds_are_the_table():
    import gpsacq
    rp = gpsacq.raim_params(3.0)
    assert rp.shape == (1,) and rp["sigma_m"][0] == 3.0 and rp["p_fa"][0] == 1e-3 and rp["exclude"][0] == 1 and rp["reserved"][0] == 0
    got = rp["threshold"][0]
    worst = np.abs(got / np.array(raim_ref.TABLE_1E3) - 1).max()
    print("p_fa 1e-3: %.3g relative from the table" % worst)
    assert worst <= 1e-12
    # the reference's own closed form and bisection agree with the table and with the library at other tails
    assert np.abs(np.array(raim_ref.params(3.0)["threshold"]) / np.array(raim_ref.TABLE_1E3) - 1).max() <= 1e-12
    for p_fa in (0.5, 0.05, 1e-5, 1e-9, 1e-15):
        lib_t = gpsacq.raim_params(1.0, p_fa)["threshold"][0]
        ref_t = np.array([raim_ref.chi2_threshold(d, p_fa) for d in range(1, 9)])
        assert np.abs(lib_t / ref_t - 1).max() <= 1e-12, p_fa
        for d in range(1, 9):  # the threshold is the quantile: the tail at it is p_fa
            assert abs(raim_ref.chi2_tail(d, lib_t[d - 1]) / p_fa - 1) <= 1e-9, (p_fa, d)


def test_thresholds_are_monotone():
    import gpsacq
    tails = (0.5, 0.1, 1e-2, 1e-3, 1e-6, 1e-10, 1e-15)
    table = np.array([gpsacq.raim_params(2.0, p)["threshold"][0] for p in tails])
    assert (np.diff(table, axis=1) > 0).all()  # in d
    assert (np.diff(table, axis=0) > 0).all()  # a smaller tail is a larger quantile
    assert table.min() > 0 and np.isfinite(table).all() and table.max() < 4000


def test_default_params_argument_errors():
    import gpsacq
    lib = gpsacq.load_library()
    out = np.full(1, 0, gpsacq.RAIM_PARAMS_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    poison = out.tobytes()
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    for sigma, p_fa in ((0.0, 1e-3), (-1.0, 1e-3), (float("nan"), 1e-3), (float("inf"), 1e-3), (3.0, 0.0), (3.0, 0.9e-15), (3.0, 0.5000001),
                        (3.0, 1.0), (3.0, -1e-3), (3.0, float("nan")), (3.0, float("inf"))):
        assert lib.gpsacq_raim_default_params(sigma, p_fa, ptr) == 1, (sigma, p_fa)
        assert out.tobytes() == poison
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            gpsacq.raim_params(sigma, p_fa)
        assert ei.value.code == 1
    assert lib.gpsacq_raim_default_params(3.0, 1e-3, None) == 1
    assert lib.gpsacq_raim_default_params(3.0, 1e-15, ptr) == 0 and lib.gpsacq_raim_default_params(3.0, 0.5, ptr) == 0  # both ends are in range


# ---- the reference on the "north" geometry: twelve satellites, ten of them above the 5-degree mask -----------------------------
def test_reference_passes_exact_observations():
    geo, ref_ms, t_rx, obs = raim_cases.truth(3)
    p, rp = atm_ref.params(), raim_ref.params(3.0)
    for k in (0, 64, 129):
        ref = raim_cases.reference(geo, obs[k], p, rp)
        raim = ref["raim"]
        print("row %d: stat_full %.3g, dof %d" % (k, raim["stat_full"], raim["dof"]))
        assert ref["status"] == 0 and ref["n_masked"] == 2 and raim["status"] == raim_ref.PASS and raim["dof"] == 6
        assert raim["stat_full"] < 1e-6 and raim["stat"] == raim["stat_full"] and raim["excluded"] == -1 and raim["n_candidates"] == 0
        assert raim["threshold"] == rp["threshold"][5]
        assert np.abs(ref["xyz"] - geo["rx"]).max() < 1e-4


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_excludes_the_faulted_satellite(seed):
    geo, ref_ms, t_rx, obs = raim_cases.truth(3)
    p, rp = atm_ref.params(), raim_ref.params(3.0)
    kept = [s for s in range(12) if s not in (9, 10)]  # what the mask leaves
    ob = raim_cases.noisy(obs[:10], seed, 3.0)
    worst_err = worst_state = 0.0
    for k in range(10):
        col = kept[k]  # each of the ten rows pulls another satellite
        ob[k:k + 1, col:col + 1] = raim_cases.shift(ob[k:k + 1, col:col + 1].copy(), 150.0)
        ref = raim_cases.reference(geo, ob[k], p, rp)
        raim = ref["raim"]
        assert raim["status"] == raim_ref.EXCLUDED and ref["excluded"] == col, (k, raim)
        assert raim["dof"] == 5 and raim["n_candidates"] == 10 and raim["stat_full"] > rp["threshold"][5] and raim["stat"] <= rp["threshold"][4]
        assert ref["n_used"] == 9 and ref["used_mask"] == 0xFFF & ~(1 << 9 | 1 << 10 | 1 << col)
        worst_err = max(worst_err, float(np.linalg.norm(ref["xyz"] - geo["rx"])))
        # FINAL ends where CORRECTED FIX ends on the row without that observation
        without = ob[k].copy()
        without["valid"][col] = 0
        u = raim_cases.usable(geo, without)
        alone = atm_ref.fix_atm(geo["ephs"], without["eph"][u], without["tx_ms"][u], without["tx_frac"][u], without["weight"][u], p)
        assert alone["status"] == 0 and alone["n_used"] == 9
        worst_state = max(worst_state, float(np.abs(ref["xyz"] - alone["xyz"]).max()), abs(ref["t_rx"] - alone["t_rx"]) * atm_ref.C)
        assert np.abs(np.array(ref["dop"]) / np.array(alone["dop"]) - 1).max() < 1e-9
    print("seed %d: final position at most %.3g m from truth, %.3g m from the fix without the observation" % (seed, worst_err, worst_state))
    assert worst_err <= 30.0 and worst_state <= 1e-6


def test_every_batch_of_the_gpu_tests_meets_its_precondition():
    """what tests/test_gpu_raim.py asserts before it looks at a GPU result, here where no GPU is needed to find a bad seed"""
    seen = set()
    for name in raim_cases.BATCHES:
        geo, ob, p, rp = raim_cases.batch(name)
        for k, ref in enumerate(raim_cases.references(name)):
            assert raim_cases.precondition(ref, p, rp) is None, (name, k, raim_cases.precondition(ref, p, rp))
            seen.add(ref["raim"]["status"])
    assert seen == {0, 1, 2, 3, 4}
    r67 = raim_cases.references("sixtyseven")
    assert r67[9]["raim"]["status"] == raim_ref.PASS and r67[9]["raim"]["dof"] == 5       # the fault on a weight-0 observation
    assert r67[13]["raim"]["status"] == raim_ref.NONE and r67[13]["status"] == 1            # three usable
    assert (r67[64]["excluded"], r67[66]["excluded"], r67[5]["excluded"]) == (0, 11, 2)    # the edge lanes; next to a hole
    assert all(r["raim"]["status"] == raim_ref.EXCLUDED for r in raim_cases.references("all_faulted"))
    assert all(r["raim"]["status"] == raim_ref.PASS for r in raim_cases.references("none_faulted"))
    assert [r["raim"]["status"] for r in raim_cases.references("five")] == [2, 4, 4, 2, 4, 2]
    assert all(r["raim"]["status"] == raim_ref.UNCHECKED for r in raim_cases.references("four"))
    assert [r["raim"]["status"] for r in raim_cases.references("no_exclusion")] == [2, 4, 4]
    assert {r["full"]["n_masked"] for r in raim_cases.references("plain")} == {0} and any(r["excluded"] >= 0 for r in raim_cases.references("plain"))
