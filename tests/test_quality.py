"""The signal-quality model of include/gpsacq.h ("Signal quality per observation") on the CPU: tests/quality_ref.py against
itself two ways, against closed forms and against the estimator's noise-only floor; gpsacq_quality_default_params through ctypes.
The parameter checks of the entry points need an engine and are marked gpu."""
import ctypes
import math

import numpy as np
import pytest

import quality_ref as qr

# std over the 50 seeds of test_noise_only_floor of the reference's reading, dB, as measured by that test (it prints it); the mean over
# the seeds read 26.677 dB-Hz against the 26.693 of the closed form
FLOOR_SPREAD_DB = 0.232


def test_prefix_sums_equal_the_window_loop():
    rng = np.random.default_rng(5)
    for epochs, min_epochs, span in ((1, 1, 1 << 12), (20, 5, 1 << 16), (200, 20, (1 << 21) - 1), (1024, 1024, (1 << 21) - 1), (1024, 3, (1 << 26) - 1)):
        p = qr.par(epochs=epochs, min_epochs=min_epochs, lock_num=3, lock_den=4)
        n = epochs + 37
        ip, qp = rng.integers(-span, span + 1, n), rng.integers(-span // 3, span // 3 + 1, n)
        a, b = qr.channel_series(ip, qp, p), qr.channel_series(ip, qp, p, direct=True)
        assert a == b
        assert [r["epochs"] for r in a] == [min(t + 1, epochs) for t in range(n)]
        assert all(((r["flags"] & qr.FULL) != 0) == (r["epochs"] == epochs) and ((r["flags"] & qr.SHORT) != 0) == (r["epochs"] < min_epochs) for r in a)
    # the last case lies past the no-wrap bound: A^2 did wrap there, and the two forms still agree
    assert any(sum(abs(int(v)) for v in ip[t - 1023:t + 1]) ** 2 > qr.M64 for t in range(1023, n))


def test_closed_forms():
    p = qr.par(epochs=50, min_epochs=10)
    n = 80
    # constant ip, no qp: A^2 = m^2 a^2 = m D
    r = qr.channel_series([700] * n, [0] * n, p)
    for t, x in enumerate(r):
        m = min(t + 1, 50)
        assert x["sig"] == (700 * m) ** 2 and x["noise"] == 0 and (x["flags"] & qr.SATURATED) and not (x["flags"] & (qr.UNLOCKED | qr.NO_POWER))
        assert x["lin"] == np.inf and x["cn0_dbhz"] == 99.0 and x["weight"] == (1.0 if m >= 10 else 0.0)
    # the navigation bit changes nothing
    assert qr.channel_series([700 * (-1) ** (t // 7) for t in range(n)], [0] * n, p) == r
    # nothing at all
    for x in qr.channel_series([0] * n, [0] * n, p):
        assert x["flags"] & qr.NO_POWER and x["flags"] & qr.UNLOCKED and x["sig"] == x["noise"] == 0 and x["lin"] == x["cn0_dbhz"] == x["weight"] == 0
    # all of the power in QP: NO_POWER through sig == 0, with D != 0
    for t, x in enumerate(qr.channel_series([0] * n, [300] * n, p)):
        m = min(t + 1, 50)
        assert x["flags"] & qr.NO_POWER and x["flags"] & qr.UNLOCKED and x["sig"] == 0 and x["noise"] == m * m * 90000 and x["weight"] == 0
    # ip = +-a, qp = +-b: A = m a, D = m (a^2 + b^2), noise = m^2 b^2, snr = a^2 / b^2 exactly
    for a, b in ((1000, 10), (1000, 100), (640, 320), (5, 2)):
        ip, qp = [a * (-1) ** t for t in range(n)], [b * (-1) ** (t // 2) for t in range(n)]
        for t, x in enumerate(qr.channel_series(ip, qp, p)):
            m = min(t + 1, 50)
            lin = np.float64(a * a * m * m) / np.float64(b * b * m * m) * np.float64(1000.0)
            assert x["sig"] == (m * a) ** 2 and x["noise"] == (m * b) ** 2 and x["lin"] == lin and x["flags"] & ~(qr.FULL | qr.SHORT) == 0
            assert x["cn0_dbhz"] == 10.0 * math.log10(lin)
            want = 0.0 if m < 10 or lin < 1000.0 else min(1.0, lin / 10.0 ** 4.5)
            assert x["weight"] == want
    x = qr.channel_series([1000, -1000] * 30, [10, -10] * 30, p)[-1]
    assert x["cn0_dbhz"] == pytest.approx(70.0, abs=1e-12) and x["weight"] == 1.0
    x = qr.channel_series([5, -5] * 30, [2, 2] * 30, p)[-1]      # 38 dB-Hz: between the gate and the reference level
    assert x["weight"] == np.float64(6250.0) / np.float64(10.0 ** 4.5) and 0 < x["weight"] < 1
    # the lock ratio: N / D = (a^2 - b^2) / (a^2 + b^2); (2, 1) gives 3 / 5, exactly on a threshold of 3 / 5
    for num, den, locked in ((3, 5, True), (2, 3, False), (1, 2, True)):
        x = qr.channel_series([2, -2] * 30, [1, 1] * 30, qr.par(epochs=50, lock_num=num, lock_den=den))[-1]
        assert ((x["flags"] & qr.UNLOCKED) == 0) == locked
    # require_lock = 0 lets an unlocked channel keep its weight
    ip, qp = [30, -30] * 30, [40, 40] * 30
    assert qr.channel_series(ip, qp, qr.par(epochs=50, cn0_min_lin=0.0))[-1]["weight"] == 0
    x = qr.channel_series(ip, qp, qr.par(epochs=50, cn0_min_lin=0.0, require_lock=0))[-1]
    assert x["flags"] & qr.UNLOCKED and x["weight"] == np.float64(562.5) / np.float64(10.0 ** 4.5)


def test_noise_only_floor():
    """1024 epochs of Gaussian ip, qp and nothing else: the estimator reads (2/pi) / (2 - 2/pi), 26.69 dB-Hz, to within three times
    its spread over 50 seeds (measured here: mean 26.677, std 0.232 dB)"""
    assert qr.FLOOR_DBHZ == pytest.approx(26.6926, abs=1e-4)
    p = qr.par(epochs=1024)
    got = []
    for seed in range(50):
        rng = np.random.default_rng(seed)
        ip, qp = np.rint(rng.standard_normal(1024) * 1000).astype(np.int64), np.rint(rng.standard_normal(1024) * 1000).astype(np.int64)
        x = qr.channel_series(ip, qp, p)[-1]
        assert x["epochs"] == 1024 and x["weight"] == 0 and x["lin"] < 1000.0   # below the default gate
        got.append(float(x["cn0_dbhz"]))
    got = np.array(got)
    print("noise-only floor over 50 seeds: mean %.3f std %.3f dB-Hz, largest distance from %.3f: %.3f" %
          (got.mean(), got.std(ddof=1), qr.FLOOR_DBHZ, np.abs(got - qr.FLOOR_DBHZ).max()))
    assert np.abs(got - qr.FLOOR_DBHZ).max() < 3 * FLOOR_SPREAD_DB


def test_reference_instants_and_weights():
    """quality_ref.quality on a small case: INVALID instants are zero records, several instants of one epoch share its record, and
    apply_weights touches the weight of valid observations only"""
    import gpsacq
    rec = np.zeros((2, 12), gpsacq.TRACK_RECORD_DTYPE)
    rec["sample"] = 100 + 10 * np.arange(12)
    rec["ip"], rec["qp"] = [[50, -50] * 6, [5, -5] * 6], [[1] * 12, [4] * 12]
    chans = np.zeros(2, gpsacq.TRACK_CHAN_DTYPE)
    chans["next_sample"] = [220, 190]
    tags = np.zeros(2, gpsacq.TIME_TAG_DTYPE)
    tags["valid"] = 1
    ne = np.array([12, 9], np.int32)
    p = qr.par(epochs=4, min_epochs=2)
    info = qr.quality(rec, ne, chans, tags, 95, 4, 33, p)
    assert info.tobytes() == qr.quality(rec, ne, chans, tags, 95, 4, 33, p, direct=True).tobytes()
    R = 95 + 4 * np.arange(33)
    assert not info[R < 100].view(np.uint8).any() and not info[R >= 220, 0].copy().view(np.uint8).any() and not info[R >= 190, 1].copy().view(np.uint8).any()
    assert (info["epochs"][(R >= 100) & (R < 190)] > 0).all()
    assert info[2, 0] == info[3, 0] and info["epochs"][2, 0] == 1 and info["flags"][2, 0] & qr.SHORT   # R = 103, 107: epoch 0
    assert info["epochs"][10, 0] == 4 and info["flags"][10, 0] == qr.FULL and info["weight"][10, 0] == 1.0  # snr 2500
    obs = np.zeros((33, 2), gpsacq.OBS_DTYPE)
    obs["valid"] = info["epochs"] > 0
    obs["weight"], obs["tx_frac"] = 1.0, 0.5e-3
    obs["weight"][0] = 7.0
    out = qr.apply_weights(obs, info)
    assert (out["weight"][0] == 7.0).all() and (out["weight"][obs["valid"] != 0] == info["weight"][obs["valid"] != 0]).all()
    out["weight"] = obs["weight"]
    assert out.tobytes() == obs.tobytes()
    tags["valid"][1] = 0
    assert not qr.quality(rec, ne, chans, tags, 95, 4, 33, p)[:, 1].copy().view(np.uint8).any()


def test_physical_capture_on_the_cpu_model():
    """quality_ref.physical_case through the CPU model of the multi-bit channels (tests/c/track_model_iq.c): this is where the loss
    and the spreads that quality_ref.physical_check asserts with were measured (it prints them), and where the capture's seed is
    checked to keep the channel on the absent PRN below the gate.  tests/test_gpu_quality.py repeats it on the GPU's records."""
    import gpsacq
    import track_iq_helpers as iqh
    buf, p, chans = qr.physical_case()
    _, rec, ne = iqh.run_model_iq(buf, 0, True, (0, 0), chans, p, 1600)
    tags = np.zeros(3, gpsacq.TIME_TAG_DTYPE)
    tags["valid"] = 1
    par = qr.par(epochs=qr.PHYS_WINDOW)
    first, step, n_fix = qr.physical_instants(chans)
    info = qr.quality(rec, ne, chans, tags, first, step, n_fix, par)
    n2 = int(ne[2])
    every = np.zeros(n2, gpsacq.QUALITY_INFO_DTYPE)
    for k, r in enumerate(qr.channel_series(rec["ip"][2, :n2], rec["qp"][2, :n2], par)):
        for name, v in r.items():
            every[name][k] = v
    qr.physical_check(info, every, int(chans["status"][2]), n2, gpsacq.TRACK_LOST)
    # the constants are the measurement, to the digits they are written with
    mean = info["cn0_dbhz"].mean(axis=0)
    assert abs(np.mean(np.array(qr.PHYS_CN0) - mean[:2]) - qr.PHYS_LOSS_DB) < 0.005
    assert np.allclose(info["cn0_dbhz"].std(axis=0, ddof=1)[:2], qr.PHYS_SPREAD_DB, atol=0.0006)
    assert abs((info["cn0_dbhz"][:, 0] - info["cn0_dbhz"][:, 1]).std(ddof=1) - qr.PHYS_DIFF_SPREAD_DB) < 0.0006


def test_default_params_through_ctypes(hip_artifacts):
    import gpsacq
    lib = gpsacq.load_library()
    assert gpsacq.QUALITY_PARAMS_DTYPE.itemsize == 48 and gpsacq.QUALITY_INFO_DTYPE.itemsize == 48
    raw = np.full(1, 0xA5, np.uint8).repeat(48).view(gpsacq.QUALITY_PARAMS_DTYPE)
    assert lib.gpsacq_quality_default_params(raw.ctypes.data_as(ctypes.c_void_p)) == 0
    assert lib.gpsacq_quality_default_params(None) == 1
    want = qr.par()
    assert {k: raw[k][0] for k in raw.dtype.names} == want and qr.params_valid(want)
    assert raw["cn0_min_lin"][0] == 1000.0 and raw["cn0_ref_lin"][0] == 10.0 ** 4.5 and raw["reserved"][0] == 0
    assert gpsacq.quality_params().tobytes() == raw.tobytes()
    got = gpsacq.quality_params(cn0_min_dbhz=25, cn0_ref_dbhz=50, epochs=100, require_lock=0, cn0_cap_dbhz=80.5)
    assert got["cn0_min_lin"][0] == 10.0 ** 2.5 and got["cn0_ref_lin"][0] == 1e5 and got["epochs"][0] == 100 and got["require_lock"][0] == 0
    assert got["cn0_cap_dbhz"][0] == 80.5 and got["min_epochs"][0] == 20
    with pytest.raises(TypeError):
        gpsacq.quality_params(window=3)
    # flags as the header numbers them
    assert (gpsacq.QUALITY_NO_POWER, gpsacq.QUALITY_SATURATED, gpsacq.QUALITY_UNLOCKED, gpsacq.QUALITY_FULL, gpsacq.QUALITY_SHORT) == \
        (qr.NO_POWER, qr.SATURATED, qr.UNLOCKED, qr.FULL, qr.SHORT)


BAD_PARAMS = (dict(epochs=0, min_epochs=0), dict(min_epochs=0), dict(min_epochs=201), dict(epochs=1025), dict(epochs=-5, min_epochs=-7), dict(lock_num=0),
              dict(lock_num=3, lock_den=2), dict(lock_num=1, lock_den=1025), dict(cn0_min_lin=-1.0), dict(cn0_min_lin=math.inf),
              dict(cn0_min_lin=math.nan), dict(cn0_ref_lin=0.0), dict(cn0_ref_lin=-3.0), dict(cn0_ref_lin=math.inf), dict(cn0_ref_lin=math.nan),
              dict(cn0_cap_dbhz=math.inf), dict(cn0_cap_dbhz=math.nan))


@pytest.mark.gpu
def test_invalid_parameters_are_argument_errors():
    """every parameter outside its range: GPSACQ_ERR_ARG from the three entry points, nothing launched and nothing written; the
    edges of the ranges are accepted (this needs an engine, hence a device)"""
    import gpsacq
    import torch
    from nav_helpers import geometry, to_records
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rec = np.zeros((2, 8), gpsacq.TRACK_RECORD_DTYPE)
    rec["sample"] = 1000 + 100 * np.arange(8)
    rec["ip"] = 90
    chans = np.zeros(2, gpsacq.TRACK_CHAN_DTYPE)
    chans["next_sample"] = 1800
    tags = np.zeros(2, gpsacq.TIME_TAG_DTYPE)
    tags["valid"] = 1
    ne = np.array([8, 8], np.int32)
    ephs = to_records(geometry("north")["ephs"])
    with gpsacq.Engine(4.092e6, 5.456e6, 5000.0) as eng:
        lib, h = eng._lib, eng._h
        obs, info = np.full(4 * 2 * 32, 0xA5, np.uint8), np.full(4 * 2 * 48, 0xA5, np.uint8)
        fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_obs, d_info, d_fix = fill(4 * 2 * 32), fill(4 * 2 * 48), fill(4 * 80)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        args = (8, p(ne), p(chans), p(tags), 2, 1000, 150, 4)
        for change in BAD_PARAMS:
            pr = gpsacq.quality_params(**change)
            assert not qr.params_valid(qr.par(pr)), change
            assert lib.gpsacq_quality_observables(h, p(rec), *args, p(pr), p(obs), p(info)) == 1, change
            assert lib.gpsacq_quality_observables_device(h, d_rec.data_ptr(), *args, p(pr), d_obs.data_ptr(), d_info.data_ptr(), 1) == 1, change
            assert lib.gpsacq_fix_quality_track_device(h, p(ephs), len(ephs), d_rec.data_ptr(), *args[:4], None, *args[4:], None, p(pr), d_obs.data_ptr(),
                                                       d_info.data_ptr(), d_fix.data_ptr(), 1) == 1, change
        with pytest.raises(gpsacq.GpsAcqError) as ei:
            eng.quality(rec, ne, chans, tags, 1000, 150, 4, params=gpsacq.quality_params(epochs=1025))
        assert ei.value.code == 1 and "epochs" in str(ei.value)
        eng.synchronize()
        assert (obs == 0xA5).all() and (info == 0xA5).all()
        for d in (d_obs, d_info, d_fix):
            assert (d.cpu().numpy() == 0xA5).all()
        for change in (dict(epochs=1, min_epochs=1), dict(epochs=1024, min_epochs=1024), dict(lock_num=1024, lock_den=1024), dict(cn0_min_lin=0.0),
                       dict(cn0_ref_lin=1e-300), dict(cn0_cap_dbhz=-1e300)):
            pr = gpsacq.quality_params(**change)
            assert qr.params_valid(qr.par(pr)), change
            got = eng.quality(rec, ne, chans, tags, 1000, 150, 4, params=pr)
            assert got.tobytes() == qr.quality(rec, ne, chans, tags, 1000, 150, 4, pr).tobytes(), change
