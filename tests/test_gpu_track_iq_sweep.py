"""gpsacq_track_iq8's multi-bit complex channels (k_track_iq, csrc/track_iq_kernels.hip) on the GPU against their CPU model
(tests/c/track_model_iq.c) byte for byte and against the independent reference (tests/track_ref.py, complex integer samples) on
every call: the scenarios of track_iq_helpers.sweep_iq on captures from gpsacq_generate_iq8_range at 2.046 .. 40 MHz -- bytes on
both rails (-128 included), means (0, 0), (7, -5) and (-128, 127), int8 and uint8, carriers near +0.26 fs, -0.21 fs and zero,
windows that start off the 8-sample grid (at half the rates above sample 2^33) and whose byte count runs over 2 .. 14 mod 16 --
then 1 to 130 channels, the device entry point and the optional outputs, gpsacq_track_default_params_iq8 against its restatement
up to the supported-RMS boundary, and lock from 60 Hz off at 10, 20 and 40 MHz.

Every comparison is equality of integers; the thresholds are the conditions of the lock runs (track_iq_helpers.assert_locked).
Longest tests, seconds on an MI355X machine, CPU model and audit included: test_channel_counts_iq[130] 2.2,
test_kernel_equals_model_sweep_iq[2.046MHz-0] 2.0 (it compiles the model), test_lock_at_10mhz_hackrf_rate 1.3; the file 20."""
import ctypes
import math

import numpy as np
import pytest

import track_iq_helpers as iqh
import track_ref
from test_track_ref import FS_FC, spm_of

pytestmark = pytest.mark.gpu
_FC = dict(FS_FC)
_IDS = [f"{fs / 1e6:g}MHz" for fs, _ in FS_FC]
PARTS = (("default", "agc", "aid"), ("fll_long", "wrap", "window_terms", "window_tight"), ("epoch_len", "entered_lost", "max_epochs", "ragged_end"))


def _engine(fs):
    import gpsacq
    return gpsacq.Engine(_FC[fs], fs, 5000.0, device=0)  # (fc plays no part in multi-bit channels)


def _inp(eng, fmt):
    signed, dc_i, dc_q = fmt
    return eng.iq8_input(signed=signed, remove_dc=(dc_i, dc_q) != (0, 0), mean=(float(dc_i), float(dc_q)), fs=eng.fs, multibit=1)


def _max_epochs(buf, p):
    return len(buf) // 2 // max(int(p.min_epoch), int(p.max_epoch) // 4) + 2


def _kernel_runner(eng, model=True):
    """run one call on the GPU and in the model: identical records, prompt, n_epochs and channel bytes; then the reference's audit
    of the GPU's output"""
    def run(buf, first, chans, p, max_epochs=None, sum_epochs=None, fmt=(True, 0, 0)):
        if max_epochs is None:
            max_epochs = _max_epochs(buf, p)
        c0 = chans.copy()
        kc = chans.copy()
        prompt, rec, ne = eng.track_iq8(buf, _inp(eng, fmt), kc, first_sample=first, max_epochs=max_epochs, records=True, params=p)
        if model:
            mc = chans.copy()
            mp, mr, mn = iqh.run_model_iq(buf, first, fmt[0], fmt[1:], mc, p, max_epochs)
            assert np.array_equal(ne, mn), (ne, mn)
            for c in range(chans.size):
                n = int(ne[c])
                assert np.array_equal(rec[c, :n], mr[c, :n]), c
                assert np.array_equal(prompt[c, :n], mp[c, :n]), c
            assert kc.tobytes() == mc.tobytes()
        reps = [track_ref.audit(buf, first, c0[c], p, rec[c], ne[c], kc[c], max_epochs=max_epochs, prompt=prompt[c], sum_epochs=sum_epochs, iq=fmt)
                for c in range(chans.size)]
        chans[:] = kc
        return reps, prompt, rec, ne
    return run


def _generate(eng, sats, n, first, seed, case):
    """gpsacq_generate_iq8_range at the window's first sample, then on the host the mean (clamped like the generator's output) and
    the rail mapping"""
    iq = eng.generate_iq8(n, [s[:5] for s in sats], if_hz=case["if_hz"], scale=float(case["scale"]), signed=case["signed"], seed=seed + 1,
                          first_sample=first, nav=np.array([np.asarray(s[5], np.int8) for s in sats]))
    return iqh.to_rails(iqh.add_dc(iq, case["signed"], case["dc"]), case["signed"])


def _capture(eng):
    return lambda sats, n, first, seed, case: _generate(eng, sats, n, first, seed, case)


@pytest.mark.parametrize("part", range(len(PARTS)))
@pytest.mark.parametrize("k", range(len(FS_FC)), ids=_IDS)
def test_kernel_equals_model_sweep_iq(k, part):
    """every scenario of the CPU sweep on the GPU, a third of them per test: the defaults, the AGC both ways, the aid; a long FLL,
    starts within a chip of the code wrap, each window term, tight windows; min / max epoch, a channel that starts LOST, a
    max_epochs cut and a window that ends with an epoch inside its last, incomplete 16-byte group"""
    fs = FS_FC[k][0]
    off = (1 << 33) + 1 + k % 7 if k % 2 else 0
    with _engine(fs) as eng:
        reps, _, first, buf, case = iqh.sweep_iq(fs, capture=_capture(eng), runner=_kernel_runner(eng), first_offset=off, only=PARTS[part])
    assert set(reps) == set(PARTS[part])
    assert k % 2 == 0 or (first > 1 << 33 and 1 <= first % 8 <= 7)
    assert np.asarray(buf).size % 16 == 2 * (1 + k % 7)  # over the rates every even residue 2 .. 14: the byte-wise tail of a group
    lo, hi = iqh.rail_share(buf, case["signed"])
    if fs <= 5.456e6:
        assert lo + hi >= 0.005 and lo > 0 and hi > 0, (lo, hi)
    iqh.check_sweep_reports(reps)
    if "default" in reps:
        assert all(x["stop"] == "window" for x in reps["default"][0])


@pytest.mark.parametrize("fs", [fs for fs, _ in FS_FC], ids=_IDS)
def test_default_params_iq8_against_restatement(fs):
    """gpsacq_track_default_params_iq8 field by field against track_iq_helpers.default_params_iq8 from a tenth of a level to just
    below the supported RMS; just above it GPSACQ_ERR_UNSUPPORTED, and params as they were"""
    import gpsacq
    bound = iqh.iq8_rms_bound(fs)
    with _engine(fs) as eng:
        for rms in (1e-9, 0.1, 0.5, 1.0, float(iqh.IQ_SCALE[fs]), bound / 2, bound / math.sqrt(2), bound * (1 - 1e-9)):
            got, want = eng.track_params_iq8(rms), iqh.default_params_iq8(fs, rms)
            for f, _ in type(got)._fields_:
                assert getattr(got, f) == getattr(want, f), (rms, f, getattr(got, f), getattr(want, f))
        for rms in (bound * (1 + 1e-9), 2 * bound, 1e6, 0.0, -1.0, float("nan"), float("inf")):
            assert iqh.default_params_iq8(fs, rms) is None
            p = gpsacq.TrackParams.from_buffer_copy(bytes(range(1, 1 + ctypes.sizeof(gpsacq.TrackParams))))
            before = bytes(p)
            assert eng._lib.gpsacq_track_default_params_iq8(eng._h, rms, ctypes.byref(p)) == 3, rms  # GPSACQ_ERR_UNSUPPORTED
            assert bytes(p) == before, rms


def _many(eng, fs, case, n_chans, secs, first, rng, n_sats=6):
    """a capture and n_chans channels on it: repeated PRNs, absent PRNs, starts spread over the window, one channel LOST"""
    spm = spm_of(fs)
    prns = rng.choice(np.arange(1, 33), n_sats, replace=False)
    sats = [(int(p), float(rng.uniform(0.12, 0.2)), float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spm)), float(rng.uniform(0, 1)),
             1 - 2 * rng.integers(0, 2, 11)) for p in prns]
    n = int(secs * fs) // 8 * 8 + 5
    buf = _generate(eng, sats, n, first, 3, case)
    p = iqh.default_params_iq8(fs, iqh.capture_rms(buf, case["signed"], case["dc"]))
    chans = []
    for c in range(n_chans):
        s = sats[c % n_sats]
        s_min = first + (int(rng.integers(0, n // 2)) if c % 4 == 3 else int(rng.integers(0, spm)))  # some start late in the window
        ch = iqh.start_chan_iq(fs, case["if_hz"], s[0], s[2], s[3], s[4], s_min, p, dop_err=float(rng.uniform(-80, 80)))
        if c % 7 == 5:  # a PRN that is not in the capture
            ch["prn"] = int([q for q in range(1, 33) if q not in prns][c % (32 - n_sats)])
        chans.append(ch)
    chans = np.concatenate(chans)
    chans["status"][min(2, n_chans - 1)] = 1 if n_chans > 1 else 0
    return buf, chans, p


_MANY = dict(if_hz=-0.21 * 5.456e6, scale=50, signed=False, dc=(7, -5))


@pytest.mark.parametrize("n_chans", [1, 3, 5, 130])
def test_channel_counts_iq(n_chans):
    """a partial workgroup, several workgroups: 1, 3, 5 and 130 channels at 5.456 MHz over 0.2 s (uint8, the mean (7, -5), bytes
    on both rails); the sums of every epoch, at 130 channels of 40 seeded epochs each"""
    fs = 5.456e6
    rng = np.random.default_rng(n_chans)
    fmt = (_MANY["signed"],) + _MANY["dc"]
    with _engine(fs) as eng:
        first = 8 * 12345 + 3
        buf, chans, p = _many(eng, fs, _MANY, n_chans, 0.2, first, rng)
        reps, _, _, ne = _kernel_runner(eng)(buf, first, chans, p, sum_epochs=None if n_chans < 100 else 40, fmt=fmt)
    lo, hi = iqh.rail_share(buf, False)
    assert lo > 0 and hi > 0 and ne.max() > 150
    if n_chans > 1:
        assert reps[2]["stop"] == "entered_lost"
        assert chans["status"][2] == 1


def test_other_forms_give_the_same_channels():
    """gpsacq_track_iq8_device on a 16-byte-aligned device buffer (at a non-zero offset of an allocation), prompt only, records
    only, neither, and max_epochs = 0: the same channels and n_epochs as the full call, the outputs asked for equal to its"""
    import gpsacq
    import torch
    fs = 6.5e6
    case = dict(if_hz=0.26 * fs, scale=35, signed=True, dc=(-128, 127))
    fmt = (True, -128, 127)
    rng = np.random.default_rng(4)
    with _engine(fs) as eng:
        first = (1 << 33) + 8 * 4000 + 5
        buf, chans, p = _many(eng, fs, case, 9, 0.15, first, rng)
        inp = _inp(eng, fmt)
        n = buf.size // 2
        full = chans.copy()
        prompt, rec, ne = eng.track_iq8(buf, inp, full, first_sample=first, records=True, params=p)
        me = prompt.shape[1]
        assert ne.max() > 100
        lib = eng._lib
        raw = np.ascontiguousarray(buf.view(np.uint8))
        for want_prompt, want_rec in ((True, False), (False, True), (False, False)):
            ch = chans.copy()
            pr = np.zeros((ch.size, me, 2), np.int32)
            rc_ = np.zeros((ch.size, me), gpsacq.TRACK_RECORD_DTYPE)
            k = np.zeros(ch.size, np.int32)
            assert lib.gpsacq_track_iq8(eng._h, ctypes.byref(inp), raw.ctypes.data_as(ctypes.c_void_p), n, first, ch.ctypes.data_as(ctypes.c_void_p),
                                        ch.size, ctypes.byref(p), pr.ctypes.data_as(ctypes.c_void_p) if want_prompt else None,
                                        rc_.ctypes.data_as(ctypes.c_void_p) if want_rec else None, me, k.ctypes.data_as(ctypes.c_void_p)) == 0
            assert np.array_equal(k, ne) and ch.tobytes() == full.tobytes()
            for c in range(ch.size):
                if want_prompt:
                    assert np.array_equal(pr[c, :ne[c]], prompt[c, :ne[c]])
                if want_rec:
                    assert np.array_equal(rc_[c, :ne[c]], rec[c, :ne[c]])
            if not want_prompt:
                assert not pr.any()
            if not want_rec:
                assert not rc_.view(np.uint8).any()
        ch = chans.copy()
        _, _, n0 = eng.track_iq8(buf, inp, ch, first_sample=first, max_epochs=0, records=True, params=p)
        assert not n0.any() and ch.tobytes() == chans.tobytes()
        # the device form
        dev = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda:0")
        assert dev.data_ptr() % 16 == 0
        dev[32:32 + raw.size] = torch.from_numpy(raw).to("cuda:0")
        d_prompt = torch.full((chans.size * me * 2,), -7, dtype=torch.int32, device="cuda:0")
        d_rec = torch.zeros(chans.size * me * 40, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ch = chans.copy()
        k = eng.track_iq8_device(dev.data_ptr() + 32, n, inp, ch, first_sample=first, max_epochs=me, d_prompt_ptr=d_prompt.data_ptr(),
                                 d_records_ptr=d_rec.data_ptr(), params=p)
        gp = d_prompt.cpu().numpy().reshape(chans.size, me, 2)
        gr = d_rec.cpu().numpy().view(rec.dtype).reshape(chans.size, me)
    assert np.array_equal(k, ne) and ch.tobytes() == full.tobytes()
    for c in range(chans.size):
        assert np.array_equal(gp[c, :ne[c]], prompt[c, :ne[c]]) and np.array_equal(gr[c, :ne[c]], rec[c, :ne[c]])


def test_lock_at_10mhz_hackrf_rate():
    """The reference's HackRF flow: 10 MHz, the carrier at +2.6 MHz, int8, 1.1 s.  The capture is the one of the CPU test
    (test_track_iq.test_iq8_defaults_lock_at_high_fs, made on the host), so the figures asserted are those measured there; the
    kernel equals the model over all 1099 epochs of both channels, the reference audits it, and the channels lock."""
    fs = 10.0e6
    sats, n, case = iqh.lock_setup(fs)
    buf = iqh.host_lock_capture(fs, sats, n, case)
    p, ch, rms = iqh.lock_params_and_chans(fs, buf, sats, case)
    with _engine(fs) as eng:
        reps, prompt, rec, ne = _kernel_runner(eng)(buf, 0, ch, p, sum_epochs=30, fmt=(case["signed"],) + case["dc"])
    print("fs %g rms %.2f (dev Hz, I/Q power)" % (fs, rms), iqh.assert_locked(fs, case, sats, reps, prompt, rec, ne))


@pytest.mark.parametrize("fs", [20.0e6, 40.0e6], ids=["20MHz", "40MHz"])
def test_lock_at_20_and_40mhz(fs):
    """the same 1.1 s on a capture from gpsacq_generate_iq8_range, without the C model (its share of the time belongs to the CPU
    tests): the reference's audit (the loop arithmetic of all epochs, the sums of 30 per channel) and the lock conditions
    (measured: the carrier within 57.0 / 27.4 Hz, I power 241 / 505 times Q power and up)"""
    sats, n, case = iqh.lock_setup(fs)
    with _engine(fs) as eng:
        buf = _generate(eng, sats, n, 0, 6, case)
        p, ch, rms = iqh.lock_params_and_chans(fs, buf, sats, case)
        got = eng.track_params_iq8(rms)
        assert bytes(got) == bytes(p)
        reps, prompt, rec, ne = _kernel_runner(eng, model=False)(buf, 0, ch, p, sum_epochs=30, fmt=(case["signed"],) + case["dc"])
    print("fs %g rms %.2f (dev Hz, I/Q power)" % (fs, rms), iqh.assert_locked(fs, case, sats, reps, prompt, rec, ne))
