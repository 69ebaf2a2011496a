"""Reference of the tests of "Snapshot signal quality on an 8-bit IQ capture" of include/gpsacq.h: the measured floor of every fine
record of a multi-bit gpsacq_refine_iq8 and, with that floor, steps 2 to 7 of "Snapshot signal quality" (tests/snapq_ref.py's
Law, reused).  Numpy int64 arrays for the samples, Python integers for the sums, written from the header and not from the kernels:

  * the floor is the DIRECT sum over the record's window o .. o + segments * spm - 1 -- no chunks, no groups, no identity for the
    mean: the sample is tests/refine_iq_ref.py's (v = byte - off - dc);
  * floors() / quality() take the capture, the tasks and the fine records (FINE_DTYPE, or a list of refine_iq_ref.refine's dicts);
  * same(): a QUALITY_INFO_DTYPE array against the reference, every field byte for byte but cn0_dbhz (snapq_ref.CN0_TOL);
  * scene(): the 24-capture scene of the defaults' CPU check, shared by tests/test_snap_quality_iq.py and the tools.

Law is a class so that a test can derive wrong readings of the text from it, one method each."""
import math

import numpy as np

import refine_iq_ref
import snapq_ref

NO_POWER, SHORT, NO_RECORD = snapq_ref.NO_POWER, snapq_ref.SHORT, snapq_ref.NO_RECORD
# gpsacq_snap_quality_default_params_iq8: the gate and the reference level measured on the CPU (tools/snap_quality_floor.py and
# tools/snap_quality_law.py --iq8; the header's PARAMETERS paragraph has the commands and the readings)
DEFAULTS = dict(min_segments=1, reserved=0, cn0_min_lin=1432.4, cn0_ref_lin=10.0 ** 4.86)


def par(params=None, **over):
    """snapq_ref.par with this section's defaults"""
    return snapq_ref.par(dict(DEFAULTS) if params is None else params, **over)


class Law(snapq_ref.Law):
    """Steps 1 and 2 of the section; the rest is snapq_ref.Law's."""

    def window(self, block, segments, stride, spm, n_samples):
        """(o, n) of a record's window, or None where the record is not of this capture"""
        o = block * (stride // 2)
        n = segments * spm
        if block < 0 or o > n_samples or o + n > n_samples:
            return None
        return o, n

    def energy(self, vi, vq, o, n):
        """sum of v_i^2 + v_q^2 over samples o .. o + n - 1, a Python integer"""
        a, b = vi[o:o + n], vq[o:o + n]
        return int((a * a).sum()) + int((b * b).sum())

    def floor_of_window(self, vi, vq, o, n):
        return 2 * self.energy(vi, vq, o, n)

    def floor(self, vi, vq, flags, segments, block, stride, spm, n_samples):
        """(record, floor): record False is NO RECORD, and the floor then reads 0"""
        flags, segments = int(flags), int(segments)
        if flags & snapq_ref.FINE_UNUSABLE or segments <= 0:
            return False, 0
        w = self.window(int(block), segments, stride, spm, n_samples)
        if w is None:
            return False, 0
        return True, self.floor_of_window(vi, vq, *w)

    def evaluate_iq(self, record, floor, segments, prompt, spm, fs, p):
        """the info record from the measured floor: steps 2 to 7 of "Snapshot signal quality" with floor_of = this floor"""
        zero = np.float64(0.0)
        if not record:
            return dict(epochs=0, flags=NO_RECORD, sig=0, noise=0, lin=zero, cn0_dbhz=zero, weight=zero)
        segments, prompt = int(segments), int(prompt)
        if floor == 0:  # an all-zero window
            return dict(epochs=segments, flags=NO_POWER | (SHORT if segments < p["min_segments"] else 0), sig=0, noise=0, lin=zero, cn0_dbhz=zero,
                        weight=zero)
        return _Measured(floor).evaluate(0, segments, prompt, spm, fs, p)


class _Measured(snapq_ref.Law):
    """snapq_ref's steps with a floor that was measured"""

    def __init__(self, floor):
        self.floor = floor

    def floor_of(self, spm, segments):
        return self.floor


LAW = Law()


def _rows(fine):
    return fine if isinstance(fine, list) else np.asarray(fine).ravel()


def floors(iq, stride, tasks, fine, spm, signed=False, mean=None, n_samples=None, law=LAW):
    """gpsacq_snap_floor_iq8 in multi-bit mode: [(record, floor)] per task; tasks a list of (block, prn index) or None for (t, t % 32)"""
    vi, vq = refine_iq_ref.samples(iq, signed, mean)
    n_samples = vi.size if n_samples is None else int(n_samples)
    vi, vq = vi[:n_samples], vq[:n_samples]  # nothing at or beyond byte 2 n_samples is read
    out = []
    for t, r in enumerate(_rows(fine)):
        block = t if tasks is None else int(tasks[t][0])
        out.append(law.floor(vi, vq, r["flags"], r["segments"], block, stride, spm, n_samples))
    return out


def quality(iq, stride, tasks, fine, spm, fs, signed=False, mean=None, n_samples=None, params=None, law=LAW):
    """gpsacq_snap_quality_iq8 in multi-bit mode: (floors as a uint64 array, QUALITY_INFO_DTYPE), both in the shape of fine"""
    import gpsacq
    p = par(params)
    assert snapq_ref.params_valid(p)
    rows = _rows(fine)
    fl = floors(iq, stride, tasks, fine, spm, signed, mean, n_samples, law)
    info = np.zeros(len(rows), gpsacq.QUALITY_INFO_DTYPE)
    for i, (r, (record, floor)) in enumerate(zip(rows, fl)):
        for k, v in law.evaluate_iq(record, floor, r["segments"], r["prompt"], spm, fs, p).items():
            info[k][i] = v
    f = np.array([x[1] for x in fl], np.uint64)
    if isinstance(fine, list):
        return f, info
    shape = np.asarray(fine).shape
    return f.reshape(shape), info.reshape(shape)


same = snapq_ref.same
apply_weights = snapq_ref.apply_weights


def mean_identity(x_i, x_q, dc_i, dc_q):
    """the floor's sum of squares of v = x - dc the way the kernels form it, S2 - 2 (dc_i S_i + dc_q S_q) + n (dc_i^2 + dc_q^2), in
    Python integers; x: the samples with the offset taken off and the mean left in (int64 arrays)"""
    s2 = int((x_i * x_i).sum()) + int((x_q * x_q).sum())
    return s2 - 2 * (dc_i * int(x_i.sum()) + dc_q * int(x_q.sum())) + x_i.size * (dc_i * dc_i + dc_q * dc_q)


# ---- the scene of the defaults' CPU check ------------------------------------------------------------------------------------------
FS, FC, SPM, IF_HZ = 5.456e6, 4.092e6, 5456, 0.4e6
STRIDE = 81920
SCENE_SATS = [(3, 0.2, -4100.0, 100.3, 0.1), (11, 0.2, -2500.0, 4000.7, 0.4), (17, 0.2, -900.0, 2727.45, 0.7), (22, 0.2, 900.0, 1801.2, 0.25),
              (28, 0.05, 2500.0, 5120.6, 0.9), (32, 0.025, 4100.0, 777.77, 0.55)]
SCENE_ABSENT = [(5, 1700.0, 333.3), (9, -3300.0, 4444.4)]


def peak_of(first, dop, cp):
    """the whole sample and the bin of the generator's law at the window's first sample, as tests/test_snapshot_iq.py places them"""
    import gen_ref
    lo_shift = int(round(dop * 40000 / FS))
    ca_rate = refine_iq_ref.nco_words(lo_shift, FC, FS, FC - IF_HZ, refine_iq_ref.REAL)[2]
    pos = float(((first + gen_ref.Fraction(cp)) * gen_ref.Fraction(gen_ref.LAW.chips_per_sample(dop, FS))) % 1023)
    return (30.0, lo_shift, int(round(pos / (ca_rate / 2 ** 32))) % SPM, 0.0)


def scene_capture(k, sats=SCENE_SATS, absent=SCENE_ABSENT, params=None):
    """Capture k of the scene: 16 blocks of 40000 samples at fs = 5.456 MHz, IF 0.4 MHz, scale 16, sigma 1, int8, the mean not
    removed, noise seed 100 + k, first sample k * 40960 * 17 + 8000; refine_iq_ref with 16-block windows, mix_hz = fc - IF, REAL.
    Returns (amplitudes, 0 for the absent PRNs; fine records; floors; info)."""
    import gen_ref
    first, win = k * 40960 * 17 + 8000, 16 * 40000
    g = gen_ref.LAW.iq8(FS, sats, IF_HZ, 16.0, 1.0, 100 + k, first, win)
    iq = gen_ref.LAW.quantise(g["v"], True).ravel()
    rows = [(s[0], s[1], s[2], s[3]) for s in sats] + [(a[0], 0.0, a[1], a[2]) for a in absent]
    tasks = [(0, r[0] - 1) for r in rows]
    peaks = [peak_of(first, r[2], r[3]) for r in rows]
    fine = refine_iq_ref.refine(iq, STRIDE, tasks, peaks, SPM, FC, FS, signed=True, mix_hz=FC - IF_HZ)
    fl, info = quality(iq, STRIDE, tasks, fine, SPM, FS, signed=True, params=params)
    return np.array([r[1] for r in rows]), fine, fl, info


def scene(captures=24):
    """scene_capture(0 .. captures - 1): (amplitudes [captures][8], info [captures][8])"""
    out = [scene_capture(k) for k in range(captures)]
    return np.stack([o[0] for o in out]), np.stack([o[3] for o in out])


def db(lin):
    return 10.0 * math.log10(lin) if lin > 0 else float("-inf")
