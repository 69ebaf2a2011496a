"""Reference of the snapshot signal-quality tests: the model of include/gpsacq.h ("Snapshot signal quality: C/N0 and the weight of
a code-phase observation") in Python integers, numpy.float64 for the named double operations and math.log10, written from that text
and not from the kernel.

  * the info record of one fine record, of an array of them, and the weights written into observations;
  * same(): a QUALITY_INFO_DTYPE array against the reference, every field byte for byte but cn0_dbhz (CN0_TOL);
  * the scene of the statistical check of the weight law, shared by tests/test_snap_quality.py and tools/snap_quality_law.py:
    captures by tests/gen_ref.py, fine records by tests/refine_ref.py, the range error of each against the generator's law.

Law is a class so that a test can derive wrong laws from it, one method each.  Nothing here loads the library except for the record
dtypes."""
import math

import numpy as np

NO_POWER, SHORT, NO_RECORD = 1, 16, 32
FINE_NO_HIT, FINE_SHORT, FINE_NO_POWER, FINE_FEW = 1, 2, 4, 8
FINE_UNUSABLE = FINE_NO_HIT | FINE_NO_POWER | FINE_FEW
DEFAULTS = dict(min_segments=1, reserved=0, cn0_min_lin=500.0, cn0_ref_lin=10.0 ** 4.35)
INT_KEYS = ("min_segments", "reserved")
CN0_TOL = 1e-9  # dB: log10 is the one libm call, and the project holds every cn0_dbhz to this
C_MPS = 299792458.0


def par(params=None, **over):
    """a dict from None (the defaults), a dict or a SNAP_QUALITY_PARAMS_DTYPE record: Python integers and numpy.float64"""
    out = dict(DEFAULTS)
    if params is not None:
        if isinstance(params, dict):
            out.update(params)
        else:
            rec = np.asarray(params).ravel()[0]
            out.update({k: rec[k] for k in rec.dtype.names})
    out.update(over)
    return {k: int(v) if k in INT_KEYS else np.float64(v) for k, v in out.items()}


def params_valid(p):
    return (p["min_segments"] >= 1 and math.isfinite(p["cn0_min_lin"]) and p["cn0_min_lin"] >= 0 and math.isfinite(p["cn0_ref_lin"])
            and p["cn0_ref_lin"] > 0)


class Law:
    """Steps 2, 4 and 6 of the text; a mutant overrides one of them."""

    def floor_of(self, spm, segments):
        return 2 * spm * segments

    def lin_of(self, snr, fs, spm):
        return snr * (np.float64(fs) / np.float64(float(spm)))

    def weight_of(self, lin, db, p):
        if lin < p["cn0_min_lin"]:
            return np.float64(0.0)
        w = lin / p["cn0_ref_lin"]
        return w if w < 1.0 else np.float64(1.0)

    def evaluate(self, flags, segments, prompt, spm, fs, p):
        """the info record of one fine record as a dict"""
        zero = np.float64(0.0)
        flags, segments, prompt = int(flags), int(segments), int(prompt)
        if flags & FINE_UNUSABLE or segments <= 0:
            return dict(epochs=0, flags=NO_RECORD, sig=0, noise=0, lin=zero, cn0_dbhz=zero, weight=zero)
        floor = self.floor_of(spm, segments)
        sig = prompt - floor if prompt > floor else 0
        out = SHORT if segments < p["min_segments"] else 0
        lin, db = zero, zero
        if sig == 0:
            out |= NO_POWER
        else:
            snr = np.float64(float(sig)) / np.float64(float(floor))   # int -> float rounds to nearest even
            lin = self.lin_of(snr, fs, spm)
            db = np.float64(10.0) * np.float64(math.log10(lin))
        weight = zero if out & (NO_POWER | SHORT) else self.weight_of(lin, db, p)
        return dict(epochs=segments, flags=out, sig=sig, noise=floor, lin=lin, cn0_dbhz=db, weight=weight)

    def quality(self, fine, spm, fs, params=None):
        """QUALITY_INFO_DTYPE in the shape of fine (FINE_DTYPE, or a list of refine_ref.refine's dicts)"""
        import gpsacq
        p = par(params)
        assert params_valid(p)
        rows = fine if isinstance(fine, list) else np.asarray(fine).ravel()
        info = np.zeros(len(rows), gpsacq.QUALITY_INFO_DTYPE)
        for i, r in enumerate(rows):
            for k, v in self.evaluate(r["flags"], r["segments"], r["prompt"], spm, fs, p).items():
                info[k][i] = v
        return info if isinstance(fine, list) else info.reshape(np.asarray(fine).shape)


LAW = Law()
quality = LAW.quality


def apply_weights(obs, info):
    """a copy of obs with the weight of every observation whose valid != 0 replaced by info's"""
    out = np.array(obs)
    sel = out["valid"] != 0
    out["weight"][sel] = info["weight"][sel]
    return out


def same(got, ref, label=""):
    """a QUALITY_INFO_DTYPE array against the reference's: cn0_dbhz within CN0_TOL, every other byte equal.  Returns the largest
    difference of cn0_dbhz."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (label, got.shape, ref.shape)
    d = np.abs(got["cn0_dbhz"] - ref["cn0_dbhz"])
    worst = float(d.max()) if d.size else 0.0
    assert worst <= CN0_TOL, (label, worst)
    a = got.copy()
    a["cn0_dbhz"] = ref["cn0_dbhz"]
    if a.tobytes() != ref.tobytes():
        for i, (x, y) in enumerate(zip(a.ravel(), ref.ravel())):
            assert x.tobytes() == y.tobytes(), (label, i, x, y)
    return worst


# ---- the statistical check of the weight law: strong and weak satellites in one capture --------------------------------------------
LAW_FS, LAW_FC, LAW_SPM = 5.456e6, 4.092e6, 5456
LAW_BLOCKS = 16
LAW_STRONG, LAW_WEAK = 0.2, (0.1, 0.07, 0.05, 0.04, 0.03)
LAW_AMPLITUDES = (LAW_STRONG,) * 6 + LAW_WEAK
LAW_PRNS = (2, 5, 9, 12, 17, 21, 24, 26, 29, 31, 32)


def law_capture(seed):
    """One capture of the scene and its fine records: LAW_BLOCKS blocks at 5.456 MHz by gen_ref, noise sigma 1, six satellites at
    LAW_STRONG and one at each of LAW_WEAK, Dopplers uniform within +-4.5 kHz, code phases uniform over the code period; each peak
    placed at the whole sample and the grid bin nearest to the generator's law; refine_ref.refine with the defaults.  Returns
    (amplitudes [11], the records (a list of dicts), the range error of each fine code phase against the law in metres [11])."""
    import gen_ref
    import refine_ref
    rng = np.random.default_rng(seed)
    n = len(LAW_AMPLITUDES)
    dop, phase, carrier = rng.uniform(-4500.0, 4500.0, n), rng.uniform(0.0, LAW_SPM, n), rng.uniform(0.0, 1.0, n)
    sats = [(LAW_PRNS[k], LAW_AMPLITUDES[k], float(dop[k]), float(phase[k]), float(carrier[k])) for k in range(n)]
    y = gen_ref.LAW.bits(LAW_FC, LAW_FS, sats, 1.0, 1000 + seed, 0, LAW_BLOCKS * 40960)["y"]
    bits = np.packbits((y < 0.0).astype(np.uint8), bitorder="little")
    peaks, truth = [], []
    for s in sats:
        chips = (s[3] * gen_ref.LAW.chips_per_sample(s[2], LAW_FS)) % 1023.0  # the code position at sample 0
        truth.append(chips / 1.023e6)
        peaks.append((100.0, int(round(s[2] / (LAW_FS / 40000))), int(round(chips / 1.023e6 * LAW_FS)) % LAW_SPM, 1.0))
    recs = refine_ref.refine(bits, 5120, [(0, s[0] - 1) for s in sats], peaks, LAW_SPM, LAW_FC, LAW_FS, blocks=LAW_BLOCKS)
    wrap = lambda t: (t + 0.5e-3) % 1e-3 - 0.5e-3
    err = np.array([C_MPS * wrap(r["tx_frac"] - t) for r, t in zip(recs, truth)])
    return np.array(LAW_AMPLITUDES), recs, err


def law_table(amps, info, err):
    """Per amplitude over pooled captures (amps, err [n]; info QUALITY_INFO_DTYPE [n]): rows of (amplitude, hits, mean S = sig / noise,
    mean C/N0 of it in dB-Hz, rms range error m, var(strong) / var, mean weight, mean(weight err^2) / mean(err^2 of the strong), the
    same at unit weight)"""
    amps, err = np.asarray(amps), np.asarray(err)
    strong = float((err[amps == LAW_STRONG] ** 2).mean())
    rows = []
    for a in sorted(set(amps.tolist()), reverse=True):
        sel = amps == a
        S = info["sig"][sel].astype(np.float64) / np.maximum(info["noise"][sel].astype(np.float64), 1.0)
        var = float((err[sel] ** 2).mean())
        rows.append((a, int(sel.sum()), float(S.mean()), 10.0 * math.log10(max(S.mean() * LAW_FS / LAW_SPM, 1e-300)), math.sqrt(var), strong / var,
                     float(info["weight"][sel].mean()), float((info["weight"][sel] * err[sel] ** 2).mean()) / strong, var / strong))
    return rows


def law_print(rows, say=print):
    say("amplitude hits  S(mean)  dB-Hz  rms m  var(0.2)/var  weight(mean)  weighted/strong  unit/strong")
    for r in rows:
        say("%9.2f %4d %8.3f %6.2f %6.2f %13.3f %13.4f %16.3f %12.3f" % r)
