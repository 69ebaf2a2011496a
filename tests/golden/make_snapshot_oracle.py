#!/usr/bin/env python3
"""Generate tests/golden/snapshot_oracle.npz: what tests/snapshot_oracle.py (the snapshot chain of include/gpsacq.h in mpmath, 40
digits) says about the fix cases of tests/golden/nav_oracle.npz -- its 11 fix sites, their constellations, 8 receive instants each
and the exact vacuum transmit times fix_vac_ms / fix_vac_frac, which are read from that file and not stored again.  Deterministic:
a second run writes the same bytes (tests/test_snapshot_oracle.py checks that).  Needs mpmath; the readers need only numpy.

    python tests/golden/make_snapshot_oracle.py

Every oracle value is stored as the double nearest to it; every input the library gets is a double or an integer stored exactly,
and the oracle is evaluated on those very numbers.  F = 11 fix sites, J = 8 instants, S = 12 satellites; MASKED is the column set
with fix_el >= 5 degrees, ALL all twelve.

  dop_drift [J]                      receiver clock drift of the instant: 2e-6 on even instants, 0 on odd ones
  dop_model [F][J][S]                Hz: the Doppler that makes PASS's res exactly 0 at (site, c drift) with t0 = (fix_ref_ms, 0) and
                                     each column's light time solved to 1e-30 s
  dop_pdop [F][J][2]                 the model's pdop over MASKED and over ALL (metres per m/s)
  dop_phys [F][J][S]                 Hz: L1 (d t_tx / d t_rx / (1 + drift) - 1) of a receiver at rest at the site at the TRUE receive
                                     time, truth_tx differenced over +-0.05 s of receiver time
  dop_diff [F][J][S]                 m/s: (c / L1) (dop_model - dop_phys), the error of the header's approximation
  coarse_dop [F][J][2][2]            (pdop, cdop) of step B's rows at the truth, over MASKED and over ALL
  fix_clock [F][J][S]                the clock correction at the uncorrected time (fix_vac_ms, fix_vac_frac), seconds: the prediction
                                     takes the satellite's place that much early (see tests/test_gpu_snapshot_oracle.py, test 7)
  pred_fs, pred_spm, pred_step_hz, pred_kmax     the engine the grid positions belong to: Engine(4.092e6, 5.456e6, 5000.0)
  pred_site [R], pred_xyz [R][3], pred_rx_ms [R], pred_rx_frac [R], pred_vel [R][5] (status, vx, vy, vz, drift)
                                     R = 2 F J + 1 fix rows.  Row 2 (8 f + j) is A: the site at the true receive time, its velocity
                                     record GPSACQ_VEL_NO_FIX with numbers that must not be read.  Row 2 (8 f + j) + 1 is B: the site moved
                                     by PRED_OFFSET, rx_frac later by PRED_LATE, GPSACQ_VEL_OK with PRED_VEL and drift 2e-6.  The last row
                                     is A of site 0, instant 0 with GPSACQ_VEL_OK, at rest, drift 1e-5: every Doppler off the grid
  pred_tx_ms, pred_tx_frac, pred_doppler_hz, pred_elev_deg, pred_ca_pos, pred_lo_pos [R][S]
                                     the record, and the unrounded tx_frac fs and doppler_hz / step
  tie_site, tie_instant, tie_rx_ms, tie_col, tie_side [T], tie_xyz [T][3], tie_N, tie_x [T][S]
                                     near-tie priors of step A over MASKED (reference = its first column): a prior within 100 km and
                                     30 s at which column tie_col has x within 1e-4 ms of a half-integer and at least 1e-5 ms from
                                     it; tie_side 1: every N is the truth's (up to the row's common integer), 0: tie_col's is one off.
                                     tie_N the oracle's N, tie_x the unrounded x (0 outside MASKED)
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import nav_oracle_data as nod  # noqa: E402
import snapshot_oracle as snap  # noqa: E402
from make_nav_oracle import to_bytes  # noqa: E402
from mpmath import mp, mpf  # noqa: E402

PATH = os.path.join(HERE, "snapshot_oracle.npz")
MASK = math.radians(5.0)
DRIFT = 2e-6
FS, SPM, STEP_HZ, KMAX = 5.456e6, 5456, 5.456e6 / 40000, 36   # gpsacq_get_info of Engine(4.092e6, 5.456e6, 5000.0)
PRED_OFFSET = (60.0, -70.0, 40.0)        # 100.5 m
PRED_LATE = 0.5e-6                       # seconds
PRED_VEL = (25.0, -18.0, 12.0)           # m/s
OFF_GRID_DRIFT = 1e-5                    # 15.8 kHz against a grid of +-4.9 kHz
VEL_OK, VEL_NO_FIX = 0, 2
TIE_SITES, TIE_KM, TIE_SECS = 6, 100.0, 20


def _f(x):
    return float(x)


def make_dopplers(d, out):
    F, J, S = d["fix_vac_ms"].shape
    drift = np.where(np.arange(J) % 2 == 0, DRIFT, 0.0)
    model, phys, pdop = np.zeros((F, J, S)), np.zeros((F, J, S)), np.zeros((F, J, 2))
    diff = np.zeros((F, J, S))
    for f in range(F):
        ephs, site = nod.constellation(f), d["site_xyz"][d["fix_site"][f]]
        for j in range(J):
            ref_ms, g = int(d["fix_ref_ms"][f, j]), snap.C * mpf(float(drift[j]))
            cols = [snap.doppler_column(e, site, g, ref_ms) for e in ephs]
            up = [k for k in range(S) if d["fix_el"][f, j, k] >= MASK]
            pdop[f, j] = [_f(snap._pdop([cols[k][1] for k in up], 4)[0]), _f(snap._pdop([c[1] for c in cols], 4)[0])]
            for s, e in enumerate(ephs):
                ph = snap.physical_doppler(e, site, ref_ms, float(d["fix_t_rx"][f, j]), float(drift[j]))
                model[f, j, s], phys[f, j, s], diff[f, j, s] = _f(cols[s][0]), _f(ph), _f((snap.C / snap.L1) * (cols[s][0] - ph))
    out.update(dop_drift=drift, dop_model=model, dop_pdop=pdop, dop_phys=phys, dop_diff=diff)


def make_coarse(d, out):
    F, J, S = d["fix_vac_ms"].shape
    dop, clock = np.zeros((F, J, 2, 2)), np.zeros((F, J, S))
    for f in range(F):
        ephs, site = nod.constellation(f), d["site_xyz"][d["fix_site"][f]]
        for j in range(J):
            rows = [snap.coarse_row(e, site, d["fix_ref_ms"][f, j], float(d["fix_t_rx"][f, j]), int(d["fix_vac_ms"][f, j, s]),
                                    float(d["fix_vac_frac"][f, j, s]))[0] for s, e in enumerate(ephs)]
            up = [k for k in range(S) if d["fix_el"][f, j, k] >= MASK]
            dop[f, j, 0] = [_f(v) for v in snap.coarse_dilution([rows[k] for k in up])]
            dop[f, j, 1] = [_f(v) for v in snap.coarse_dilution(rows)]
            clock[f, j] = [_f(snap.orc.sat_state(e, int(d["fix_vac_ms"][f, j, s]), float(d["fix_vac_frac"][f, j, s]))[1]) for s, e in enumerate(ephs)]
    out.update(coarse_dop=dop, fix_clock=clock)


def make_predictions(d, out):
    F, J, S = d["fix_vac_ms"].shape
    R = 2 * F * J + 1
    site_of, xyz, rx_ms, rx_frac, vel = np.zeros(R, np.int32), np.zeros((R, 3)), np.zeros(R, np.int32), np.zeros(R), np.zeros((R, 5))
    for f in range(F):
        site = d["site_xyz"][d["fix_site"][f]]
        for j in range(J):
            a = 2 * (J * f + j)
            ms, t = int(d["fix_ref_ms"][f, j]), float(d["fix_t_rx"][f, j])
            site_of[a], xyz[a], rx_ms[a], rx_frac[a], vel[a] = f, site, ms, t, (VEL_NO_FIX, 100.0, -100.0, 100.0, 1e-6)
            late = t + PRED_LATE
            if late >= 1e-3:
                ms, late = (ms + 1) % snap.WEEK_MS, late - 1e-3
            site_of[a + 1], xyz[a + 1], rx_ms[a + 1], rx_frac[a + 1] = f, site + np.array(PRED_OFFSET), ms, late
            vel[a + 1] = (VEL_OK,) + PRED_VEL + (DRIFT,)
    site_of[-1], xyz[-1], rx_ms[-1], rx_frac[-1], vel[-1] = 0, xyz[0], rx_ms[0], rx_frac[0], (VEL_OK, 0.0, 0.0, 0.0, OFF_GRID_DRIFT)
    names = ("tx_ms", "tx_frac", "doppler_hz", "elev_deg", "ca_pos", "lo_pos")
    res = {n: np.zeros((R, S), np.int32 if n == "tx_ms" else np.float64) for n in names}
    for r in range(R):
        ephs = nod.constellation(int(site_of[r]))
        v = tuple(vel[r, 1:]) if vel[r, 0] == VEL_OK else None
        for s, e in enumerate(ephs):
            p = snap.predict(e, xyz[r], int(rx_ms[r]), float(rx_frac[r]), FS, STEP_HZ, v)
            for n in names:
                res[n][r, s] = p[n] if n == "tx_ms" else _f(p[n])
    out.update(pred_fs=np.float64(FS), pred_spm=np.int32(SPM), pred_step_hz=np.float64(STEP_HZ), pred_kmax=np.int32(KMAX), pred_site=site_of,
               pred_xyz=xyz, pred_rx_ms=rx_ms, pred_rx_frac=rx_frac, pred_vel=vel)
    out.update({"pred_" + n: res[n] for n in names})


def _tie_rows(d, f, j):
    """the two rows (truth side, other side) of site f at instant j, or None"""
    ephs, site = nod.constellation(f), d["site_xyz"][d["fix_site"][f]]
    cols = [k for k in range(12) if d["fix_el"][f, j, k] >= MASK]
    frac = [float(d["fix_vac_frac"][f, j, k]) for k in cols]
    rx_ms = int((int(d["fix_ref_ms"][f, j]) + (1 if f % 2 == 0 else -1) * 1000 * TIE_SECS) % snap.WEEK_MS)
    truth = [snap.orc.fold_ms(int(d["fix_vac_ms"][f, j, k]) - rx_ms) for k in cols]
    # directions from the site to the satellites, for the choice of a direction only
    unit = []
    for k in cols:
        p = snap.orc.sat_state(ephs[k], rx_ms, mpf("-0.075"))[0]
        v = np.array([float(p[i]) - site[i] for i in range(3)])
        unit.append(v / np.linalg.norm(v))

    def offset(c, place):
        """how far column c of cols stands from the integer the truth gives it, in milliseconds: continuous in the place"""
        _, _, x, N = snap.step_a(ephs, [cols[0], cols[c]], [frac[0], frac[c]], place, rx_ms)
        return x[1] - N[0] - (truth[c] - truth[0])

    for c in range(1, len(cols)):
        for sign in (1.0, -1.0):
            way = unit[c] - unit[0]
            way = sign * way / np.linalg.norm(way)
            far = offset(c, site + TIE_KM * 1e3 * way)
            if abs(far) < mpf("0.5001"):
                continue
            s = 1 if far > 0 else -1
            rows = []
            for side in (1, 0):
                target = s * (mpf("0.5") - mpf("5e-5") * (1 if side else -1))
                lo, hi = mpf(0), mpf(TIE_KM * 1e3)
                for _ in range(60):
                    mid = (lo + hi) / 2
                    y = offset(c, tuple(mpf(site[i]) + mid * mpf(way[i]) for i in range(3)))
                    if abs(y - target) < mpf("2e-5"):
                        break
                    if (y - target) * s < 0:
                        lo = mid
                    else:
                        hi = mid
                place = np.array([float(mpf(site[i]) + mid * mpf(way[i])) for i in range(3)])
                _, _, x, N = snap.step_a(ephs, cols, frac, place, rx_ms)
                off = [N[i] - truth[i] for i in range(len(cols))]
                gap = abs(abs(x[c] - mp.floor(x[c])) - mpf("0.5"))
                margins = [mpf("0.5") - abs(x[i] - N[i]) for i in range(1, len(cols)) if i != c]
                want = [off[0] + (0 if side or i != c else s) for i in range(len(cols))]
                if not (mpf("1e-5") <= gap <= mpf("1e-4") and min(margins) >= mpf("0.05") and off == want
                        and np.linalg.norm(place - site) <= TIE_KM * 1e3):
                    break
                Nfull, xfull = np.zeros(12, np.int32), np.zeros(12)
                for i, k in enumerate(cols):
                    Nfull[k], xfull[k] = N[i], float(x[i])
                rows.append(dict(site=f, instant=j, rx_ms=rx_ms, col=cols[c], side=side, xyz=place, N=Nfull, x=xfull))
            if len(rows) == 2:
                return rows
    return None


def make_ties(d, out):
    rows = []
    sites = 0
    for f in range(d["fix_vac_ms"].shape[0]):
        got = _tie_rows(d, f, f % 8)
        if got:
            rows += got
            sites += 1
        if sites == TIE_SITES:
            break
    for name, kind in (("site", np.int32), ("instant", np.int32), ("rx_ms", np.int32), ("col", np.int32), ("side", np.int32), ("xyz", np.float64),
                       ("N", np.int32), ("x", np.float64)):
        out["tie_" + name] = np.array([r[name] for r in rows], kind)


def build():
    """every array of the fixture, by name"""
    d = nod.load()
    out = {}
    make_dopplers(d, out)
    make_coarse(d, out)
    make_predictions(d, out)
    make_ties(d, out)
    return out


if __name__ == "__main__":
    data = to_bytes(build())
    with open(PATH, "wb") as fh:
        fh.write(data)
    print("%s: %d bytes" % (PATH, len(data)))
