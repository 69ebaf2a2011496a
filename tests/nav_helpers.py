"""Glue between tests/nav_ref.py (plain dicts) and the library's records, shared by the ephemeris and fix tests."""
import numpy as np

import nav_ref

DOUBLE_FIELDS = [k for k in nav_ref.FIELDS if k not in nav_ref.INT_FIELDS]


def to_record(eph, have=7, tow=0):
    """an EPHEMERIS_DTYPE record (shape (1,)) holding a nav_ref ephemeris dict"""
    import gpsacq
    rec = np.zeros(1, gpsacq.EPHEMERIS_DTYPE)
    rec["prn"], rec["have"], rec["tow"] = eph.get("prn", 1), have, eph.get("tow", tow)
    for name in nav_ref.FIELDS:
        rec[name] = eph[name]
    return rec


def to_records(ephs):
    return np.concatenate([to_record(e) for e in ephs])


def assert_fields_exact(rec, eph):
    """integers equal, doubles bit-equal"""
    for name in nav_ref.INT_FIELDS:
        assert int(rec[name][0]) == int(eph[name]), name
    for name in DOUBLE_FIELDS:
        assert np.float64(rec[name][0]).tobytes() == np.float64(eph[name]).tobytes(), (name, rec[name][0], eph[name])


_geometry = {}


def geometry(which="north"):
    """The receiver, constellation and satellite subsets of the fix tests, made once.  which: "north" (the mid-latitude receiver,
    t_oe mid-week), "south" (-60 deg, 170 deg) or "rollover" (receive times that straddle the end of the week).  Subsets are
    the lowest-PDOP choice of 4, 5 and 8 among the satellites above the horizon, and all 12."""
    if which in _geometry:
        return _geometry[which]
    lla = nav_ref.RX_LLA_SOUTH if which == "south" else nav_ref.RX_LLA
    t_oe, ref_ms = (604784, 604_799_900) if which == "rollover" else (nav_ref.T_OE, nav_ref.REF_MS)
    rx = nav_ref.ecef_of(*lla)
    ephs = nav_ref.make_constellation(rx, t_oe=t_oe, ref_ms=ref_ms)
    sat_xyz = np.array([nav_ref.position(e, float(nav_ref.fold_ms(ref_ms - 1000 * t_oe)) * 1e-3)[0] for e in ephs])
    elev = nav_ref.elevation(rx, sat_xyz)
    up = [k for k in range(len(ephs)) if elev[k] > 0]
    subsets = {k: nav_ref.best_subset(rx, sat_xyz, up, k)[0] for k in (4, 5, 8)}
    subsets[12] = list(range(12))
    g = dict(lla=lla, rx=rx, ephs=ephs, sat_xyz=sat_xyz, elevation=elev, subsets=subsets, ref_ms=ref_ms, t_oe=t_oe)
    _geometry[which] = g
    return g


def truth_obs(geo, ref_ms, t_rx):
    """OBS_DTYPE [n_fix][12]: what a receiver at geo's position reads off its twelve replicas at receive times ref_ms[k] + t_rx[k]
    (eph = satellite index, valid = 1, weight = 1)"""
    import gpsacq
    obs = np.zeros((len(t_rx), len(geo["ephs"])), gpsacq.OBS_DTYPE)
    for j, eph in enumerate(geo["ephs"]):
        ms, frac = nav_ref.split_time(ref_ms, nav_ref.truth_tx(eph, geo["rx"], ref_ms, t_rx))
        obs["tx_ms"][:, j], obs["tx_frac"][:, j] = ms, frac
        obs["eph"][:, j] = j
    obs["valid"], obs["weight"] = 1, 1.0
    return obs
