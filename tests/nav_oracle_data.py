"""Reader of tests/golden/nav_oracle.npz (made by tests/golden/make_nav_oracle.py from tests/nav_oracle.py), shared by
tests/test_nav_oracle.py and tests/test_gpu_nav_oracle.py.  numpy only.

The tolerances are the project's own (tests/test_gpu_fix.py, test_gpu_velocity.py, test_gpu_atm.py), unchanged: against the model
evaluated to 40 digits the fp64 references stay more than a hundred times inside them (tests/test_nav_oracle.py)."""
import os

import numpy as np

import nav_ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nav_oracle.npz")
POS_TOL, CLOCK_TOL, VEL_TOL, DRIFT_TOL = 1e-4, 1e-13, 1e-7, 1e-16
TIME_TOL, ANGLE_TOL, DELAY_TOL, LATLON_TOL, ALT_TOL = 1e-12, 1e-12, 1e-9, 1e-10, 1e-4
SITE_ANTIMERIDIAN, SITE_POLE = 3, 8   # y == 0.0 with x < 0; on the axis
EXCL_EL, EXCL_X, EXCL_AZ = 1, 2, 4

_cache = {}


def load():
    """the fixture's arrays, read once, read-only"""
    if "data" not in _cache:
        with np.load(PATH) as z:
            data = {k: z[k] for k in z.files}
        for v in data.values():
            v.setflags(write=False)
        _cache["data"] = data
    return _cache["data"]


def eph_dicts(rows, fields):
    """nav_ref ephemeris dicts from rows [n][len(fields)]"""
    out = []
    for k, row in enumerate(rows):
        eph = {str(name): (int(v) if name in nav_ref.INT_FIELDS else float(v)) for name, v in zip(fields, row)}
        eph["prn"] = k + 1
        out.append(eph)
    return out


def ephemerides():
    d = load()
    if "ephs" not in _cache:
        _cache["ephs"] = eph_dicts(d["eph"], d["eph_fields"])
    return _cache["ephs"]


def constellation(f):
    d = load()
    return eph_dicts(d["fix_eph"][f], d["eph_fields"])


def atm_params(a, elev_mask=np.radians(5.0)):
    """atm_ref's parameter dict of parameter set a"""
    d = load()
    return dict(alpha=list(d["atm_alpha"][a]), beta=list(d["atm_beta"][a]), elev_mask=float(elev_mask), flags=int(d["atm_flags"][a]))


def angle_diff(a, b):
    return np.abs((np.asarray(a) - np.asarray(b) + np.pi) % (2 * np.pi) - np.pi)
