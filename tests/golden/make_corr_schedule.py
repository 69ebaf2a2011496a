"""Records tests/golden/corr_schedule_cells.npz: the cells of tests/test_gpu_corr_schedule.py's cases as raw 32-bit words, computed on
an MI355X by the tree this script is run from.  It was run on the commit BEFORE the correlator's schedule change (the one-workgroup-
per-cell form and the persistent form agreed word for word, which the script checks); re-run it only when a change is MEANT to move
the cells.  Usage: python tests/golden/make_corr_schedule.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "gnss-gps-sdr_amd", "python"))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import gpsacq
    import test_gpu_corr_schedule as t
    gpsacq.load_library()
    out = {}
    for name, fn in sorted(t.CASES.items()):
        on, off = fn(gpsacq, HERE, True), fn(gpsacq, HERE, False)
        assert on.dtype == np.uint32 and np.array_equal(on, off), name
        out[name] = on
        print(name, on.shape, "%d bytes" % on.nbytes, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, t.FIXTURE)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
