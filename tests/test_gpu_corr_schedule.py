"""GPU tests of where k_corr issues its memory operations inside a sub-transform (pass 2's output twiddles read one pair of rows
ahead of its stores; any later move of the table image's refresh): a change of schedule only, so every cell must stay what it was
WORD FOR WORD.  The fixture tests/golden/corr_schedule_cells.npz holds the cells (max_pwr, max_i, tot_pwr, snr as raw 32-bit words)
that the commit before the schedule change computed on an MI355X for the cases below (tests/golden/make_corr_schedule.py recorded
them); both launch forms (run-time hand-out of cells on / off) must reproduce them.  No reference equivalent: what a cell is stays
pinned by the oracle tests; this file pins that a re-ordering inside the kernel moves no bit.

Cases: nine tasks of the 22-column folded instance from a device task list with one entry the kernel rejects (more than one task per
XCD: a workgroup carries its table image across a unit boundary); one task with a one-point Doppler window (first and last
sub-transform of a workgroup, no next cell); a 35 Hz grid (293 points = 3 chunks of 98: a void ticket at the end of the last
chunk); the 12-column instance with two non-coherent sums in registers and the 33-column one (they share pass 2's function)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = "corr_schedule_cells.npz"
NOTT = ("synth_nott_fs5456.bin", 4.092e6, 5.456e6, 5000.0)   # BASELINE configs[1]: 73 bins, 22 columns (FOLD)
NINE = [(0, 0), (1, 20), (2, 28), (3, 3), (-1, 2), (4, 29), (5, 30), (6, 31), (7, 7)]  # task 4 is rejected by the kernel


def _words(cells):
    return np.ascontiguousarray(cells).view(np.uint32).reshape(cells.shape + (4,)).copy()


def _read(golden_dir, name, n_blocks=None):
    buf = open(os.path.join(golden_dir, name), "rb").read()
    n = len(buf) // 5120 if n_blocks is None else n_blocks
    return buf[:n * 5120]


class _NineTasks:
    """configs[1], nine tasks x 73 bins from a device task list (torch tensors stay alive with the object)"""
    def __init__(self, gpsacq, golden_dir):
        import torch
        self.torch, self.gpsacq = torch, gpsacq
        self.dev = torch.device("cuda", 0)
        buf = np.frombuffer(_read(golden_dir, NOTT[0], 8), dtype=np.uint8)
        self.d_bits = torch.from_numpy(buf.copy()).to(self.dev)
        self.d_tasks = torch.from_numpy(np.array(NINE, dtype=np.int32)).to(self.dev)
        self.eng = gpsacq.Engine(*NOTT[1:])
        assert self.eng.acc_columns == 22 and self.eng.num_doppler == 73

    def run(self):
        torch, e = self.torch, self.eng
        d_cells = torch.full((len(NINE), e.num_doppler, 4), 0x55, dtype=torch.int32, device=self.dev)
        d_pk = torch.zeros((len(NINE), 4), dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()
        e.search_device(self.d_bits.data_ptr(), 8, d_pk.data_ptr(), d_tasks_ptr=self.d_tasks.data_ptr(), n_tasks=len(NINE),
                        d_cells_ptr=d_cells.data_ptr(), sync=True)
        return d_cells.cpu().numpy().view(np.uint32).reshape(len(NINE), e.num_doppler, 4)

    def close(self):
        self.eng.close()


def case_nine_tasks(gpsacq, golden_dir, handout):
    c = _NineTasks(gpsacq, golden_dir)
    try:
        c.eng.set_cell_handout(handout)
        return c.run()
    finally:
        c.close()


def case_one_point(gpsacq, golden_dir, handout):
    with gpsacq.Engine(*NOTT[1:]) as eng:
        eng.set_cell_handout(handout)
        eng.set_doppler_window(6, 1)
        cells, _ = eng.search(_read(golden_dir, NOTT[0], 1), tasks=[(0, 0)])
        assert cells.shape == (1, 1)
        return _words(cells)


def case_chunked_grid(gpsacq, golden_dir, handout):
    with gpsacq.Engine(*NOTT[1:]) as eng:
        eng.set_cell_handout(handout)
        eng.set_doppler_step(35.0)
        assert eng.num_doppler == 293 and eng.acc_columns == 22
        cells, _ = eng.search(_read(golden_dir, NOTT[0], 2), tasks=[(1, 20)])
        return _words(cells)


def case_12_columns_ncreg(gpsacq, golden_dir, handout):
    rtl = _read(golden_dir, "synth_rtl_fs2800.bin")
    with gpsacq.Engine(0.62e6, 2.8e6, 5000.0) as eng:
        eng.set_cell_handout(handout)
        assert eng.acc_columns == 12
        stride = eng.aligned_stride()
        eng.set_noncoherent(2, 1)
        cells, _ = eng.search(rtl, tasks=[(0, 0), (1, 20)], stride=stride)
        return _words(cells)


def case_33_columns(gpsacq, golden_dir, handout):
    with gpsacq.Engine(2.046e6, 8.184e6, 5000.0) as eng:
        eng.set_cell_handout(handout)
        assert eng.acc_columns == 33
        cells, _ = eng.search(_read(golden_dir, "gps_sig_tmp.bin", 4), tasks=[(0, 0), (3, 5)])
        return _words(cells)


CASES = {"nine_tasks": case_nine_tasks, "one_point": case_one_point, "chunked_grid": case_chunked_grid,
         "ncreg_12": case_12_columns_ncreg, "cols_33": case_33_columns}


@pytest.fixture(scope="module")
def gpsacq_mod():
    import gpsacq
    gpsacq.load_library()
    return gpsacq


@pytest.fixture(scope="module")
def fixture_cells(golden_dir):
    with np.load(os.path.join(golden_dir, FIXTURE)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("handout", [True, False], ids=["persistent", "one_workgroup_per_cell"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cells_equal_the_recorded_words(gpsacq_mod, golden_dir, fixture_cells, name, handout):
    got = CASES[name](gpsacq_mod, golden_dir, handout)
    want = fixture_cells[name]
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d words differ, first at %s: %08x != %08x" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def test_rejected_task_keeps_its_marker(fixture_cells):
    """(the fixture itself: the rejected task's cells are the kernel's marker, every other cell is a real one)"""
    w = fixture_cells["nine_tasks"]
    assert (w[4, :, 1].view(np.int32) == -1).all() and (w[4, :, 0] == 0).all()
    assert (np.delete(w, 4, axis=0)[:, :, 1].view(np.int32) >= 0).all()


def test_twenty_launches_in_a_row_are_the_first(gpsacq_mod, golden_dir, fixture_cells):
    """A table image left over from the previous launch's last sub-transform, or a DMA that lands late, would show as a launch that
    differs from the first."""
    c = _NineTasks(gpsacq_mod, golden_dir)
    try:
        first = c.run()
        assert np.array_equal(first, fixture_cells["nine_tasks"])
        for k in range(1, 20):
            assert np.array_equal(c.run(), first), k
    finally:
        c.close()
