"""Register census of the FRAME-MODE kernels of psfm_solver_multi.hip (psfm_connect_batch's joint redo of the sequences whose solves
reject steps) from the code-object metadata (no GPU needed; the flags the library is built with).

The frame-mode forms run the per-track code of the row-mode multi kernels -- and of the single chain -- with their arguments read
from a table row and rebased to the frame: the row and the rebase cost scalar registers.  They use no scratch, no more VGPRs than the
row-mode kernels of the same code object (which in turn stay at or below the single chain's), and the LDS of the single forms (plus,
pc_init only, the control block that the single kernel keeps in scratch)."""
import pytest

from test_persist_resources import _census

FRAME = ("psfm_pc_multi_frame_init_kernel", "psfm_pc_multi_frame_iter_kernel", "psfm_pc_multi_frame_writeback_kernel",
         "psfm_pc_multi_frame_poll_kernel")
# what the code object says (gfx950, the library's flags): VGPRs of the frame-mode init / iter kernels
PINNED_VGPRS = {"psfm_pc_multi_frame_init_kernel": 146, "psfm_pc_multi_frame_iter_kernel": 145}


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    return {u: _census(u, tmp_path_factory.mktemp(u.split(".")[0])) for u in ("psfm_solver.hip", "psfm_solver_multi.hip")}


def test_the_frame_mode_kernels_exist_and_use_no_scratch(units):
    got = units["psfm_solver_multi.hip"]
    for name in FRAME:
        assert (name, ()) in got, name
        k = got[(name, ())]
        print(name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, name


@pytest.mark.parametrize("frame,row,single", [
    ("psfm_pc_multi_frame_init_kernel", "psfm_pc_multi_init_kernel", "psfm_pc_init_kernel"),
    ("psfm_pc_multi_frame_iter_kernel", "psfm_pc_multi_iter_kernel", "psfm_pc_iter_kernel"),
    ("psfm_pc_multi_frame_writeback_kernel", "psfm_pc_multi_writeback_kernel", "psfm_pc_writeback_kernel")])
def test_frame_mode_kernels_take_no_more_vgprs_than_the_row_mode_kernels(units, frame, row, single):
    f, r = units["psfm_solver_multi.hip"][(frame, ())], units["psfm_solver_multi.hip"][(row, ())]
    s = units["psfm_solver.hip"][(single, ())]
    print(frame, f, "\n", row, r, "\n", single, s)
    if frame in PINNED_VGPRS:
        assert f["vgpr_count"] <= r["vgpr_count"] <= s["vgpr_count"]
        assert f["vgpr_count"] <= PINNED_VGPRS[frame]
    else:
        # the frame-mode write-back does what the SINGLE write-back does and the row-mode one has no use for -- the birth frame of
        # every lane (pc_participates), the frame's statistics and the lane snapshot (pc_writeback_scalars): bounded by the single
        # form (16 VGPRs, far from anything that limits occupancy)
        assert f["vgpr_count"] <= s["vgpr_count"] <= 16
    # LDS as in the single forms (pc_init: plus the control block built in LDS, as the row-mode kernel has it)
    assert f["group_segment_fixed_size"] <= s["group_segment_fixed_size"] + 256
    assert f["group_segment_fixed_size"] <= r["group_segment_fixed_size"]


def test_the_poll_kernel_is_small(units):
    p = units["psfm_solver_multi.hip"][("psfm_pc_multi_frame_poll_kernel", ())]
    q = units["psfm_solver_multi.hip"][("psfm_pc_multi_poll_kernel", ())]
    print(p, "\n", q)
    assert p["vgpr_count"] <= 32 and p["group_segment_fixed_size"] == 0
