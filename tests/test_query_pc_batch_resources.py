"""Register census of psfm_solver_multi.hip and psfm_query_pc_batch.hip from the code-object metadata (no GPU needed; the flags the
library is built with).

The multi-problem forms of pc_init / pc_iter run the single chain's per-track code with their arguments read from a table row: the
row costs scalar registers, so they need no scratch and no more VGPRs than psfm_pc_init_kernel / psfm_pc_iter_kernel.  The batched
step kernel runs the single step kernel's body and must fit the same 8 waves per SIMD (at most 64 VGPRs); the scan and rows kernels
stay at or below their single forms."""
import pytest

from test_persist_resources import _census


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    return {u: _census(u, tmp_path_factory.mktemp(u.split(".")[0]))
            for u in ("psfm_solver.hip", "psfm_solver_multi.hip", "psfm_query_pc.hip", "psfm_query_pc_batch.hip")}


def _clean(k):
    return k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0


def test_no_kernel_of_the_new_units_uses_scratch(units):
    for u in ("psfm_solver_multi.hip", "psfm_query_pc_batch.hip"):
        assert len(units[u]) > 0
        for key, k in units[u].items():
            print(u, key, k)
            assert _clean(k), (u, key)


@pytest.mark.parametrize("multi,single", [("psfm_pc_multi_init_kernel", "psfm_pc_init_kernel"),
                                          ("psfm_pc_multi_iter_kernel", "psfm_pc_iter_kernel"),
                                          ("psfm_pc_multi_writeback_kernel", "psfm_pc_writeback_kernel")])
def test_multi_problem_kernels_take_no_more_vgprs_than_the_single_chain(units, multi, single):
    m, s = units["psfm_solver_multi.hip"][(multi, ())], units["psfm_solver.hip"][(single, ())]
    print(multi, m, "\n", single, s)
    assert m["vgpr_count"] <= s["vgpr_count"]
    # LDS: the single kernel's, plus (pc_init only) the control block that the single kernel keeps in scratch; far from what limits the
    # occupancy of a 146-VGPR kernel (3 blocks per CU: 60 KB of 160)
    assert m["group_segment_fixed_size"] <= s["group_segment_fixed_size"] + 256


def test_batched_step_kernel_has_both_forms_and_fits_eight_waves(units):
    got = units["psfm_query_pc_batch.hip"]
    assert sorted(t for (n, t) in got if n == "psfm_qpb_step_kernel") == [(0,), (1,)]    # (MB)
    for mb in (0, 1):
        b, s = got[("psfm_qpb_step_kernel", (mb,))], units["psfm_query_pc.hip"][("psfm_query_pc_step_kernel", (mb,))]
        print(mb, b, "\n", s)
        assert b["vgpr_count"] <= 64, "more than 64 VGPRs: fewer than 8 waves per SIMD"
        assert b["vgpr_count"] <= s["vgpr_count"] and b["group_segment_fixed_size"] == 0


@pytest.mark.parametrize("batch,single", [("psfm_qpb_scan_kernel", "psfm_query_pc_scan_kernel"), ("psfm_qpb_rows_kernel", "psfm_query_pc_rows_kernel"),
                                          ("psfm_qpb_scatter_kernel", "psfm_query_pc_scatter_kernel"), ("psfm_qpb_init_kernel", "psfm_query_pc_init_kernel")])
def test_the_other_batched_kernels_stay_at_their_single_forms(units, batch, single):
    b, s = units["psfm_query_pc_batch.hip"][(batch, ())], units["psfm_query_pc.hip"][(single, ())]
    print(batch, b, "\n", single, s)
    assert b["vgpr_count"] <= s["vgpr_count"]
