"""Register census of psfm_query_batch.hip from the code-object metadata (no GPU needed; the flags the library is built with).

The batched tracking kernel of psfm_track_queries_batch runs the single kernel's per-lane loop with its arguments read from a table
row; like the single kernel it must fit 8 waves per SIMD -- at most 64 VGPRs -- with no scratch and no spilled scalars."""
import pytest

from test_persist_resources import _census


@pytest.fixture(scope="module")
def query_batch(tmp_path_factory):
    return _census("psfm_query_batch.hip", tmp_path_factory.mktemp("query_batch"))


def test_batched_tracking_kernel_has_its_four_instantiations(query_batch):
    assert sorted(t for (n, t) in query_batch if n == "psfm_query_batch_track_kernel") == [(0, 0), (0, 1), (1, 0), (1, 1)]   # (MB, BACK)


@pytest.mark.parametrize("targs", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_batched_tracking_kernel_fits_eight_waves_without_spills(query_batch, targs):
    k = query_batch[("psfm_query_batch_track_kernel", targs)]
    print(targs, k)
    assert k["vgpr_count"] <= 64, "more than 64 VGPRs: fewer than 8 waves per SIMD"
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0


def test_no_kernel_of_the_unit_spills(query_batch):
    for key, k in query_batch.items():
        print(key, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
