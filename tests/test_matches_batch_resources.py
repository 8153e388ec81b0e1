"""Register census of the batched saved-set and match-table kernels (psfm_result_filter_batch, psfm_traj_to_matches_batch,
psfm_labels_to_matches_batch) from the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage; no GPU needed; the flags
the library is built with), as tests/test_front_batch_resources.py does for the classifier's front end.

A batched kernel finds its sequence -- block-uniform, 64 scalar compares over a column in the kernel arguments -- and then applies
the single kernel's rules through the sequence's row of the table in device memory: no new kernel uses scratch or spills, and every
batched kernel has the occupancy of its single kernel in the same build."""
import pytest

from test_front_batch_resources import _remarks


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    d = tmp_path_factory.mktemp("matches_batch_res")
    out = {}
    for src in ("psfm_matches.hip", "psfm_matches_batch.hip", "psfm_window.hip"):
        out.update(_remarks(src, d))
    return out


PAIRS = [("pm_keep_kernel", "pmb_keep_kernel"), ("pm_compact_kernel", "pmb_compact_kernel"), ("pm_kp_off_kernel", "pmb_kp_off_kernel"),
         ("pm_kp_kernel", "pmb_kp_kernel"), ("pm_count_kernel", "pmb_count_kernel"), ("pm_emit_kernel", "pmb_emit_kernel"),
         ("pm_rows_kernel", "pmb_rows_kernel"), ("pm_pairs_kernel", "pmb_pairs_kernel"),
         ("psfm_filter_flag_kernel", "pfb_flag_kernel"), ("psfm_filter_meta_kernel", "pfb_meta_kernel"),
         ("psfm_filter_copy_kernel", "pfb_copy_kernel")]
NEW = [b for _, b in PAIRS] + ["pmb_sizes_kernel", "pfb_sizes_kernel", "pfb_off_kernel"]


@pytest.mark.parametrize("kernel", NEW)
def test_no_new_kernel_uses_scratch(census, kernel):
    k = census[kernel]
    print(kernel, k)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0 and k["agpr"] == 0


@pytest.mark.parametrize("single,batch", PAIRS)
def test_the_batched_kernel_has_the_occupancy_of_its_single_kernel(census, single, batch):
    s, b = census[single], census[batch]
    print(single, s)
    print(batch, b)
    assert b["occupancy"] == s["occupancy"]
    assert b["scratch"] == s["scratch"] == 0 and b["lds"] == s["lds"]
