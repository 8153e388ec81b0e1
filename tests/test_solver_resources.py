"""Register census of the path-consistency solver's kernels over its translation units, from the code-object metadata.

The solver is split by solve form: the launch chain, the resident solve and the host driver (psfm_solver.hip), the fused / frame /
device-paced kernels (psfm_solver_fused.hip) and their batched forms (psfm_solver_batch.hip).  The split moved code and changed none: every kernel and instantiation the single unit had is emitted by
exactly one unit, and none needs more registers, spills, scratch or LDS than it did there.  The ceilings were read with the same
function from the single unit, before the split.

One device-only compile per unit (no GPU needed), with the flags the library is built with.
"""
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_persist_resources import _census

UNITS = ("psfm_solver.hip", "psfm_solver_fused.hip", "psfm_solver_batch.hip")
CEIL_KEYS = ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
# (kernel, template arguments) -> ceilings in the order of CEIL_KEYS
CEIL = {
    ('psfm_batch_pack_kernel', ()): (27, 0, 0, 0, 0),
    ('psfm_batch_set_pc_kernel', ()): (8, 0, 0, 0, 0),
    ('psfm_frame_kernel', (0,)): (126, 26, 0, 16, 40512),
    ('psfm_frame_kernel', (1,)): (126, 26, 0, 16, 40512),
    ('psfm_frame_kernel', (2,)): (126, 26, 0, 16, 40512),
    ('psfm_frame_kernel', (4,)): (126, 26, 0, 16, 40512),
    ('psfm_pc_clear_sel_kernel', ()): (1, 0, 0, 0, 0),
    ('psfm_pc_control_kernel', ()): (99, 14, 0, 160, 9248),
    ('psfm_pc_eval_kernel', ()): (42, 0, 0, 0, 0),
    ('psfm_pc_flush_batch_kernel', ()): (16, 0, 0, 0, 0),
    ('psfm_pc_flush_kernel', ()): (8, 0, 0, 0, 0),
    ('psfm_pc_fused_kernel', (3,)): (127, 0, 0, 0, 40392),
    ('psfm_pc_fused_kernel', (4,)): (125, 0, 0, 0, 40392),
    ('psfm_pc_init_kernel', ()): (146, 0, 0, 160, 19952),
    ('psfm_pc_iter_kernel', ()): (145, 0, 0, 0, 19928),
    ('psfm_pc_load_rows_kernel', ()): (12, 0, 0, 0, 0),
    ('psfm_pc_raise_stall_kernel', ()): (2, 0, 0, 0, 0),
    ('psfm_pc_resident_kernel', (1, 0)): (250, 67, 0, 0, 28560),
    ('psfm_pc_resident_kernel', (1, 1)): (247, 79, 0, 0, 28560),
    ('psfm_pc_resident_kernel', (2, 0)): (256, 61, 15, 64, 53136),
    ('psfm_pc_resident_kernel', (2, 1)): (256, 75, 6, 28, 53136),
    ('psfm_pc_resident_kernel', (3, 0)): (256, 65, 39, 160, 77712),
    ('psfm_pc_resident_kernel', (3, 1)): (256, 81, 32, 124, 77712),
    ('psfm_pc_writeback_kernel', ()): (16, 0, 0, 0, 0),
    ('psfm_seq_batch_kernel', (0, 4)): (128, 38, 9, 32, 40512),
    ('psfm_seq_batch_kernel', (1, 4)): (128, 36, 9, 32, 40512),
    ('psfm_seq_batch_kernel', (2, 4)): (128, 36, 9, 32, 40512),
    ('psfm_seq_batch_kernel', (4, 4)): (128, 36, 9, 32, 40512),
    ('psfm_seq_kernel', (0, 3)): (125, 48, 0, 0, 42560),
    ('psfm_seq_kernel', (0, 4)): (123, 48, 0, 16, 40512),
    ('psfm_seq_kernel', (1, 3)): (125, 53, 0, 0, 42560),
    ('psfm_seq_kernel', (1, 4)): (123, 53, 0, 16, 40512),
    ('psfm_seq_kernel', (2, 3)): (125, 53, 0, 0, 42560),
    ('psfm_seq_kernel', (2, 4)): (123, 53, 0, 16, 40512),
    ('psfm_seq_kernel', (4, 3)): (125, 53, 0, 0, 42560),
    ('psfm_seq_kernel', (4, 4)): (123, 53, 0, 16, 40512),
}


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    out = tmp_path_factory.mktemp("solver")
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(lambda u: _census(u, out), UNITS)))


def test_every_kernel_is_emitted_by_exactly_one_unit(units):
    seen = {}
    for unit, census in units.items():
        for key in census:
            assert key not in seen, "%s is emitted by %s and by %s" % (key, seen[key], unit)
            seen[key] = unit
    assert set(seen) == set(CEIL)
    assert len(CEIL) == 36


def test_no_kernel_needs_more_than_in_the_single_unit(units):
    for unit, census in units.items():
        for key, k in census.items():
            print(unit, key, k)
            for name, ceil in zip(CEIL_KEYS, CEIL[key]):
                assert k[name] <= ceil, (unit, key, name)
