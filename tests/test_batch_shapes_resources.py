"""Register census of the two launches psfm_connect_batch adds for sequences of different frame sizes, from the code-object metadata
(no GPU needed; the flags the library is built with; tests/test_persist_resources.py::_census).

psfm_flow_check_x2v_shapes_kernel (psfm_track.hip) and psfm_kill_map_shapes_kernel (psfm_motion_boundary.hip) do for a block of a grid
flattened over the sequences what psfm_flow_check_x2v_batch_kernel and psfm_kill_map_batch_kernel<WEVEN> / _px_kernel do for a block of
(chunks, pairs, sequences): the frame's constants come from the sequence's row through scalar loads instead of the kernel arguments.
They are streams like their twins -- no scratch, no spill, no LDS, and no more vector registers than the twin (the kill-map kernel, which
holds all three forms: than the widest of them), so the waves per SIMD that hide their latency are the twins'."""
import pytest

from test_persist_resources import _census


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    out = tmp_path_factory.mktemp("batch_shapes")
    return {u: _census(u, out) for u in ("psfm_track.hip", "psfm_motion_boundary.hip")}


def no_scratch(k):
    return k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["group_segment_fixed_size"] == 0


def test_flow_check_over_shapes_is_the_stream_its_twin_is(units):
    track = units["psfm_track.hip"]
    k, twin = track[("psfm_flow_check_x2v_shapes_kernel", ())], track[("psfm_flow_check_x2v_batch_kernel", ())]
    print("shapes", k, "\ntwin", twin)
    assert no_scratch(k), k
    assert k["vgpr_count"] <= twin["vgpr_count"], (k["vgpr_count"], twin["vgpr_count"])


def test_kill_maps_over_shapes_are_the_stream_their_twins_are(units):
    mb = units["psfm_motion_boundary.hip"]
    k = mb[("psfm_kill_map_shapes_kernel", ())]
    twins = [mb[("psfm_kill_map_batch_kernel", (0,))], mb[("psfm_kill_map_batch_kernel", (1,))], mb[("psfm_kill_map_batch_px_kernel", ())]]
    print("shapes", k, "\ntwins", twins)
    assert no_scratch(k), k
    assert k["vgpr_count"] <= max(t["vgpr_count"] for t in twins), (k["vgpr_count"], [t["vgpr_count"] for t in twins])
