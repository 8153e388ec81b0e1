"""Register census of the batched launches of the motion-boundary option, from the code-object metadata (no GPU needed; the flags the
library is built with; tests/test_persist_resources.py::_census).

psfm_connect_batch with the option on launches the MB = 1 forms of its two frame kernels -- psfm_chain_step_batch_kernel<R, OPT, 1>
(psfm_motion_boundary.hip) and psfm_seq_batch_kernel<R, WAVES, 1> (psfm_solver_batch_mb.hip) -- and builds the kill maps of all
sequences with psfm_kill_map_batch_kernel.  The MB = 0 forms stay in the units they had (psfm_track.hip, psfm_solver_batch.hip), with
the template arguments they had: the literals below are their figures on the parent of the change that added the MB forms, read with
the same function from the parent's build.

The MB = 1 merged kernel is not its twin with one more comparison.  The twin has 32 bytes of scratch and 9 spilled VGPRs on the
parent (tests/test_solver_resources.py records them as ceilings): it keeps the frame's rebased pointers in VGPR pairs, because the
device-side program counter they are rebased by is loaded per lane, and its replay of Ceres' control flow works on a local copy of the
control block, which the compiler turns into a per-thread array of 2 KB of LDS per field for the one thread that replays.  The MB = 1
form reads the program counter into scalars and keeps ONE copy of the control block per block in LDS (psfm_seq_body<R, true>,
pc_fused_replay<true>, psfm_pc_fused.h): no scratch, no spilled VGPR, a quarter of the LDS, at the same four waves per SIMD."""
import pytest

from test_persist_resources import _census

RATIOS = (0, 1, 2, 4)

# (sgpr_count, sgpr_spill_count, vgpr_count, vgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size) on the parent
KEYS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
PARENT_CHAIN_BATCH = {      # psfm_chain_step_batch_kernel<R, OPT> of psfm_track.hip
    (0, 0): (78, 19, 59, 0, 0, 2176), (0, 1): (78, 35, 59, 0, 0, 2176),
    (1, 0): (78, 15, 59, 0, 0, 2176), (1, 1): (78, 13, 59, 0, 0, 2176),
    (2, 0): (78, 15, 59, 0, 0, 2176), (2, 1): (78, 13, 59, 0, 0, 2176),
    (4, 0): (78, 15, 59, 0, 0, 2176), (4, 1): (78, 13, 59, 0, 0, 2176),
}
PARENT_SEQ_BATCH = {        # psfm_seq_batch_kernel<R, WAVES> of psfm_solver_batch.hip
    (0, 4): (106, 38, 128, 9, 32, 40512), (1, 4): (106, 36, 128, 9, 32, 40512),
    (2, 4): (106, 36, 128, 9, 32, 40512), (4, 4): (106, 36, 128, 9, 32, 40512),
}


def waves_per_simd(vgprs):
    """Waves of a kernel that fit a SIMD's 512 registers per lane (allocated in steps of 8), 8 at the most."""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    out = tmp_path_factory.mktemp("mb_batch")
    return {u: _census(u, out) for u in ("psfm_track.hip", "psfm_solver_batch.hip", "psfm_motion_boundary.hip", "psfm_solver_batch_mb.hip")}


def figures(k):
    return tuple(k[x] for x in KEYS)


def test_mb0_kernels_have_the_parents_figures(units):
    track, solver = units["psfm_track.hip"], units["psfm_solver_batch.hip"]
    assert sorted(t for (n, t) in track if n == "psfm_chain_step_batch_kernel") == sorted(PARENT_CHAIN_BATCH)
    assert sorted(t for (n, t) in solver if n == "psfm_seq_batch_kernel") == sorted(PARENT_SEQ_BATCH)
    for t, want in PARENT_CHAIN_BATCH.items():
        assert figures(track[("psfm_chain_step_batch_kernel", t)]) == want, t
    for t, want in PARENT_SEQ_BATCH.items():
        assert figures(solver[("psfm_seq_batch_kernel", t)]) == want, t


def test_mb_chain_step_batch_kernels_exist_and_keep_the_occupancy(units):
    mb, track = units["psfm_motion_boundary.hip"], units["psfm_track.hip"]
    have = sorted(t for (n, t) in mb if n == "psfm_chain_step_batch_kernel")
    assert have == sorted(t + (1,) for t in PARENT_CHAIN_BATCH), have            # every ratio and OPT the MB = 0 forms have, MB = 1 only
    for t in PARENT_CHAIN_BATCH:
        k, twin = mb[("psfm_chain_step_batch_kernel", t + (1,))], track[("psfm_chain_step_batch_kernel", t)]
        print(t, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, t
        assert waves_per_simd(k["vgpr_count"]) >= waves_per_simd(twin["vgpr_count"]), (t, k["vgpr_count"], twin["vgpr_count"])
        assert k["group_segment_fixed_size"] == twin["group_segment_fixed_size"], t


def test_mb_sequence_kernels_exist_with_the_waves_of_their_twins(units):
    """Four waves per SIMD like the twins: at most 128 VGPRs -- the scalars the form spills travel in lanes of those VGPRs (64 per
    register, v_writelane), so this bound covers them; their number is not compared with the twin's, because the MB form holds in
    scalars the rebased pointers the twin holds in VGPR pairs -- and no more LDS than the twin, of which four blocks fit a CU."""
    mb, solver = units["psfm_solver_batch_mb.hip"], units["psfm_solver_batch.hip"]
    assert sorted(mb) == sorted(("psfm_seq_batch_kernel", t + (1,)) for t in PARENT_SEQ_BATCH), sorted(mb)      # nothing else in the unit
    for t in PARENT_SEQ_BATCH:
        k, twin = mb[("psfm_seq_batch_kernel", t + (1,))], solver[("psfm_seq_batch_kernel", t)]
        print(t, k)
        assert t[1] == 4 and waves_per_simd(k["vgpr_count"]) == waves_per_simd(twin["vgpr_count"]) == 4, t
        assert k["group_segment_fixed_size"] <= twin["group_segment_fixed_size"], t
        assert 4 * k["group_segment_fixed_size"] <= 160 * 1024, t


@pytest.mark.parametrize("R", RATIOS)
def test_mb_sequence_kernels_have_no_scratch(units, R):
    k = units["psfm_solver_batch_mb.hip"][("psfm_seq_batch_kernel", (R, 4, 1))]
    print(R, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0


def test_kill_map_batch_kernels_have_no_scratch_and_no_lds(units):
    mb = units["psfm_motion_boundary.hip"]
    names = sorted(key for key in mb if key[0].startswith("psfm_kill_map_batch"))
    assert names == [("psfm_kill_map_batch_kernel", (0,)), ("psfm_kill_map_batch_kernel", (1,)), ("psfm_kill_map_batch_px_kernel", ())], names
    for key in names:
        k = mb[key]
        print(key, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, key
        assert k["group_segment_fixed_size"] == 0, key
        assert k["vgpr_count"] <= 64, key            # a stream: 8 waves per SIMD hide the latency
