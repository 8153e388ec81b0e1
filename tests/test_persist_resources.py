"""Register census of the persistent frame loop and of the per-frame chain kernels, from the code-object metadata.

The loop (psfm_persist.hip) needs all its blocks resident at once: 8 blocks of 256 threads per CU, i.e. 8 waves per SIMD -- at
most 64 VGPRs, no scratch, and an LDS footprint of which eight fit a CU.  Its scalar side is the other half: the compiler allots
78 SGPRs at that occupancy, and what does not fit is spilled to VGPR lanes (v_writelane / v_readlane: VALU instructions that
compute nothing, in a loop that is close to instruction-bound).  Before the argument block was split into a hot and a cold part
the four instantiations spilled 182 / 168 / 168 / 176 scalars; the targets below are what the split was made for
(profiles/EXPERIMENTS.md section 12).  The kernels of psfm_track.hip share psfm_chain.h with the loop: they must not pay for its
diet, so the figures they had before it are their ceilings.

One device-only compile per file (no GPU needed), with the flags the library is built with.
"""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _build_module():
    spec = importlib.util.spec_from_file_location("psfm_build", os.path.join(ROOT, "particle-sfm_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _census(src, out_dir):
    """{(kernel, template arguments): {metadata key: int}} of one translation unit."""
    b = _build_module()
    out = os.path.join(str(out_dir), src.replace(".hip", ".s"))
    cmd = [b.HIPCC] + list(b.FLAGS) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = {}
    for blk in re.split(r"\n  - ", meta)[1:]:
        if ".sgpr_spill_count:" not in blk:
            continue                        # (what follows the list of kernels: target, version)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_Z(\d+)", name)     # Itanium mangling: length-prefixed identifier, then I<template arguments>E
        assert m, name
        ident, rest = name[m.end():m.end() + int(m.group(1))], name[m.end() + int(m.group(1)):]
        t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        targs = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", t.group(1))) if t else ()
        res[(ident, targs)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS}
    return res


@pytest.fixture(scope="module")
def persist(tmp_path_factory):
    return _census("psfm_persist.hip", tmp_path_factory.mktemp("persist"))


@pytest.fixture(scope="module")
def track(tmp_path_factory):
    return _census("psfm_track.hip", tmp_path_factory.mktemp("track"))


# generic ratio: at most a quarter of the 182 scalars it spilled before; compile-time ratios: none
SGPR_SPILL_TARGET = {0: 182 // 4, 1: 0, 2: 0, 4: 0}


@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_persistent_loop_fits_eight_waves_without_spills(persist, R):
    k = persist[("psfm_chain_persist_kernel", (R,))]
    print(R, k)
    assert k["vgpr_count"] <= 64, "more than 64 VGPRs: 7 waves per SIMD, the grid barrier's blocks are no longer all resident"
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, "scratch in the frame loop"
    assert k["sgpr_count"] <= 78, "the scalar allotment at 8 waves per SIMD"
    assert k["group_segment_fixed_size"] <= 12464, "LDS per block grew: eight blocks per CU must fit"
    assert k["sgpr_spill_count"] <= SGPR_SPILL_TARGET[R]


def test_persistent_loop_has_its_four_instantiations(persist):
    assert sorted(t[0] for (n, t) in persist if n == "psfm_chain_persist_kernel") == [0, 1, 2, 4]


# (kernel, (ratio, optimize)) -> scalars spilled before the loop's argument block was split
TRACK_SGPR_SPILL_CEIL = {
    ("psfm_chain_step_kernel", (1, 1)): 13, ("psfm_chain_step_kernel", (2, 1)): 13,
    ("psfm_chain_step_kernel", (4, 1)): 13, ("psfm_chain_step_kernel", (0, 1)): 21,
    ("psfm_chain_step_kernel", (1, 0)): 13, ("psfm_chain_step_kernel", (2, 0)): 13,
    ("psfm_chain_step_kernel", (4, 0)): 13, ("psfm_chain_step_kernel", (0, 0)): 25,
    ("psfm_chain_step_batch_kernel", (1, 1)): 13, ("psfm_chain_step_batch_kernel", (2, 1)): 13,
    ("psfm_chain_step_batch_kernel", (4, 1)): 13, ("psfm_chain_step_batch_kernel", (0, 1)): 35,
    ("psfm_chain_step_batch_kernel", (1, 0)): 15, ("psfm_chain_step_batch_kernel", (2, 0)): 15,
    ("psfm_chain_step_batch_kernel", (4, 0)): 15, ("psfm_chain_step_batch_kernel", (0, 0)): 19,
}


def test_per_frame_kernels_do_not_spill_more_than_before(track):
    for key, ceil in TRACK_SGPR_SPILL_CEIL.items():
        k = track[key]
        print(key, k)
        assert k["sgpr_spill_count"] <= ceil, key
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        assert k["vgpr_count"] <= 64, key
    for key, k in track.items():
        if key not in TRACK_SGPR_SPILL_CEIL:       # flow_check, grid_sample, init ...: nothing spilled, before or now
            assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0, key
