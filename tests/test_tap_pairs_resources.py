"""Vector-memory census of the persistent frame loop (psfm_persist.hip), from a device-only `hipcc -S` with the flags the library is
built with (no GPU needed): in the fused flow_check slices the two taps of a row of the backward flow are ONE 16-byte load
(psfm_device.h, tap pairs), so every instantiation of psfm_chain_persist_kernel has 16-byte load sites where it had pairs of 8-byte
ones, and fewer 8-byte + 1-byte load sites than before the pairing (profiles/EXPERIMENTS.md section 14: 71 `global_load_dwordx2` + 9
`global_load_ubyte` sites in every instantiation then, no 16-byte load).  The chain step keeps one load per tap: paired it measured
slower (same section)."""
import collections
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sites per instantiation before the taps were paired (the same for R = 0, 1, 2, 4)
BEFORE = {"global_load_dwordx2": 71, "global_load_ubyte": 9}
# the fused flow_check slice is inlined at three sites (prologue, barrier wait, in front of the arrival), 4 pixels each, 2 rows of B per pixel
FC_PAIR_LOADS = 3 * 4 * 2


def _build_module():
    spec = importlib.util.spec_from_file_location("psfm_build", os.path.join(ROOT, "particle-sfm_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def loads(tmp_path_factory):
    """{R: Counter of global_load mnemonics} of psfm_chain_persist_kernel<R>."""
    b = _build_module()
    out = os.path.join(str(tmp_path_factory.mktemp("tap_pairs")), "psfm_persist.s")
    cmd = [b.HIPCC] + list(b.FLAGS) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "psfm_persist.hip"), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    res, cur = {}, None
    for line in open(out):
        m = re.match(r"_Z25psfm_chain_persist_kernelILi(\d+)EEv\w*:", line)
        if m:
            cur = res.setdefault(int(m.group(1)), collections.Counter())
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            tok = line.split()
            if tok and tok[0].startswith("global_load_"):
                cur[tok[0]] += 1
    return res


def test_every_instantiation_is_counted(loads):
    assert sorted(loads) == [0, 1, 2, 4]


@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_slice_taps_are_pair_loads(loads, R):
    c = loads[R]
    print(R, dict(c))
    # the slices' taps of B are 16-byte loads (today 24 sites: three inlined slices x 4 pixels x 2 rows; the compiler may merge or
    # duplicate sites, so the bound is one per pixel of a slice) ...
    assert c["global_load_dwordx4"] >= FC_PAIR_LOADS // 6
    # ... and what matters: fewer 8-byte + 1-byte load sites than before the pairing
    assert c["global_load_dwordx2"] < BEFORE["global_load_dwordx2"]
    assert c["global_load_dwordx2"] + c["global_load_ubyte"] < BEFORE["global_load_dwordx2"] + BEFORE["global_load_ubyte"]
