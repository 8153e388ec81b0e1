"""Resource census of the finalize gather that sums in the write layout (psfm_gather_delta2_kernel, psfm_finalize.hip), from the
code-object metadata.

The kernel is there to keep eight blocks of 256 threads on a CU -- 32 waves, against the 12 that the serial kernel's two tiles allow:
at most 64 VGPRs, no scratch, and an LDS footprint of which eight fit the CU's 160 KB.  The serial kernel stays in the tree as the
A/B form (PSFM_FIN_GATHER=0); its figures are recorded, not bounded.

One device-only compile (no GPU needed), with the flags the library is built with."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
LDS_PER_CU = 160 * 1024
BLOCKS_PER_CU = 8


@pytest.fixture(scope="module")
def finalize(tmp_path_factory):
    """{kernel: {metadata key: int}} of psfm_finalize.hip."""
    spec = importlib.util.spec_from_file_location("psfm_build", os.path.join(ROOT, "particle-sfm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = os.path.join(str(tmp_path_factory.mktemp("finalize")), "psfm_finalize.s")
    cmd = [b.HIPCC] + list(b.FLAGS) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "psfm_finalize.hip"), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = {}
    for blk in re.split(r"\n  - ", meta)[1:]:
        if ".sgpr_spill_count:" not in blk:
            continue                        # (what follows the list of kernels: target, version)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_Z(\d+)", name)     # Itanium mangling: length-prefixed identifier
        if not m:
            continue                        # (rocPRIM's kernels: nested names)
        ident = name[m.end():m.end() + int(m.group(1))]
        res[ident] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS}
    return res


def test_blocked_gather_fits_eight_blocks_per_cu(finalize):
    k = finalize["psfm_gather_delta2_kernel"]
    print(k, "serial form:", finalize["psfm_gather_delta_kernel"])
    assert k["vgpr_count"] <= 64, "more than 64 VGPRs: fewer than 8 waves per SIMD"
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, "spills in the gather"
    assert k["private_segment_fixed_size"] == 0, "scratch in the gather"
    assert 0 < k["group_segment_fixed_size"] * BLOCKS_PER_CU <= LDS_PER_CU, "LDS per block grew: eight blocks per CU must fit"


def test_serial_gather_is_still_built(finalize):
    assert "psfm_gather_delta_kernel" in finalize and "psfm_gather_kernel" in finalize
