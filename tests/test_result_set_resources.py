"""Register census of psfm_result_set.hip from the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage; no GPU needed;
the flags the library is built with), as tests/test_front_batch_resources.py does for the classifier's front end.

The four kernels of psfm_result_set / psfm_load_track_npy move metadata: one lane per given trajectory or per record, no scratch, no
spills, and -- the lowest bad index travels through ONE integer atomicMin, the largest frame through one integer atomicMax per wave
-- no floating-point atomic anywhere in the unit's own code.  The decode stages a block's records in LDS: 256 records of at most 68
bytes and the 15 bytes an unaligned first record can add, in 16-byte vectors."""
import os
import re
import subprocess

import pytest

from test_front_batch_resources import _remarks
from test_persist_resources import _build_module

KERNELS = ["psfm_rs_validate_kernel", "psfm_rs_scatter_kernel", "psfm_rs_decode_kernel", "psfm_rs_span_kernel"]
LDS_DECODE = (256 * 68 + 15 + 15) // 16 * 16            # PSFM_RS_LDS_VECS vectors
# the census of this build (profiles/EXPERIMENTS.md section 36.1): VGPRs, SGPRs
VGPR = {"psfm_rs_validate_kernel": 12, "psfm_rs_scatter_kernel": 11, "psfm_rs_decode_kernel": 15, "psfm_rs_span_kernel": 10}
SGPR = {"psfm_rs_validate_kernel": 20, "psfm_rs_scatter_kernel": 14, "psfm_rs_decode_kernel": 30, "psfm_rs_span_kernel": 14}


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    return _remarks("psfm_result_set.hip", tmp_path_factory.mktemp("result_set_res"))


def test_the_unit_has_its_four_kernels(census):
    assert sorted(k for k in census if k.startswith("psfm_rs_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_kernel_uses_scratch_or_spills(census, kernel):
    k = census[kernel]
    print(kernel, k)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["agpr"] == 0
    assert k["vgpr"] == VGPR[kernel] and k["sgpr"] == SGPR[kernel] and k["occupancy"] == 8
    assert k["lds"] == (LDS_DECODE if kernel == "psfm_rs_decode_kernel" else 0)


def test_no_floating_point_atomic_in_the_units_kernels(tmp_path):
    b = _build_module()
    out = str(tmp_path / "psfm_result_set.s")
    cmd = [b.HIPCC] + list(b.FLAGS) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "psfm_result_set.hip"), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    text = open(out).read()
    seen = 0
    for kernel in KERNELS:
        m = re.search(r"^_Z\d+%s\w*:[^\n]*\n(.*?)^\.Lfunc_end" % kernel, text, flags=re.S | re.M)
        assert m, kernel
        atomics = re.findall(r"^\s+((?:global|flat|ds|buffer)_atomic\w*|ds_(?:add|min|max|pk_add)\w*)", m.group(1), flags=re.M)
        seen += len(atomics)
        assert not any(re.search(r"_f(16|32|64)|bf16|fadd|fmin|fmax|pk_add", a) for a in atomics), (kernel, atomics)
        assert all(re.search(r"_u?(min|max)(_x2)?$", a) for a in atomics), (kernel, atomics)      # integer minima / maxima only
        if kernel == "psfm_rs_scatter_kernel":
            assert atomics == []
    assert seen >= 3        # the two verdicts and the frame maximum are there, as integer minima / maxima
