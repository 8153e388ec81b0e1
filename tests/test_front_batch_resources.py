"""Register census of the batched front end of the motion classifier (psfm_window_sample_batch, psfm_traj_augment_batch,
psfm_traj_encode_batch) from the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage; no GPU needed; the flags the
library is built with).

A batched kernel runs the single kernel's body after it found its window; the window is block-uniform and its table lies in the
kernel arguments, so it may cost scalar registers only: the batched encoder and the batched augment have the VGPR count and the LDS
of their single kernels in the same build, and no new kernel uses scratch.

Figures of this build (gfx950): augment 22 VGPRs, no LDS, single and batched alike (36 and 90 SGPRs).  Encoder: 152 VGPRs, 33 792 B of
LDS, 3 waves per SIMD, single and batched alike.  The encoder's body writes the row a phase exchanges in ONE place
(psfm_enc_phase): with two places the compiler left two floats of the token state in scratch, 12 bytes per lane, in both kernels."""
import os
import re
import subprocess

import pytest

from test_persist_resources import _build_module

FIELDS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}


def _remarks(src, out_dir):
    """{kernel identifier: {field: int}} of one translation unit, from the resource remarks alone."""
    b = _build_module()
    cmd = [b.HIPCC] + list(b.FLAGS) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(b.CSRC, src),
                                       "-o", os.path.join(str(out_dir), src.replace(".hip", ".dev.out"))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    res, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            mm = re.match(r"_Z(\d+)", name)            # Itanium mangling: a length-prefixed identifier
            cur = res.setdefault(name[mm.end():mm.end() + int(mm.group(1))] if mm else name, {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return res


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    d = tmp_path_factory.mktemp("front_batch")
    out = {}
    for src in ("psfm_window_batch.hip", "psfm_augment.hip", "psfm_encoder.hip"):
        out.update(_remarks(src, d))
    return out


NEW = ["psfm_winb_count_kernel", "psfm_winb_first_kernel", "psfm_winb_compact_kernel", "psfm_winb_hash_kernel", "psfm_winb_gather_kernel",
       "psfm_traj_augment_batch_kernel", "psfm_traj_encode_batch_kernel"]


@pytest.mark.parametrize("kernel", NEW)
def test_no_new_kernel_uses_scratch(census, kernel):
    k = census[kernel]
    print(kernel, k)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0


@pytest.mark.parametrize("single,batch", [("psfm_traj_encode_kernel", "psfm_traj_encode_batch_kernel"),
                                          ("psfm_traj_augment_kernel", "psfm_traj_augment_batch_kernel")])
def test_the_window_costs_scalar_registers_only(census, single, batch):
    s, b = census[single], census[batch]
    print(single, s)
    print(batch, b)
    assert b["lds"] == s["lds"] and b["agpr"] == s["agpr"] == 0 and b["occupancy"] == s["occupancy"]
    assert b["vgpr"] == s["vgpr"]
    assert b["scratch"] == s["scratch"] and b["vgpr_spill"] == s["vgpr_spill"] == 0
