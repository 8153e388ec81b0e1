#!/usr/bin/env python3
"""One line per kernel of csrc/*.hip units: demangled name, instruction lines, sha256 of its normalised assembly text.

    python scripts/kernel_digest.py psfm_solver.hip psfm_solver_fused.hip ... [path/to/another/tree/unit.hip]

Each unit is compiled device-only with the library's flags (as tests/test_persist_resources.py::_census does).  A kernel's text
runs from its label to .Lfunc_end; everything behind ';' is stripped, empty lines are dropped and .LBB<n>_ becomes .LBB_, so that
two units agree on a kernel exactly when the compiler emitted the same code for it, whatever else the module holds.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
import build as psfm_build


def digest(src):
    """[(demangled name, instruction lines, sha256)] of one translation unit, in the order of its assembly."""
    path = src if os.path.exists(src) else os.path.join(psfm_build.CSRC, src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        cmd = [psfm_build.HIPCC] + list(psfm_build.FLAGS) + ["--cuda-device-only", "-S", path, "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit(r.stdout)
        lines = open(out).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    dem = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    rows = []
    for name, d in zip(names, dem):
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[a:b]]
        body = [l for l in body if l.strip()]
        n_ins = sum(1 for l in body if l[0] in " \t" and not l.lstrip().startswith("."))
        rows.append((re.sub(r"^void |\(.*", "", d), n_ins, hashlib.sha256("\n".join(body).encode()).hexdigest()))
    return rows


if __name__ == "__main__":
    for unit in sys.argv[1:]:
        for name, n_ins, h in digest(unit):
            print("%-28s %-44s %6d  %s" % (os.path.basename(unit), name, n_ins, h))
