"""The tap-PAIR flow sampler of particle-sfm_amd/csrc/psfm_device.h (two 16-byte loads per bilinear sample: the persistent loop's fused
flow_check slices) against the four-tap sampler, on the host: tests/host/tap_pairs_host.cpp enumerates every north-west tap column
x0 in [-3, W + 2] for every W in [2, 6] (rows likewise), with distinct sentinel values per pixel and each pixel in turn NaN / +Inf /
-Inf, and compares the bits; then the flow_check verdict of a pixel in both forms around every border.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_pick_rule_matches_four_taps_exhaustively(tmp_path):
    exe = str(tmp_path / "tap_pairs_host")
    cmd = ["g++", "-O2", "-mfma", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "tap_pairs_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    n, bad = [int(x) for x in r.stdout.strip().split("\n")[-1].replace(",", "").split() if x.isdigit()]
    assert bad == 0 and n > 100000
