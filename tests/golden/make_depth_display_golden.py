#!/usr/bin/env python3
"""Golden vectors for the display images of sparse depth maps (sfm/convert.py:26-41 and :95), produced by the REFERENCE's own
function: sfm/convert.py is imported UNMODIFIED from the reference checkout (root: oracle/ref_shim.py) and its
normalize_depth_for_display(d, pc, cmap) is followed by matplotlib's cm.ScalarMappable().to_rgba(img, bytes=True) -- the conversion
plt.imsave applies; the generator asserts once that a PNG written by plt.imsave decodes to the same array.  z1, z2 are np.percentile's.
Only a `tqdm` stand-in is installed when the real one is missing.

Writes tests/golden/depth_display.npz: per map `d_<k>` (h, w) f64, `rgba_<k>` (h, w, 4) u8 (absent for a map without a positive
depth), `z_<k>` (2,); per case its name, first map, number of maps (more than one: a batch of one call), pc and colour map; the colour
tables of 'binary' and 'gray'.  Before it writes, the generator asserts that the NumPy model (psfm_sfm.convert.depth_display_host)
equals the reference on every map.  Data only.  Run in the build container, never on the GPU machine:
    python tests/golden/make_depth_display_golden.py
"""
import importlib
import os
import sys
import tempfile
import types
import warnings

os.environ["MPLBACKEND"] = "Agg"

import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
from oracle import ref_shim          # noqa: E402

MAX_BYTES = 900000
CHUNK = 1024                          # valid pixels per block of the compaction (psfm_depth_display_chunk(); the GPU test checks it)


def load_reference():
    if "tqdm" not in sys.modules:
        try:
            importlib.import_module("tqdm")
        except ImportError:
            m = types.ModuleType("tqdm")
            m.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = m
    sfm = os.path.join(ref_shim.REFERENCE_ROOT, "sfm")
    if not os.path.isdir(sfm):
        raise RuntimeError("reference tree not present at %s" % ref_shim.REFERENCE_ROOT)
    sys.path.insert(0, sfm)
    return importlib.import_module("convert")


def sparse(rng, h, w, n, lo=0.5, hi=30.0, coarse=False):
    """(h, w) map with exactly n positive depths at random pixels, 0.0 elsewhere."""
    d = np.zeros(h * w)
    v = rng.uniform(lo, hi, n)
    if coarse:
        v = v.astype(np.float32).astype(np.float64)                       # (compresses better; as many distinct values)
    d[rng.choice(h * w, n, replace=False)] = v
    return d.reshape(h, w)


def low_byte_map():
    """Valid inv that differ only in the lowest byte of their bit pattern: depths next to each other around 1.0."""
    for m in range(1, 4000):
        d = 1.0 + m * 2.0 ** -49 + np.arange(90) * 2.0 ** -52
        bits = (1.0 / (d + 1.0)).view(np.uint64)
        if len(set((bits >> np.uint64(8)).tolist())) == 1 and len(set(bits.tolist())) > 20:
            return d.reshape(9, 10)
    raise AssertionError("no run of depths whose inv share their upper seven bytes")


def cases():
    """[(name, [map], pc, cmap)]"""
    rng = np.random.default_rng(2100)
    out = []
    for h, w in ((1, 1), (1, 5), (5, 1), (3, 7)):
        out.append(("shape_%dx%d" % (h, w), [sparse(rng, h, w, max(1, h * w // 2))], 98, "binary"))
    for w in range(1, 10):                                                # every tail of the vector store
        out.append(("width_%d" % w, [sparse(rng, 3, w, max(1, 2 * w))], 98, "binary"))
    out.append(("batch_widths", [sparse(rng, 3, w, max(1, 2 * w)) for w in range(1, 10)], 98, "binary"))
    out.append(("batch_misaligned", [sparse(rng, 3, 5, 9), sparse(rng, 4, 4, 7), sparse(rng, 2, 3, 4)], 98, "binary"))
    empty = np.array([[0.0, -2.0, -1.0], [np.nan, -0.25, 0.0]])
    out.append(("batch_with_empty", [sparse(rng, 3, 5, 6), empty, sparse(rng, 2, 3, 3), np.zeros((4, 4)), sparse(rng, 1, 7, 5)], 98, "binary"))
    one = np.array([[0.0, -0.5, 3.25, 0.0], [-3.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, -7.5]])
    two = one.copy()
    two[2, 1] = 0.75
    equal = np.where(one != 0, one, 0.0)
    equal[0, :2], equal[2, 2:] = 2.5, 2.5                                 # all positive depths equal: z1 == z2, NaN and +-inf pixels
    equal[0, 2] = 2.5
    for name, d in (("n_1", one), ("n_2", two), ("all_equal", equal)):
        for pc in (98, 50):
            out.append(("%s_pc%d" % (name, pc), [d], pc, "binary"))
    mid = sparse(rng, 13, 17, 120)
    n51, n101 = sparse(rng, 6, 10, 51), sparse(rng, 11, 10, 101)
    for pc in (98, 2, 50, 0, 100):
        out.append(("mid_pc%d" % pc, [mid], pc, "binary"))
        out.append(("n51_pc%d" % pc, [n51], pc, "binary"))
        out.append(("n101_pc%d" % pc, [n101], pc, "binary"))
    ties = np.zeros(12 * 11)
    ties[rng.choice(132, 100, replace=False)] = rng.choice([1.0, 2.0, 2.0, 2.0, 5.0], 100)
    out.append(("ties", [ties.reshape(12, 11)], 98, "binary"))
    out.append(("ties_pc50", [ties.reshape(12, 11)], 50, "gray"))
    out.append(("low_byte", [low_byte_map()], 98, "binary"))
    out.append(("low_byte_pc50", [low_byte_map()], 50, "binary"))
    expo = np.zeros(48)
    expo[:40] = 2.0 ** np.arange(1, 41) - 1.0                              # inv = 2^-k exactly: only the exponent differs
    out.append(("exponent", [rng.permutation(expo).reshape(6, 8)], 98, "binary"))
    out.append(("exponent_pc2", [rng.permutation(expo).reshape(6, 8)], 2, "gray"))
    neg = sparse(rng, 7, 9, 20)
    neg.reshape(-1)[rng.choice(63, 25, replace=False)] = rng.uniform(-5, -0.01, 25)
    neg[0, 0], neg[3, 4], neg[6, 8], neg[2, 2] = -1.0, -1.0, np.nan, np.inf
    out.append(("negative", [neg], 98, "binary"))
    out.append(("negative_gray", [neg], 98, "gray"))
    out.append(("no_positive", [empty], 98, "binary"))
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        out.append(("chunk_%d" % n, [sparse(rng, 40, 41, n)], 98, "binary"))
    out.append(("blocks", [sparse(rng, 300, 400, 40000, coarse=True)], 98, "binary"))
    out.append(("gray", [sparse(rng, 9, 14, 60)], 98, "gray"))
    return out


def main():
    from matplotlib import cm, pyplot as plt
    from psfm_sfm.convert import colour_table, depth_display_host
    ref = load_reference()
    arrays, names, first, count, pcs, cmaps, k = {}, [], [], [], [], [], 0
    checked_png = False
    for name, maps, pc, cmap in cases():
        names.append(name)
        first.append(k)
        count.append(len(maps))
        pcs.append(float(pc))
        cmaps.append(cmap)
        for d in maps:
            d = np.ascontiguousarray(d, np.float64)
            arrays["d_%d" % k] = d
            got, g1, g2 = depth_display_host(d, pc, cmap)
            if np.any(d > 0):
                with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    img = ref.normalize_depth_for_display(d.copy(), pc, cmap)
                    inv = 1.0 / (d + 1)
                want = cm.ScalarMappable().to_rgba(img, bytes=True)
                z = np.array([np.percentile(inv[d > 0], pc), np.percentile(inv[d > 0], 100 - pc)])
                assert want.dtype == np.uint8 and want.shape == d.shape + (4,)
                assert got is not None and np.array_equal(got, want), name
                assert np.array_equal(np.array([g1, g2]).view(np.uint64), z.view(np.uint64)), (name, g1, g2, z)
                arrays["rgba_%d" % k], arrays["z_%d" % k] = want, z
                if not checked_png and d.size > 50:
                    from PIL import Image
                    with tempfile.TemporaryDirectory() as tmp:
                        plt.imsave(os.path.join(tmp, "x.png"), img)
                        assert np.array_equal(np.asarray(Image.open(os.path.join(tmp, "x.png"))), want)
                    checked_png = True
            else:
                assert got is None
            k += 1
    assert checked_png
    for cmap in ("binary", "gray"):
        arrays["table_" + cmap], arrays["bad_" + cmap] = colour_table(cmap)
    assert arrays["bad_binary"].tolist() == [0, 0, 0, 255]
    assert not np.array_equal(arrays["table_binary"][:, 0], 255 - np.arange(256))     # (a table, not the formula)
    arrays.update(case_names=np.array(names), case_first=np.array(first, np.int64), case_count=np.array(count, np.int64),
                  case_pc=np.array(pcs), case_cmap=np.array(cmaps), chunk=np.int64(CHUNK))
    path = os.path.join(HERE, "depth_display.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("depth_display.npz: %d cases, %d maps, %d bytes" % (len(names), k, size))


if __name__ == "__main__":
    main()
