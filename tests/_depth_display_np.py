"""Shared by tests/test_depth_display_host.py and tests/test_gpu_depth_display.py: the fixture tests/golden/depth_display.npz (the
reference's own normalize_depth_for_display followed by matplotlib's byte conversion, tests/golden/make_depth_display_golden.py),
loaded once and never written."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def fixture():
    if not _cache:
        with np.load(os.path.join(GOLDEN, "depth_display.npz")) as z:
            f = {k: z[k] for k in z.files}
        for v in f.values():
            v.setflags(write=False)
        _cache.update(f)
    return _cache


def case_names():
    return fixture()["case_names"].tolist()


def case(name):
    """-> (maps [(h, w) f64], want [(rgba (h, w, 4) u8 or None, z (2,) or None)], pc, cmap)"""
    f = fixture()
    i = case_names().index(name)
    ks = range(int(f["case_first"][i]), int(f["case_first"][i]) + int(f["case_count"][i]))
    maps = [f["d_%d" % k] for k in ks]
    want = [(f.get("rgba_%d" % k), f.get("z_%d" % k)) for k in ks]
    return maps, want, float(f["case_pc"][i]), str(f["case_cmap"][i])


def table_words(cmap):
    """The colour table as the 257 little-endian words the kernels index: 256 entries and the bad one."""
    f = fixture()
    return np.concatenate([f["table_" + cmap].reshape(-1), f["bad_" + cmap]]).view("<u4").copy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
