"""Every exported function of include/psfm.h that takes `void* stream` has a row in tests/_stream_gate.py::STREAM_CONTRACT -- async,
synchronising, or exempt with a reason -- and every async and synchronising row is named by a test of
tests/test_gpu_stream_order.py: in COVERS when it runs while a gate holds, in ON_SIDE_STREAM_ONLY when it takes no device input of
the caller's and can only be made with the side stream's pointer.  A new entry point cannot be added without classifying it."""
import os
import re

import _stream_gate as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    """{name: argument text} of every function declared in include/psfm.h (comments removed first)."""
    with open(os.path.join(ROOT, "include", "psfm.h")) as fp:
        text = fp.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = text[text.index('extern "C"'):]
    out = {}
    for m in re.finditer(r"\b(psfm_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        out[m.group(1)] = " ".join(m.group(2).split())
    return out


def stream_functions():
    return sorted(n for n, args in header_functions().items() if re.search(r"\bvoid\s*\*\s*stream\b", args))


def covered_names():
    """{entry point: [tests]} from the COVERS table of the GPU file, read without importing torch or touching a device."""
    import ast
    path = os.path.join(ROOT, "tests", "test_gpu_stream_order.py")
    with open(path) as fp:
        tree = ast.parse(fp.read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    found = {}
    for node in tree.body:
        for name in ("COVERS", "ON_SIDE_STREAM_ONLY"):
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
                found[name] = ast.literal_eval(node.value)
    assert set(found) == {"COVERS", "ON_SIDE_STREAM_ONLY"}, "tests/test_gpu_stream_order.py lacks a table: %s" % sorted(found)
    return found["COVERS"], found["ON_SIDE_STREAM_ONLY"], tests


def test_the_parser_sees_the_whole_header():
    fns = header_functions()
    assert len(fns) > 100 and "psfm_connect" in fns and "psfm_profile_get" in fns and "psfm_last_error" in fns
    st = stream_functions()
    print("%d of %d exported functions take `void* stream`" % (len(st), len(fns)))
    assert "psfm_traj_decode_batch" in st and "psfm_shard_solve_peer" in st and "psfm_result_device" not in st


def test_every_stream_entry_point_is_classified():
    st = stream_functions()
    missing = [n for n in st if n not in sg.STREAM_CONTRACT]
    assert not missing, "entry points that take a stream and have no row in STREAM_CONTRACT: %s" % missing
    stale = sorted(set(sg.STREAM_CONTRACT) - set(st))
    assert not stale, "rows of STREAM_CONTRACT that name no `void* stream` entry point of psfm.h: %s" % stale
    for n in st:
        c = sg.STREAM_CONTRACT[n]
        if isinstance(c, str):
            assert c in ("async", "synchronising"), (n, c)
        else:
            assert len(c) == 2 and c[0] == "exempt" and isinstance(c[1], str) and len(c[1]) > 20 and "\n" not in c[1], (n, c)
    for cls in ("async", "synchronising", "exempt"):
        print("%s: %s" % (cls, ", ".join(n for n in st if sg.contract_class(n) == cls)))


def test_what_the_header_calls_asynchronous_is_classified_async():
    """The rows follow the header's own words: an entry point whose comment says ASYNCHRONOUS / Asynchronous on `stream` is async."""
    for n in ("psfm_traj_augment", "psfm_traj_encode", "psfm_traj_decode", "psfm_traj_decode_batch", "psfm_traj_augment_batch",
              "psfm_traj_encode_batch", "psfm_window_sample_batch", "psfm_labels_merge_window", "psfm_traj_eval_counts", "psfm_sort_records",
              "psfm_sort_records64", "psfm_kill_map", "psfm_kill_map_batch", "psfm_motion_boundary", "psfm_path_consistency_eval"):
        assert sg.STREAM_CONTRACT[n] == "async", n


def test_every_async_and_synchronising_row_is_named_by_a_gpu_test():
    gated, side_only, tests = covered_names()
    assert not set(gated) & set(side_only), "an entry point is either gated or not: %s" % sorted(set(gated) & set(side_only))
    assert all(sg.contract_class(n) == "synchronising" for n in side_only), "an asynchronous entry point can always be gated"
    covers = dict(gated, **side_only)
    for name, by in covers.items():
        assert name in sg.STREAM_CONTRACT and by, name
        for t in by:
            assert t in tests, "the tables name %s, which tests/test_gpu_stream_order.py does not define" % t
    print("run while a gate holds: %s" % ", ".join(sorted(gated)))
    print("made with the side stream's pointer only (no device input of the caller's to gate): %s" % ", ".join(sorted(side_only)))
    bare = [n for n in stream_functions() if sg.contract_class(n) != "exempt" and n not in covers]
    assert not bare, "classified async / synchronising but named by no test: %s" % bare
    listed_exempt = [n for n in covers if sg.contract_class(n) == "exempt"]
    assert not listed_exempt, "exempt rows that a test covers after all (classify them): %s" % listed_exempt
