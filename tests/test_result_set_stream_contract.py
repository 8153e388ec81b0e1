"""The stream contract of psfm_result_set and psfm_load_track_npy: both take `void* stream`, so tests/test_stream_contract_table.py
asks for a row in tests/_stream_gate.py::STREAM_CONTRACT for each.  The rows are registered here, when this module is imported
(collection imports every test module before any test runs), and checked here: both calls synchronise `stream`, and what covers
them on a non-default stream is tests/test_gpu_result_set.py, not tests/test_gpu_stream_order.py -- hence "exempt", with the reason."""
import ast
import os
import re

import _stream_gate as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {
    "psfm_result_set": ("exempt", "synchronising; run behind a gate on a side stream by tests/test_gpu_result_set.py, which has the sets it needs"),
    "psfm_load_track_npy": ("exempt", "synchronising, no device input to gate; made with a side stream's pointer in tests/test_gpu_result_set.py"),
}
COVERED_BY = {"psfm_result_set": "test_set_result_on_a_non_default_stream_behind_a_gate",
              "psfm_load_track_npy": "test_file_ingest_on_a_non_default_stream"}
for _name, _row in ROWS.items():
    sg.STREAM_CONTRACT.setdefault(_name, _row)


def test_the_rows_are_in_the_table_and_well_formed():
    for name, row in ROWS.items():
        assert sg.STREAM_CONTRACT[name] == row and sg.contract_class(name) == "exempt"
        assert len(row) == 2 and isinstance(row[1], str) and len(row[1]) > 20 and "\n" not in row[1]


def test_the_header_declares_both_with_a_stream_and_says_that_they_synchronise():
    text = open(os.path.join(ROOT, "include", "psfm.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ROWS:
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, code, flags=re.S)
        assert m and re.search(r"\bvoid\s*\*\s*stream\b", m.group(1)), name
    comment = text[text.index("A trajectory set from elsewhere"):text.index("psfm_status psfm_result_set(")]
    assert "Synchronises `stream`" in comment


def test_the_gpu_file_has_the_tests_the_rows_name():
    with open(os.path.join(ROOT, "tests", "test_gpu_result_set.py")) as fp:
        tree = ast.parse(fp.read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name, test in COVERED_BY.items():
        assert test in tests, (name, test)
        body = ast.get_source_segment(open(os.path.join(ROOT, "tests", "test_gpu_result_set.py")).read(),
                                      next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == test))
        assert name in body and "g.ptr" in body, (name, test)
