"""The rules of psfm_result_set and psfm_load_track_npy without a GPU: particle-sfm_amd/csrc/psfm_result_set.h -- the validation
verdict with its lowest bad index, the expansion to index == id, the footer check, the record decode block by block as the kernel
stages it -- compiled for the host by tests/host/result_set_host.cpp and compared with a NumPy statement of the same rules and with
point_trajectory/reference_pickle.py's own field extraction.  Every equality is exact: nothing here rounds."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 2 ** 64 - 1
ID_END, FRAME_END = 1 << 28, 1 << 30
BAD_ID, BAD_ORDER, BAD_LEN, BAD_BIRTH, BAD_END, BAD_TEMPLATE, BAD_BN, BAD_SPAN = 1, 2, 3, 4, 5, 8, 9, 10
FOOT_OK, FOOT_SHORT, FOOT_MAGIC, FOOT_END, FOOT_REC_SIZE, FOOT_RECORDS, FOOT_POINTS = range(7)
FIELDS = ("id", "b", "bn", "s", "e", "n")
REC = 63          # bytes of one record as point_trajectory/reference_pickle.py writes it (its _record_template() is the definition)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("result_set") / "libresult_set_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "tests", "host"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "result_set_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp, lg, u64 = ctypes.c_void_p, ctypes.c_long, ctypes.c_uint64
    L.psfm_host_rs_id_end.restype = L.psfm_host_rs_frame_end.restype = lg
    L.psfm_host_rs_validate.argtypes = [lg, vp, vp, vp, ctypes.c_int]
    L.psfm_host_rs_validate.restype = u64
    L.psfm_host_rs_verdict_index.argtypes = [u64]
    L.psfm_host_rs_verdict_index.restype = lg
    L.psfm_host_rs_verdict_reason.argtypes = [u64]
    L.psfm_host_rs_expand.argtypes = [lg, vp, vp, vp, lg, vp, vp, vp]
    L.psfm_host_rs_expand.restype = None
    L.psfm_host_rs_spans.argtypes = [lg, vp, vp, vp, vp]
    L.psfm_host_rs_spans.restype = u64
    L.psfm_host_rs_footer.argtypes = [vp, lg, lg, vp]
    L.psfm_host_rs_template_ok.argtypes = [vp, ctypes.c_int, vp]
    L.psfm_host_rs_decode.argtypes = [vp, lg, lg, lg, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.psfm_host_rs_decode.restype = u64
    return L


def i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).astype(np.int32))


# ---- the NumPy statement ---------------------------------------------------------------------------------------------------------

def verdict_np(ids, birth, length):
    """(lowest bad index, its first reason) or None."""
    ids, birth, length = (np.asarray(a, np.int64) for a in (ids, birth, length))
    why = np.zeros(len(ids), np.int64)
    prev = np.concatenate([[-1], ids[:-1]])
    for code, bad in ((BAD_END, birth + length > FRAME_END), (BAD_BIRTH, birth < 0), (BAD_LEN, length < 1),
                      (BAD_ORDER, (np.arange(len(ids)) > 0) & (prev >= ids)), (BAD_ID, (ids < 0) | (ids >= ID_END))):
        why[bad] = code                                    # (later rules of the list come first in the header)
    bad = np.flatnonzero(why)
    return (int(bad[0]), int(why[bad[0]])) if len(bad) else None


def expand_np(ids, birth, length):
    n_result = int(ids[-1]) + 1 if len(ids) else 0
    db, dl = np.zeros(n_result, np.int32), np.zeros(n_result, np.int32)
    db[ids], dl[ids] = birth, length
    off = np.zeros(n_result + 1, np.int64)
    np.cumsum(dl, out=off[1:])
    return db, dl, off


def run_validate(host, ids, birth, length):
    a, b, c = i32(ids), i32(birth), i32(length)
    out = []
    for reverse in (0, 1):                                 # any lane order gives the same minimum
        v = host.psfm_host_rs_validate(len(a), a.ctypes.data, b.ctypes.data, c.ctypes.data, reverse)
        out.append(None if v == NONE else (host.psfm_host_rs_verdict_index(v), host.psfm_host_rs_verdict_reason(v)))
    assert out[0] == out[1]
    return out[0]


def test_the_bounds(host):
    assert host.psfm_host_rs_id_end() == ID_END and host.psfm_host_rs_frame_end() == FRAME_END
    assert host.psfm_host_rs_block() == 256 and host.psfm_host_rs_rec_max() >= REC


GOOD = dict(ids=[2, 3, 7, 8, 20], birth=[0, 4, 1, 0, 9], length=[3, 1, 5, 2, 4])


@pytest.mark.parametrize("name,where,value,reason", [
    ("ids", 0, -1, BAD_ID), ("ids", 4, ID_END, BAD_ID), ("ids", 0, 3, BAD_ORDER), ("ids", 4, 8, BAD_ORDER), ("ids", 2, 3, BAD_ORDER),
    ("length", 0, 0, BAD_LEN), ("length", 4, -2, BAD_LEN), ("birth", 0, -1, BAD_BIRTH), ("birth", 4, -5, BAD_BIRTH),
    ("birth", 0, FRAME_END - 2, BAD_END), ("birth", 4, FRAME_END - 3, BAD_END), ("length", 4, 2 ** 31 - 1, BAD_END)])
def test_each_refusal_names_the_lowest_bad_index(host, name, where, value, reason):
    s = {k: list(v) for k, v in GOOD.items()}
    assert run_validate(host, **s) is None and verdict_np(**s) is None
    s[name][where] = value
    got = run_validate(host, **s)
    assert got == verdict_np(**s)
    # ids[0] = 3 makes entry 1 the offender (3 >= 3 is read by lane 1); every other case names the entry that was changed
    assert got == ((1 if (name, where, value) == ("ids", 0, 3) else where), reason)


def test_two_bad_entries_the_lower_one_wins(host):
    s = {k: list(v) for k, v in GOOD.items()}
    s["length"][3] = 0
    s["birth"][1] = -4
    assert run_validate(host, **s) == verdict_np(**s) == (1, BAD_BIRTH)
    s["ids"][1] = 1                                        # entry 1 now breaks two rules: the header's first one is reported
    assert run_validate(host, **s) == verdict_np(**s) == (1, BAD_ORDER)


@pytest.mark.parametrize("ids,ok", [([0], True), ([5], True), ([0, ID_END - 1], True), ([ID_END], False), ([0, ID_END], False)])
def test_id_range(host, ids, ok):
    got = run_validate(host, ids, [0] * len(ids), [1] * len(ids))
    assert got == verdict_np(ids, [0] * len(ids), [1] * len(ids))
    assert (got is None) == ok and (ok or got == (len(ids) - 1, BAD_ID))


def test_frame_range_edge(host):
    assert run_validate(host, [0], [FRAME_END - 4], [4]) is None
    assert run_validate(host, [0], [FRAME_END - 4], [5]) == (0, BAD_END)


def test_random_sets_against_numpy(host):
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        ids = np.cumsum(rng.integers(1, 4, n)) - 1
        birth, length = rng.integers(0, 30, n), rng.integers(1, 12, n)
        for _ in range(int(rng.integers(0, 3))):
            k, j = int(rng.integers(0, 5)), int(rng.integers(0, n))
            if k == 0: ids[j] = rng.choice([-1, ID_END, ids[j - 1] if j else -3])
            if k == 1: length[j] = rng.choice([0, -1])
            if k == 2: birth[j] = -1
            if k == 3: birth[j] = FRAME_END - 1
        assert run_validate(host, ids, birth, length) == verdict_np(ids, birth, length)


@pytest.mark.parametrize("ids,birth,length", [
    ([3, 4, 5], [1, 0, 2], [2, 3, 1]),                      # a gap at the front
    ([0, 1, 6, 7, 9], [0, 1, 2, 3, 4], [4, 1, 2, 9, 3]),    # gaps in the middle
    ([0, 1, 2, 3], [5, 0, 1, 0], [1, 2, 3, 4]),             # none
    ([], [], []), ([0], [7], [1]), ([11], [0], [1])])       # n_traj 0 and 1, a trajectory of length 1
def test_expansion_against_numpy(host, ids, birth, length):
    a, b, c = i32(ids), i32(birth), i32(length)
    db_w, dl_w, off_w = expand_np(a, b, c)
    n_result = len(db_w)
    db, dl, off = np.full(n_result, -7, np.int32), np.full(n_result, -7, np.int32), np.full(n_result + 1, -7, np.int64)
    host.psfm_host_rs_expand(len(a), a.ctypes.data, b.ctypes.data, c.ctypes.data, n_result, db.ctypes.data, dl.ctypes.data, off.ctypes.data)
    assert np.array_equal(db, db_w) and np.array_equal(dl, dl_w) and np.array_equal(off, off_w)
    absent = np.setdiff1d(np.arange(n_result), a)
    assert np.all(dl[absent] == 0) and np.all(db[absent] == 0) and np.all(off[absent + 1] == off[absent])
    assert int(off[-1]) == int(np.sum(c))
    # the records' slices are the dense offsets at the ids
    s, e = i32(np.cumsum(c) - c), i32(np.cumsum(c))
    assert host.psfm_host_rs_spans(len(a), a.ctypes.data, s.ctypes.data, e.ctypes.data, off.ctypes.data) == NONE
    if len(a):
        e[-1] += 1
        v = host.psfm_host_rs_spans(len(a), a.ctypes.data, s.ctypes.data, e.ctypes.data, off.ctypes.data)
        assert (host.psfm_host_rs_verdict_index(v), host.psfm_host_rs_verdict_reason(v)) == (len(a) - 1, BAD_SPAN)


# ---- the footer ------------------------------------------------------------------------------------------------------------------

def small_set(n, seed=3):
    from point_trajectory.optimize.build import particlesfm
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 4, n)) - 1 if n else np.zeros(0, np.int64)
    birth, length = rng.integers(0, 20, n).astype(np.int32), rng.integers(1, 9, n).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(length, out=off[1:])
    return particlesfm.TrajectorySet._from_csr(ids, birth, length, off, rng.uniform(0, 99, (int(off[-1]), 2)))


@pytest.fixture(scope="module")
def real_file(tmp_path_factory):
    from point_trajectory.trajectory import save_track_npy
    path = str(tmp_path_factory.mktemp("track") / "track.npy")
    ts = small_set(37)
    save_track_npy(path, ts)
    return path, ts, open(path, "rb").read()


def parse(host, data, rec_size=REC):
    foot = np.frombuffer(data[-64:].rjust(64, b"\0"), np.uint8).copy()
    out = np.zeros(6, np.int64)
    return host.psfm_host_rs_footer(foot.ctypes.data, len(data), rec_size, out.ctypes.data), out


def with_footer(data, **change):
    from point_trajectory import reference_pickle as rp
    f = dict(zip(("m0", "xy_data", "n_points", "rec_start", "n", "R", "end", "m1"), rp._FOOTER.unpack(data[-64:])))
    f.update(change)
    return data[:-64] + rp._FOOTER.pack(*[f[k] for k in ("m0", "xy_data", "n_points", "rec_start", "n", "R", "end", "m1")])


def test_footer_of_a_real_file(host, real_file):
    from point_trajectory import reference_pickle as rp
    path, ts, data = real_file
    code, out = parse(host, data)
    assert code == FOOT_OK
    _, xy_data, n_points, rec_start, n, R, end, _ = rp._FOOTER.unpack(data[-64:])
    assert out.tolist() == [xy_data, n_points, rec_start, n, R, end] and n == 37 and R == REC and end == len(data) - 64
    assert np.array_equal(np.frombuffer(data[xy_data:xy_data + 16 * n_points], np.float64).reshape(-1, 2), ts._csr[4])


def test_every_field_pushed_out_of_bounds_by_one(host, real_file):
    from point_trajectory import reference_pickle as rp
    _, _, data = real_file
    _, xy_data, n_points, rec_start, n, R, end, _ = rp._FOOTER.unpack(data[-64:])
    room = (end - rec_start - 1) // R                      # the largest n with rec_start + n R < end
    assert parse(host, with_footer(data, n=room))[0] == FOOT_OK
    cases = [(dict(end=end + 1), FOOT_END), (dict(end=end - 1), FOOT_END), (dict(R=R + 1), FOOT_REC_SIZE), (dict(R=R - 1), FOOT_REC_SIZE),
             (dict(n=room + 1), FOOT_RECORDS), (dict(n=-1), FOOT_RECORDS), (dict(rec_start=end), FOOT_RECORDS), (dict(rec_start=-1), FOOT_RECORDS),
             (dict(rec_start=end - n * R), FOOT_RECORDS),  # rec_start + n R == end: the pickle's tail must follow the records
             (dict(xy_data=0), FOOT_POINTS), (dict(xy_data=rec_start), FOOT_POINTS), (dict(n_points=-1), FOOT_POINTS),
             (dict(n_points=(rec_start - xy_data) // 16 + 1), FOOT_POINTS)]
    for change, want in cases:
        assert parse(host, with_footer(data, **change))[0] == want, change
    assert parse(host, with_footer(data, n_points=(rec_start - xy_data) // 16))[0] == FOOT_OK
    assert parse(host, data, rec_size=REC + 1)[0] == FOOT_REC_SIZE and parse(host, data, rec_size=0)[0] == FOOT_REC_SIZE


def test_either_magic_wrong(host, real_file):
    _, _, data = real_file
    assert parse(host, with_footer(data, m0=b"PSFMTRK2"))[0] == FOOT_MAGIC
    assert parse(host, with_footer(data, m1=b"psfmtrk1"))[0] == FOOT_MAGIC


def test_every_truncation_is_refused(host, real_file):
    from point_trajectory import reference_pickle as rp
    _, _, data = real_file
    _, xy_data, n_points, rec_start, n, R, end, _ = rp._FOOTER.unpack(data[-64:])
    cuts = list(range(len(data) - 64, len(data))) + [rec_start + 5 * R + 7, xy_data + 16 * 3 + 5, 64, 63, 10, 0]
    for cut in cuts:
        code, _ = parse(host, data[:cut])
        assert code != FOOT_OK, cut
        assert (code == FOOT_SHORT) == (cut <= 64), cut


def test_overflow_guards(host, real_file):
    _, _, data = real_file
    big = (1 << 62) + 12345
    for change in (dict(n=big), dict(n=(1 << 63) - 1), dict(n_points=big), dict(n_points=(1 << 63) - 1), dict(n=big, n_points=big),
                   dict(rec_start=(1 << 63) - 1), dict(xy_data=(1 << 63) - 1), dict(n=(1 << 63) // REC), dict(n_points=1 << 60)):
        assert parse(host, with_footer(data, **change))[0] in (FOOT_RECORDS, FOOT_POINTS), change


def test_an_empty_set_has_a_footer_without_points(host, tmp_path):
    from point_trajectory.trajectory import save_track_npy
    path = str(tmp_path / "empty.npy")
    save_track_npy(path, small_set(0))
    code, out = parse(host, open(path, "rb").read())
    assert code == FOOT_OK and out[1] == 0 and out[3] == 0


# ---- the records -----------------------------------------------------------------------------------------------------------------

def records(n, seed=9):
    """n records as the writer fills them (reference_pickle.dump), their fields, the template and the offsets."""
    from point_trajectory import reference_pickle as rp
    rec, at = rp._record_template()
    rng = np.random.default_rng(seed)
    length = rng.integers(1, 40, n)
    birth = rng.integers(0, 500, n)
    f = {"id": np.cumsum(rng.integers(1, 5, n)) - 1, "b": birth, "bn": birth + length, "s": np.cumsum(length) - length, "e": np.cumsum(length),
         "n": length}
    buf = np.tile(np.frombuffer(rec, np.uint8), n).reshape(n, len(rec))
    for name, v in f.items():
        buf[:, at[name]:at[name] + 4] = v.astype("<i4").view(np.uint8).reshape(-1, 4)
    return buf, f, np.frombuffer(rec, np.uint8).copy(), np.asarray([at[k] for k in FIELDS], np.int32)


def decode(host, buf, tmpl, field_at, rec0=0):
    n = len(buf)
    ws = np.full(rec0 + buf.size + 16 + (-(rec0 + buf.size)) % 16, 0x5A, np.uint8)
    ws[rec0:rec0 + buf.size] = buf.reshape(-1)
    out = [np.full(n, -9, np.int32) for _ in range(5)]
    fault = ctypes.c_int(0)
    v = host.psfm_host_rs_decode(ws.ctypes.data, len(ws), rec0, n, tmpl.ctypes.data, len(tmpl), field_at.ctypes.data, *[a.ctypes.data for a in out],
                                 ctypes.byref(fault))
    assert fault.value == 0
    return (None if v == NONE else (host.psfm_host_rs_verdict_index(v), host.psfm_host_rs_verdict_reason(v))), out


def fields_np(buf, at_list):
    """reference_pickle.load's field extraction."""
    return [np.ascontiguousarray(buf[:, a:a + 4]).view("<i4").reshape(-1) for a in at_list]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 1025])
@pytest.mark.parametrize("rec0", [0, 6])
def test_decode_against_the_writers_field_extraction(host, n, rec0):
    buf, f, tmpl, field_at = records(n)
    assert len(tmpl) == REC and host.psfm_host_rs_template_ok(tmpl.ctypes.data, REC, field_at.ctypes.data) == 1
    verdict, (ids, birth, length, s, e) = decode(host, buf, tmpl, field_at, rec0)
    assert verdict is None
    want = dict(zip(FIELDS, fields_np(buf, field_at.tolist())))
    for got, name in ((ids, "id"), (birth, "b"), (length, "n"), (s, "s"), (e, "e")):
        assert np.array_equal(got, want[name]) and np.array_equal(got, f[name].astype(np.int32)), name


@pytest.mark.parametrize("n", [257, 1025])
def test_a_flipped_template_byte_names_its_record(host, n):
    buf, f, tmpl, field_at = records(n)
    field_bytes = {a + j for a in field_at.tolist() for j in range(4)}
    plain = [j for j in range(REC) if j not in field_bytes]
    for r in (0, 255, 256, n - 1):
        for j in (plain[0], plain[len(plain) // 2], plain[-1]):
            bad = buf.copy()
            bad[r, j] ^= 0x10
            assert decode(host, bad, tmpl, field_at)[0] == (r, BAD_TEMPLATE), (r, j)
    bad = buf.copy()
    bad[256, plain[3]] ^= 1
    bad[255, plain[5]] ^= 1
    assert decode(host, bad, tmpl, field_at)[0] == (255, BAD_TEMPLATE)         # the lower record wins
    # every byte of a record is either a field byte or compared
    for j in range(REC):
        bad = buf.copy()
        bad[n - 1, j] ^= 0x80
        got = decode(host, bad, tmpl, field_at)[0]
        if j in plain:
            assert got == (n - 1, BAD_TEMPLATE), j
        else:
            assert got is None or got == (n - 1, BAD_BN), j                    # (a field changed: at most the b + n rule sees it here)


def test_fields_that_disagree(host):
    buf, f, tmpl, field_at = records(600)
    at = dict(zip(FIELDS, field_at.tolist()))
    bad = buf.copy()
    bad[300, at["bn"]:at["bn"] + 4] = np.asarray([int(f["bn"][300]) + 1], "<i4").view(np.uint8)
    verdict, _ = decode(host, bad, tmpl, field_at)
    assert verdict == (300, BAD_BN)
    # s / e: the decode passes them on; the pass behind the scan objects
    for name, delta in (("s", 1), ("e", -1)):
        bad = buf.copy()
        bad[411, at[name]:at[name] + 4] = np.asarray([int(f[name][411]) + delta], "<i4").view(np.uint8)
        verdict, (ids, birth, length, s, e) = decode(host, bad, tmpl, field_at)
        assert verdict is None and run_validate(host, ids, birth, length) is None
        _, _, off = expand_np(ids, birth, length)
        v = host.psfm_host_rs_spans(len(ids), ids.ctypes.data, s.ctypes.data, e.ctypes.data, off.ctypes.data)
        assert (host.psfm_host_rs_verdict_index(v), host.psfm_host_rs_verdict_reason(v)) == (411, BAD_SPAN)


def test_template_offsets_are_checked(host):
    _, _, tmpl, field_at = records(1)
    for k, v in ((0, -1), (5, REC - 3), (1, int(field_at[0]) + 2)):             # outside the record; overlapping another field
        bad = field_at.copy()
        bad[k] = v
        assert host.psfm_host_rs_template_ok(tmpl.ctypes.data, REC, bad.ctypes.data) == 0
    assert host.psfm_host_rs_template_ok(tmpl.ctypes.data, int(field_at.max()) + 3, field_at.ctypes.data) == 0     # (the last field ends outside)
    assert host.psfm_host_rs_template_ok(tmpl.ctypes.data, 69, field_at.ctypes.data) == 0


def test_the_real_files_records_decode_to_its_set(host, real_file):
    from point_trajectory import reference_pickle as rp
    _, ts, data = real_file
    _, xy_data, n_points, rec_start, n, R, end, _ = rp._FOOTER.unpack(data[-64:])
    rec, at = rp._record_template()
    buf = np.frombuffer(data[rec_start:rec_start + n * R], np.uint8).reshape(n, R)
    verdict, (ids, birth, length, s, e) = decode(host, buf, np.frombuffer(rec, np.uint8).copy(), np.asarray([at[k] for k in FIELDS], np.int32))
    assert verdict is None and run_validate(host, ids, birth, length) is None
    cids, cbirth, clen, coff, _, _ = ts._csr
    assert np.array_equal(ids, cids) and np.array_equal(birth, cbirth) and np.array_equal(length, clen)
    assert np.array_equal(s, coff[:-1]) and np.array_equal(e, coff[1:])
