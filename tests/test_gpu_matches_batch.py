"""psfm_result_filter_batch / psfm_traj_to_matches_batch / psfm_labels_to_matches_batch (csrc/psfm_matches_batch.hip) on the device:
every context of a batch holds, byte for byte, what the single calls leave in it -- compared through psfm_matches_copy /
psfm_result_filtered_copy with the single calls on the device and with the NumPy model match_tables_host (pinned to the reference by
tests/test_consumers_golden.py).  The sets are those of tests/_matches_batch_np.py (tests/test_matches_batch_host.py says what each
one is for); labelled sets enter the contexts through psfm_labels_set, the saved sets come from psfm_connect_batch on three small
synthetic sequences.  Refusals are argument checks: nothing here faults."""
import ctypes

import numpy as np
import pytest

import _matches_batch_np as mb
from test_gpu_database import labels_set, vp

pytestmark = pytest.mark.gpu
NAMES = ("kp_off", "kp_xy", "pair_key", "pair_off", "pair_first", "rows")


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import utils, trajectory, _hip
    from psfm_sfm import matches_from_flow as mff
    _hip.context()
    class NS: pass
    ns = NS()
    ns.utils, ns.trajectory, ns.hip, ns.mff, ns.torch = utils, trajectory, _hip, mff, torch
    return ns


def assert_tables_bit_equal(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, name)


def handles(ctxs):
    return (ctypes.c_void_p * len(ctxs))(*[None if c is None else c.handle.value for c in ctxs])


def labels_batch(pt, ctxs, n_imgs, remove_dynamic=True, n_seq=None):
    """psfm_labels_to_matches_batch only: [(n_kp, n_m, n_pairs)], the tables stay in the contexts."""
    n = len(ctxs)
    kp, m, p = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()
    n_img = (ctypes.c_int32 * max(n, 1))(*[int(v) for v in n_imgs])
    live = [c for c in ctxs if c is not None]
    pt.hip.check(pt.hip.lib().psfm_labels_to_matches_batch(handles(ctxs), n if n_seq is None else n_seq, n_img, pt.mff.SAMPLE_K,
                                                           1 if remove_dynamic else 0, kp, m, p, pt.hip.current_stream_ptr(live[0].device)))
    return [(int(kp[i]), int(m[i]), int(p[i])) for i in range(n)]


def traj_batch(pt, ctxs, n_imgs, labels=None):
    n = len(ctxs)
    kp, m, p = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    n_img = (ctypes.c_int32 * n)(*[int(v) for v in n_imgs])
    lab = None if labels is None else (ctypes.c_void_p * n)(*[pt.hip.ptr(t).value for t in labels])
    pt.hip.check(pt.hip.lib().psfm_traj_to_matches_batch(handles(ctxs), n, n_img, pt.mff.SAMPLE_K, lab, kp, m, p,
                                                         pt.hip.current_stream_ptr(ctxs[0].device)))
    return [(int(kp[i]), int(m[i]), int(p[i])) for i in range(n)]


def traj_single(pt, ctx, n_img, labels=None):
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(pt.hip.lib().psfm_traj_to_matches(ctx.handle, int(n_img), pt.mff.SAMPLE_K, pt.hip.ptr(labels), ctypes.byref(a), ctypes.byref(b),
                                                   ctypes.byref(c), pt.hip.current_stream_ptr(ctx.device)))
    return int(a.value), int(b.value), int(c.value)


def copy_tables(pt, ctx, n_img, sizes):
    return pt.mff._copy_tables(ctx, int(n_img), *sizes)


def copy_expecting_empty(pt, ctx, n_img, room):
    """psfm_matches_copy into buffers with room for an earlier call's tables, filled with a sentinel: empty tables write none of it
    but the zero-filled kp_off and pair_off[0]."""
    n_kp, n_m, n_p = room
    kp_off = np.full(n_img + 1, -7, np.int64)
    kp_xy = np.full((max(n_kp, 1), 2), -7.0)
    pair_key, pair_off, pair_first = np.full(max(n_p, 1), -7, np.int64), np.full(max(n_p, 1) + 1, -7, np.int64), np.full(max(n_p, 1), -7, np.int64)
    rows = np.full((max(n_m, 1), 2), -7, np.int32)
    pt.hip.check(pt.hip.lib().psfm_matches_copy(ctx.handle, vp(kp_off), vp(kp_xy), vp(pair_key), vp(pair_off), vp(pair_first), vp(rows),
                                                pt.hip.current_stream_ptr(ctx.device)))
    assert not kp_off.any() and pair_off[0] == 0
    assert (kp_xy == -7).all() and (pair_key == -7).all() and (pair_off[1:] == -7).all() and (pair_first == -7).all() and (rows == -7).all()


def model(pt, seq, remove_dynamic=True):
    off, frames, xy, labels, n_img = seq
    return pt.mff.match_tables_host(off, frames, xy, labels, n_img, remove_dynamic)


def load_sets(pt, ctxs, seqs):
    for c, (off, frames, xy, labels, _) in zip(ctxs, seqs):
        labels_set(pt, c, off, frames, xy, labels)


@pytest.fixture(scope="module")
def models():
    """the NumPy model of every set the labelled tests use, computed once"""
    from psfm_sfm import matches_from_flow as mff
    cache = {}

    def get(seq, remove_dynamic=True):
        key = (id(seq[1]), seq[4], remove_dynamic)
        if key not in cache:
            cache[key] = (seq, mff.match_tables_host(seq[0], seq[1], seq[2], seq[3], seq[4], remove_dynamic))
        return cache[key][1]
    return get


# ---- 1. labelled route, the hand-shaped batch -----------------------------------------------------------------------------------------

ORDERS = mb.orders()


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("remove_dynamic", [True, False])
def test_labelled_route_small_batch(pt, models, order, remove_dynamic):
    seqs = ORDERS[order]
    ctxs = pt.hip.batch_contexts(9)
    load_sets(pt, ctxs[:8], seqs)
    sizes = labels_batch(pt, ctxs[:8], [s[4] for s in seqs], remove_dynamic)
    got = [copy_tables(pt, ctxs[b], seqs[b][4], sizes[b]) for b in range(8)]
    ninth = ctxs[8]
    for b, seq in enumerate(seqs):                      # no sequence skipped
        assert_tables_bit_equal(got[b], models(seq, remove_dynamic), "model, sequence %d" % b)
        labels_set(pt, ninth, *seq[:4])
        assert_tables_bit_equal(got[b], pt.mff.match_tables_labelled_device(ninth, seq[4], remove_dynamic), "single call, sequence %d" % b)
    first, again = [b for b, s in enumerate(seqs) if s[4] == 45]
    assert_tables_bit_equal(got[first], got[again])
    assert sizes[first][1] > 1000 and sum(1 for s in sizes if s[1] == 0) == (3 if remove_dynamic else 2)
    # two identical calls give identical bytes
    assert labels_batch(pt, ctxs[:8], [s[4] for s in seqs], remove_dynamic) == sizes
    for b in range(8):
        assert_tables_bit_equal(copy_tables(pt, ctxs[b], seqs[b][4], sizes[b]), got[b], "second call, sequence %d" % b)


# ---- 2. batch sizes and refusals ----------------------------------------------------------------------------------------------------

def test_one_sequence_equals_the_single_call(pt, models):
    seq = mb.hand_shaped_batch()[0]
    ctx = pt.hip.batch_contexts(1)[0]
    labels_set(pt, ctx, *seq[:4])
    sizes = labels_batch(pt, [ctx], [seq[4]])
    got = copy_tables(pt, ctx, seq[4], sizes[0])
    assert_tables_bit_equal(got, pt.mff.match_tables_labelled_device(ctx, seq[4]))
    assert_tables_bit_equal(got, models(seq))


def test_sixty_four_sequences(pt):
    seqs = mb.random_sets(64, 5)
    ctxs = pt.hip.batch_contexts(64)
    load_sets(pt, ctxs, seqs)
    sizes = labels_batch(pt, ctxs, [s[4] for s in seqs])
    n_pts = [len(s[1]) for s in seqs]
    assert min(n_pts) < 20 and max(n_pts) > 250 and len(set(n_pts)) > 40
    for b, seq in enumerate(seqs):                      # every sequence is compared
        assert_tables_bit_equal(copy_tables(pt, ctxs[b], seq[4], sizes[b]), model(pt, seq), "sequence %d" % b)


def test_refused_calls_leave_earlier_tables(pt, models):
    seqs = mb.hand_shaped_batch()
    a, b = seqs[0], seqs[4]
    ctxs = pt.hip.batch_contexts(66)
    load_sets(pt, ctxs[:2], [a, b])
    sizes = labels_batch(pt, ctxs[:2], [a[4], b[4]])
    before = [copy_tables(pt, ctxs[0], a[4], sizes[0]), copy_tables(pt, ctxs[1], b[4], sizes[1])]

    def still_there():
        assert_tables_bit_equal(copy_tables(pt, ctxs[0], a[4], sizes[0]), before[0])
        assert_tables_bit_equal(copy_tables(pt, ctxs[1], b[4], sizes[1]), before[1])
        assert_tables_bit_equal(before[0], models(a))

    for what, args, kw in (("n_seq=0", (ctxs[:2], [a[4], b[4]]), {"n_seq": 0}),
                           ("n_seq=65", (ctxs[:65], [a[4]] * 65), {}),
                           ("given twice", ([ctxs[0], ctxs[1], ctxs[0]], [a[4], b[4], a[4]]), {}),
                           ("NULL", ([ctxs[0], None, ctxs[1]], [a[4], 3, b[4]]), {}),
                           ("n_img=0", (ctxs[:2], [a[4], 0]), {})):
        with pytest.raises(pt.hip.PsfmError) as e:
            labels_batch(pt, *args, **kw)
        assert e.value.status == pt.hip.PSFM_ERR_ARG, what
        print(what, "->", e.value)
        still_there()
    with pytest.raises(pt.hip.PsfmError, match="context 2"):
        labels_batch(pt, [ctxs[0], ctxs[1], ctxs[0]], [a[4], b[4], a[4]])
    with pytest.raises(pt.hip.PsfmError, match="context 1"):
        labels_batch(pt, [ctxs[0], None], [a[4], 3])
    with pytest.raises(pt.hip.PsfmError, match="sequence 1"):
        labels_batch(pt, ctxs[:2], [a[4], 0])
    # the filter and the saved-set route check the same way
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctxs[0].device)
    k2, n2 = (ctypes.c_int64 * 66)(), (ctypes.c_int64 * 66)()
    for hs, n in ((handles(ctxs[:2]), 0), (handles(ctxs[:65]), 65), (handles([ctxs[0], ctxs[0]]), 2), (handles([ctxs[0], None]), 2)):
        assert L.psfm_result_filter_batch(hs, n, 3, k2, n2, sp) == pt.hip.PSFM_ERR_ARG
        nimg = (ctypes.c_int32 * 66)(*([5] * 66))
        assert L.psfm_traj_to_matches_batch(hs, n, nimg, 20, None, k2, n2, k2, sp) == pt.hip.PSFM_ERR_ARG
    nimg = (ctypes.c_int32 * 2)(a[4], b[4])
    assert L.psfm_labels_to_matches_batch(handles(ctxs[:2]), 2, nimg, 0, 1, k2, n2, k2, sp) == pt.hip.PSFM_ERR_ARG      # sample_k < 1
    still_there()


# ---- 3. the saved-set route -----------------------------------------------------------------------------------------------------------

N_FLOWS = (5, 9, 12)


@pytest.fixture(scope="module")
def connected(pt):
    """three synthetic sequences of 48 x 64 with 5, 9 and 12 flows at sample_ratio 2, connected as one batch; the results stay in the
    contexts for the tests of this module"""
    import psfm_synth
    seqs = []
    for i, n in enumerate(N_FLOWS):
        d = psfm_synth.synth_sequence(n + 1, 48, 64, seed=30 + i, stride2=False)
        seqs.append((pt.torch.from_numpy(np.stack(d["flows_f"])).cuda(), pt.torch.from_numpy(np.stack(d["flows_b"])).cuda(), None, None))
    ctxs, infos = pt.trajectory.run_connect_batch(seqs, 1.0, 2)
    assert all(int(i.n_traj) > 100 for i in infos)
    return list(ctxs)


def filter_batch(pt, ctxs, traj_min_len):
    n = len(ctxs)
    k, npt = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    pt.hip.check(pt.hip.lib().psfm_result_filter_batch(handles(ctxs), n, traj_min_len, k, npt, pt.hip.current_stream_ptr(ctxs[0].device)))
    return [(int(k[i]), int(npt[i])) for i in range(n)]


def filter_single(pt, ctx, traj_min_len):
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(pt.hip.lib().psfm_result_filter(ctx.handle, traj_min_len, ctypes.byref(k), ctypes.byref(n), pt.hip.current_stream_ptr(ctx.device)))
    return int(k.value), int(n.value)


def filtered_copy(pt, ctx, k, n):
    ids, birth, length = np.full(k, -7, np.int32), np.full(k, -7, np.int32), np.full(k, -7, np.int32)
    off, xy = np.full(k + 1, -7, np.int64), np.full((n, 2), -7.0)
    pt.hip.check(pt.hip.lib().psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), pt.hip.current_stream_ptr(ctx.device)))
    return ids, birth, length, off, xy


def test_filter_batch_equals_the_single_filter(pt, connected):
    got_sizes = filter_batch(pt, connected, 3)
    got = [filtered_copy(pt, c, *s) for c, s in zip(connected, got_sizes)]
    for b, c in enumerate(connected):
        assert filter_single(pt, c, 3) == got_sizes[b] and got_sizes[b][0] > 50
        want = filtered_copy(pt, c, *got_sizes[b])
        for name, g, w in zip(("ids", "birth", "len", "off", "xy"), got[b], want):
            assert g.tobytes() == w.tobytes(), (b, name)
        assert (np.diff(got[b][0]) > 0).all() and got[b][2].min() >= 3 and got[b][3][-1] == got_sizes[b][1] == got[b][2].sum()
    # above every length: all counts 0, the tables empty
    room = traj_batch(pt, connected, [n + 1 for n in N_FLOWS])
    assert all(r[1] > 0 for r in room)
    assert filter_batch(pt, connected, 1000) == [(0, 0)] * 3
    assert traj_batch(pt, connected, [n + 1 for n in N_FLOWS]) == [(0, 0, 0)] * 3
    for b, c in enumerate(connected):
        copy_expecting_empty(pt, c, N_FLOWS[b] + 1, room[b])
    assert filter_batch(pt, connected, 3) == got_sizes


@pytest.mark.parametrize("labelling", ["none", "all", "one_null"])
def test_saved_set_route(pt, connected, labelling):
    sizes_f = filter_batch(pt, connected, 3)
    sets = [filtered_copy(pt, c, *s) for c, s in zip(connected, sizes_f)]
    n_imgs = [N_FLOWS[0] + 1, N_FLOWS[1] + 1 + 6, N_FLOWS[2] + 1]          # one larger than the frames present
    rng = np.random.default_rng(8)
    lab_np = [(rng.random(s[1]) < 0.3).astype(np.uint8) for s in sizes_f]
    if labelling == "none":
        lab_np = [None] * 3
    if labelling == "one_null":
        lab_np[1] = None
    lab = [None if a is None else pt.torch.from_numpy(a).cuda() for a in lab_np]
    sizes = traj_batch(pt, connected, n_imgs, None if labelling == "none" else lab)
    got = [copy_tables(pt, c, n_imgs[b], sizes[b]) for b, c in enumerate(connected)]
    for b, c in enumerate(connected):
        assert traj_single(pt, c, n_imgs[b], lab[b]) == sizes[b] and sizes[b][2] > 0
        assert_tables_bit_equal(got[b], copy_tables(pt, c, n_imgs[b], sizes[b]), "single call, sequence %d" % b)
        ids, birth, length, off, xy = sets[b]
        n = sizes_f[b][1]
        frames = (np.repeat(birth, length) + np.arange(n) - np.repeat(off[:-1], length)).astype(np.int64)
        labels = np.zeros(n, bool) if lab_np[b] is None else lab_np[b].astype(bool)
        assert_tables_bit_equal(got[b], pt.mff.match_tables_host(off, frames, xy, labels, n_imgs[b]), "model, sequence %d" % b)
        assert len(got[b][0]) == n_imgs[b] + 1


# ---- 4. errors found on the device, and a missing labelled set ---------------------------------------------------------------------

def test_frame_outside_the_image_list(pt, models):
    seqs = mb.hand_shaped_batch()
    use = [seqs[0], seqs[4], seqs[6]]
    ctxs = pt.hip.batch_contexts(3)
    load_sets(pt, ctxs, use)
    n_imgs = [s[4] for s in use]
    good = labels_batch(pt, ctxs, n_imgs)
    short = list(n_imgs)
    short[1] = int(use[1][1].max())                       # smaller than its last frame + 1
    with pytest.raises(pt.hip.PsfmError, match="sequence 1") as e:
        labels_batch(pt, ctxs, short)
    assert e.value.status == pt.hip.PSFM_ERR_ARG
    for b, c in enumerate(ctxs):                          # every context of the call copies out empty tables
        copy_expecting_empty(pt, c, short[b], good[b])
    # two sequences with such a frame: the lowest is named
    short[2] = 3
    with pytest.raises(pt.hip.PsfmError, match="sequence 1"):
        labels_batch(pt, ctxs, short)
    assert labels_batch(pt, ctxs, n_imgs) == good         # the corrected call
    for b, c in enumerate(ctxs):
        assert_tables_bit_equal(copy_tables(pt, c, n_imgs[b], good[b]), models(use[b]), "sequence %d" % b)
    # a context whose labelled set was never finished: refused by index, the others keep their tables
    fresh = pt.hip.Context(ctxs[0].device)
    try:
        with pytest.raises(pt.hip.PsfmError, match="sequence 2") as e:
            labels_batch(pt, [ctxs[0], ctxs[1], fresh], n_imgs)
        assert e.value.status == pt.hip.PSFM_ERR_ARG
    finally:
        fresh.close()
    for b, c in enumerate(ctxs):
        assert_tables_bit_equal(copy_tables(pt, c, n_imgs[b], good[b]), models(use[b]), "sequence %d" % b)


# ---- 5. downstream ------------------------------------------------------------------------------------------------------------------

def test_database_rows_after_the_batch_call(pt):
    from _database_np import assert_tables_bit_equal as assert_db_equal
    from psfm_sfm.database import database_tables_device
    seqs = mb.hand_shaped_batch()[:5]
    ctxs = pt.hip.batch_contexts(5)
    load_sets(pt, ctxs, seqs)
    labels_batch(pt, ctxs, [s[4] for s in seqs])
    n_img = seqs[0][4]
    rng = np.random.default_rng(9)
    db_id, db_pos = (rng.permutation(n_img) + 5).astype(np.int32), rng.permutation(n_img).astype(np.int32)
    got = database_tables_device(ctxs[0], n_img, db_id, db_pos)
    pt.mff.match_tables_labelled_device(ctxs[0], n_img)
    want = database_tables_device(ctxs[0], n_img, db_id, db_pos)
    assert_db_equal(got, want)
    assert len(got.rows) > 100


# ---- 6. the budget ------------------------------------------------------------------------------------------------------------------

def census(pt, ctx):
    a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
    pt.hip.check(pt.hip.lib().psfm_matches_batch_census(ctx.handle, ctypes.byref(a), ctypes.byref(b)))
    return int(a.value), int(b.value)


def test_synchronisations_and_launches_do_not_depend_on_n_seq(pt, connected):
    seqs = [s for s in mb.random_sets(80, 6) if len(s[1]) > 40][:64]
    assert len(seqs) == 64
    ctxs = pt.hip.batch_contexts(64)
    load_sets(pt, ctxs, seqs)
    assert all(s[1] > 0 for s in labels_batch(pt, ctxs[:2], [s[4] for s in seqs[:2]]))
    two = census(pt, ctxs[0])
    assert all(s[1] > 0 for s in labels_batch(pt, ctxs, [s[4] for s in seqs]))
    all64 = census(pt, ctxs[0])
    print("tables: (synchronisations, launches) with 2 sequences", two, "with 64", all64)
    assert two == all64 and 1 <= two[0] <= 4 and two[1] > 0
    # the filter: at most two, whatever the number of sequences
    filter_batch(pt, connected[:2], 3)
    f2 = census(pt, connected[0])
    filter_batch(pt, connected, 3)
    f3 = census(pt, connected[0])
    print("filter: (synchronisations, launches) with 2 sequences", f2, "with 3", f3)
    assert f2 == f3 and 1 <= f2[0] <= 2 and f2[1] > 0
    traj_batch(pt, connected[:2], [n + 1 for n in N_FLOWS[:2]])
    t2 = census(pt, connected[0])
    traj_batch(pt, connected, [n + 1 for n in N_FLOWS])
    assert census(pt, connected[0]) == t2 == two


# ---- 7. the Python mirror -----------------------------------------------------------------------------------------------------------

def test_grouped_python_functions(pt, connected, tmp_path):
    s = mb.hand_shaped_batch()
    seqs = [s[0], s[4], s[5], s[6], s[2]]
    n_pts = [len(x[1]) for x in seqs]
    assert [g[:2] for g in pt.mff.group_sequences(n_pts, 400)] == [(0, 2), (2, 3), (3, 5)]          # three groups
    ctxs = pt.hip.batch_contexts(6)
    load_sets(pt, ctxs[:5], seqs)
    n_imgs = [x[4] for x in seqs]
    for cap in (400, 200):                                                                          # 200: three sequences go alone
        got = pt.mff.match_tables_labelled_batch_device(ctxs[:5], n_imgs, max_points=cap)
        assert len(got) == 5
        for b, seq in enumerate(seqs):
            labels_set(pt, ctxs[5], *seq[:4])
            assert_tables_bit_equal(got[b], pt.mff.match_tables_labelled_device(ctxs[5], seq[4]), "cap %d, sequence %d" % (cap, b))
    assert sum(1 for g in pt.mff.group_sequences(n_pts, 200) if g[2]) == 3
    # the saved-set route, one sequence per group, and the assembled form
    n_imgs = [n + 1 for n in N_FLOWS]
    got = pt.mff.match_tables_batch_device(connected, n_imgs, max_points=1)
    whole = pt.mff.match_tables_batch_device(connected, n_imgs)
    for b, c in enumerate(connected):
        want = pt.mff.match_tables_device(c, n_imgs[b])
        assert_tables_bit_equal(got[b], want, "alone, sequence %d" % b)
        assert_tables_bit_equal(whole[b], want, "one group, sequence %d" % b)
    names = [["%03d.png" % i for i in range(n)] for n in n_imgs]
    files = [str(tmp_path / ("pairs%d.txt" % b)) for b in range(3)]
    out = pt.mff.traj_to_matches_batch_device(connected, names, files)
    for b, c in enumerate(connected):
        one = pt.mff.traj_to_matches_device(c, names[b], str(tmp_path / "one.txt"))
        assert list(out[b]) == list(one) and open(files[b]).read() == open(str(tmp_path / "one.txt")).read()
        for name in names[b]:
            assert np.array_equal(out[b][name].keypoints, one[name].keypoints) and list(out[b][name].match_pairs) == list(one[name].match_pairs)
            assert all(np.array_equal(out[b][name].match_pairs[k], one[name].match_pairs[k]) for k in one[name].match_pairs)


# ---- 8. the single entry points at their edges (psfm_labels_to_matches through ctypes, bit-compared with the model) -------------------
# tests/test_matches_batch_host.py::test_the_edge_sets_are_what_they_say holds every property claimed of these sets

def labels_single(pt, ctx, n_img, remove_dynamic=True):
    a, b, c = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    pt.hip.check(pt.hip.lib().psfm_labels_to_matches(ctx.handle, int(n_img), pt.mff.SAMPLE_K, 1 if remove_dynamic else 0, ctypes.byref(a),
                                                     ctypes.byref(b), ctypes.byref(c), pt.hip.current_stream_ptr(ctx.device)))
    return int(a.value), int(b.value), int(c.value)


def single_equals_model(pt, ctx, models, seq, remove_dynamic=True, what=""):
    want = models(seq, remove_dynamic)
    sizes = labels_single(pt, ctx, seq[4], remove_dynamic)
    assert sizes == (len(want[1]), len(want[5]), len(want[2])), what
    assert_tables_bit_equal(copy_tables(pt, ctx, seq[4], sizes), want, what)
    return sizes


@pytest.mark.parametrize("remove_dynamic", [True, False])
@pytest.mark.parametrize("n_points", mb.EDGE_POINTS)
def test_single_call_at_the_edges_of_a_block(pt, models, n_points, remove_dynamic):
    """1, 255, 256, 257 and 513 points in trajectories of 1, 2, 20, 21, 40 and 41 points, frames not ascending and with gaps"""
    seq = mb.EDGE_SETS[n_points]
    ctx = pt.hip.batch_contexts(1)[0]
    labels_set(pt, ctx, *seq[:4])
    sizes = single_equals_model(pt, ctx, models, seq, remove_dynamic)
    assert (sizes[1] > 0) == (n_points > 1) and len(seq[1]) == n_points


def test_single_call_with_every_point_dynamic(pt, models):
    seq = mb.ALL_DYNAMIC_SET
    ctx = pt.hip.batch_contexts(1)[0]
    labels_set(pt, ctx, *seq[:4])
    room = single_equals_model(pt, ctx, models, seq, False)             # every point kept
    assert room[0] == 257 and room[1] > 1000
    assert labels_single(pt, ctx, seq[4], True) == (0, 0, 0)            # every point dropped: the earlier tables are gone
    copy_expecting_empty(pt, ctx, seq[4], room)
    assert_tables_bit_equal(copy_tables(pt, ctx, seq[4], (0, 0, 0)), models(seq, True))


@pytest.mark.parametrize("n_img", mb.EDGE_N_IMG)
def test_single_call_at_the_edges_of_the_key_widths(pt, models, n_img):
    """n_img 1, 2, 255, 256, 257: the frame key grows from 8 to 9 bits, the pair key from 16 to 17; a point in the last image"""
    seq = mb.N_IMG_SETS[n_img]
    ctx = pt.hip.batch_contexts(1)[0]
    labels_set(pt, ctx, *seq[:4])
    sizes = single_equals_model(pt, ctx, models, seq)
    assert (sizes[1] > 0) == (n_img > 1) and int(seq[1].max()) == n_img - 1
    # the same set as a batch of one and as the second sequence of a batch of two: the composed key with 0 and with 1 sequence bit
    ctxs = pt.hip.batch_contexts(2)
    assert labels_batch(pt, ctxs[:1], [n_img]) == [sizes]
    assert_tables_bit_equal(copy_tables(pt, ctxs[0], n_img, sizes), models(seq), "batch of one")
    first = mb.N_IMG_SETS[2]
    load_sets(pt, ctxs, [first, seq])
    both = labels_batch(pt, ctxs, [2, n_img])
    assert both[1] == sizes
    assert_tables_bit_equal(copy_tables(pt, ctxs[1], n_img, sizes), models(seq), "second of two")
    assert_tables_bit_equal(copy_tables(pt, ctxs[0], 2, both[0]), models(first), "first of two")


def test_single_calls_and_batch_calls_in_any_order_on_the_same_contexts(pt, models):
    """a single call on the context that owned a batch call's intermediates, one on a context that did not, and a batch call behind
    them with the contexts the other way round"""
    seqs = mb.hand_shaped_batch()
    a, b = seqs[0], seqs[6]
    ctxs = pt.hip.batch_contexts(2)
    load_sets(pt, ctxs, [a, b])
    sizes = labels_batch(pt, ctxs, [a[4], b[4]])
    assert single_equals_model(pt, ctxs[0], models, a, what="ctxs[0] after the batch call") == sizes[0]
    assert single_equals_model(pt, ctxs[1], models, b, what="ctxs[1] after the batch call") == sizes[1]
    for c, s, n in ((ctxs[0], a, sizes[0]), (ctxs[1], b, sizes[1])):     # neither call touched the other context
        assert_tables_bit_equal(copy_tables(pt, c, s[4], n), models(s))
    load_sets(pt, ctxs, [b, a])                                          # the larger set moves to the other context
    assert labels_batch(pt, [ctxs[1], ctxs[0]], [a[4], b[4]]) == sizes
    assert_tables_bit_equal(copy_tables(pt, ctxs[1], a[4], sizes[0]), models(a), "ctxs[1] as the owner")
    assert_tables_bit_equal(copy_tables(pt, ctxs[0], b[4], sizes[1]), models(b), "ctxs[0] as the second")
    assert single_equals_model(pt, ctxs[0], models, b, what="ctxs[0] after the second batch call") == sizes[1]
    assert sizes[0][1] > 1000 and sizes[1][1] > 0
