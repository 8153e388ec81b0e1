"""The batch plan of psfm_traj_decode_batch without a GPU: particle-sfm_amd/csrc/psfm_decoder_batch.h -- the table of windows, the
flattened tile and slice maps, the per-window workspace offsets, the lookup a block performs and the plan by section names --
compiled for the host by tests/host/decoder_batch_host.cpp and compared with a brute-force enumeration written here.  The last test
walks the whole batch on the host (decoder_host.cpp's arithmetic, the batch's addresses) and asks for the bits of the single call."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from _decoder_np import seeded_decoder_inputs, seeded_decoder_weights
from psfm_motion_seg.decoder import pack_decoder_weights_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 2, 63, 64, 65, 511, 512, 513, 735]
TILE, SLICE, MAX = 64, 512, 64
INT32_MAX = 2 ** 31 - 1


def k_lists():
    """Lists of lengths 1, 2, 5 and 64 over SIZES, in several orders."""
    rng = np.random.default_rng(11)
    out = [[k] for k in SIZES]
    out += [list(p) for p in itertools.product([0, 2, 65, 513], repeat=2)] + [[735, 64], [64, 735], [512, 511], [0, 735]]
    five = [[65, 2, 0, 513, 64], [0, 0, 2, 0, 0], [735, 513, 512, 511, 65], [2, 63, 64, 65, 511], [0, 512, 0, 512, 0], [64, 64, 64, 64, 64]]
    out += five + [l[::-1] for l in five]
    out += [[int(k) for k in rng.permutation(SIZES)[:5]] for _ in range(4)]
    full = [SIZES[i % len(SIZES)] for i in range(MAX)]
    out += [full, full[::-1], [int(k) for k in rng.choice(SIZES, MAX)], [0] * 63 + [65], [65] + [0] * 63, [735] * MAX, [2] * MAX]
    assert {len(l) for l in out} == {1, 2, 5, 64}
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("decoder_batch") / "libdecoder_batch_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "tests", "host"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "decoder_batch_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_decoder_batch_arg_bytes.restype = ctypes.c_size_t
    L.psfm_host_decoder_batch_layout.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.psfm_host_decoder_batch_find.argtypes = [vp, ctypes.c_int]
    L.psfm_host_decoder_batch_plan_mismatches.argtypes = [vp, ctypes.c_int]
    L.psfm_host_decoder_batch_plan_mismatches.restype = ctypes.c_long
    L.psfm_host_decoder_workspace_bytes.argtypes = [ctypes.c_long]
    L.psfm_host_decoder_workspace_bytes.restype = ctypes.c_size_t
    L.psfm_host_decoder_tables.argtypes = [ctypes.c_long, vp, vp]
    L.psfm_host_decoder_tables.restype = None
    L.psfm_host_traj_decode.argtypes = [vp, vp, ctypes.c_long, vp, ctypes.c_size_t, vp, vp, vp]
    L.psfm_host_traj_decode_batch.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp]
    return L


def layout(L, ks, n_win=None):
    """(status, k[64], ws_off[64], tile0[64], slice0[64], (n_win, tiles, slices, bad), total) of the header's layout."""
    n_win = len(ks) if n_win is None else n_win
    k = (ctypes.c_long * max(len(ks), 1))(*ks)
    cols = [(ctypes.c_long * MAX)() for _ in range(4)]
    info, total = (ctypes.c_long * 4)(), ctypes.c_size_t(12345)
    rc = L.psfm_host_decoder_batch_layout(k, n_win, *cols, info, ctypes.byref(total))
    return (rc,) + tuple(list(c) for c in cols) + (tuple(info), int(total.value))


def single_layout(L, k):
    ws = (ctypes.c_long * 14)()
    L.psfm_host_decoder_tables(k, (ctypes.c_long * 8)(), ws)
    return list(ws)


def test_the_table_and_a_layer_fit_the_kernel_arguments(host):
    assert host.psfm_host_decoder_batch_max() == MAX
    assert host.psfm_host_decoder_batch_arg_bytes() <= 4096


@pytest.mark.parametrize("ks", k_lists(), ids=lambda ks: "n%d_%s" % (len(ks), "_".join(str(k) for k in ks[:5])))
def test_maps_offsets_and_lookup_against_enumeration(host, ks):
    rc, k, ws_off, tile0, slice0, (n_win, tiles, slices, bad), total = layout(host, ks)
    assert rc == 0 and n_win == len(ks) and bad == -1
    assert k[:n_win] == ks and all(v == 0 for v in k[n_win:])
    assert all(v == INT32_MAX for v in tile0[n_win:] + slice0[n_win:])
    # brute force: every (window, tile) and every (window, slice) once, window-major and ascending
    want_tiles = [(b, t) for b, kb in enumerate(ks) for t in range(-(-kb // TILE))]
    want_slices = [(b, s) for b, kb in enumerate(ks) for s in range(-(-kb // SLICE))]
    assert tiles == len(want_tiles) and slices == len(want_slices)
    for first, want in ((tile0, want_tiles), (slice0, want_slices)):
        col = (ctypes.c_long * MAX)(*first)
        got = []
        for blk in range(len(want)):
            b = host.psfm_host_decoder_batch_find(col, blk)
            got.append((b, blk - first[b]))
        assert got == want
        assert len(set(got)) == len(got)
    # the window layouts: psfm_dec_workspace(k) each, at 256-aligned disjoint offsets that add up to the size function's answer
    end = 0
    for b, kb in enumerate(ks):
        if kb == 0:
            continue
        one = single_layout(host, kb)
        assert ws_off[b] % 256 == 0 and ws_off[b] == end, (b, ws_off[b], end)
        assert one[11] == host.psfm_host_decoder_workspace_bytes(kb)
        end = ws_off[b] + one[11]
        assert (tile0[b + 1] if b + 1 < n_win else tiles) - tile0[b] == one[12]
        assert (slice0[b + 1] if b + 1 < n_win else slices) - slice0[b] == one[13]
    assert total == end == sum(host.psfm_host_decoder_workspace_bytes(kb) for kb in ks if kb)        # (an empty window takes nothing)
    # the plan by names, resolved per window, is the single call's plan for that window: every address, every field
    assert host.psfm_host_decoder_batch_plan_mismatches((ctypes.c_long * len(ks))(*ks), len(ks)) == 0


def test_refusals(host):
    for ks, at in (([65, 2, 0, 1, 64], 3), ([1], 0), ([2, -1], 1), ([64, 65, 2 ** 24], 2), ([-5, 1], 0)):
        rc, _, _, _, _, info, total = layout(host, ks)
        assert rc == 2 and info[3] == at and total == 0, ks
        assert host.psfm_host_decoder_batch_plan_mismatches((ctypes.c_long * len(ks))(*ks), len(ks)) == -1
    for n in (65, -1, 1000):
        rc, _, _, _, _, _, total = layout(host, [2] * 65, n_win=n)
        assert rc == 1 and total == 0, n
    assert layout(host, [2 ** 24 - 1])[0] == 0                     # the single call's cap is the window's cap


@pytest.mark.parametrize("ks", [[], [0], [0, 0], [0] * 5, [0] * 64])
def test_an_all_zero_list_plans_no_launch(host, ks):
    rc, k, ws_off, tile0, slice0, (n_win, tiles, slices, _), total = layout(host, ks)
    assert rc == 0 and n_win == len(ks) and tiles == 0 and slices == 0 and total == 0
    assert host.psfm_host_traj_decode_batch(len(ks), None, (ctypes.c_long * max(len(ks), 1))(*ks), None, None, 0, None, None, None) == 0


def test_the_host_batch_gives_the_bits_of_the_host_single_call(host):
    """[65, 2, 0, 513, 64]: a tile boundary, the smallest window, an empty one in the middle, a slice boundary -- one walk over the
    plan by names, a workspace full of NaN, against psfm_host_traj_decode per window."""
    packed = pack_decoder_weights_host(seeded_decoder_weights())
    ks = [65, 2, 0, 513, 64]
    xs = [np.ascontiguousarray(seeded_decoder_inputs(k, 900 + i)) for i, k in enumerate(ks)]
    want = []
    for x, k in zip(xs, ks):
        need = host.psfm_host_decoder_workspace_bytes(k)
        ws = np.full(need, 0xFF, np.uint8)
        lo, pr, pd = np.full(k, np.nan, np.float32), np.full(k, np.nan, np.float32), np.full(k, 77, np.uint8)
        if k:
            assert host.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, k, ws.ctypes.data, need, lo.ctypes.data, pr.ctypes.data, pd.ctypes.data) > 0
        want.append((lo, pr, pd))
    total = layout(host, ks)[6]
    ws = np.full(total + 64, 0xFF, np.uint8)
    ws[total:] = 0x5A
    got = [(np.full(k, np.nan, np.float32), np.full(k, np.nan, np.float32), np.full(k, 77, np.uint8)) for k in ks]
    vp = ctypes.c_void_p
    ptrs = lambda arrs: (vp * len(ks))(*[a.ctypes.data if a.size else None for a in arrs])
    kk = (ctypes.c_long * len(ks))(*ks)
    args = (len(ks), ptrs(xs), kk, packed.ctypes.data, ws.ctypes.data)
    outs = (ptrs([g[0] for g in got]), ptrs([g[1] for g in got]), ptrs([g[2] for g in got]))
    assert host.psfm_host_traj_decode_batch(*args, total - 1, *outs) == -1
    assert host.psfm_host_traj_decode_batch(*args, total, *outs) == 39
    assert (ws[total:] == 0x5A).all()
    for b, (g, w) in enumerate(zip(got, want)):
        for u, v in zip(g, w):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), b
        assert ks[b] == 0 or np.isfinite(g[0]).all()


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from psfm_motion_seg.decoder import decode_windows_device
    from psfm_motion_seg.merge_labels import decode_groups, label_sequences_batched, label_trajectories_batched
    packed = np.zeros(529497, np.float32)
    with pytest.raises(RuntimeError):
        decode_windows_device([np.zeros((16, 4), np.float32)], packed)
    with pytest.raises(RuntimeError):
        label_trajectories_batched(23, 10, (48, 64), (30, 50), 1000, packed, packed, lambda t: None)
    assert label_sequences_batched([], [], 10, (48, 64), (30, 50), 1000, packed, packed, lambda s, t: None) == []
    # the grouping is plain arithmetic: consecutive windows, a group closes before the window that would take it above the cap
    assert decode_groups([5, 5, 5], 1) == [(0, 1), (1, 2), (2, 3)] and decode_groups([5, 5, 5], 10) == [(0, 2), (2, 3)]
    assert decode_groups([5, 5, 5]) == [(0, 3)] and decode_groups([50, 1, 1], 10) == [(0, 1), (1, 3)] and decode_groups([], 3) == []
