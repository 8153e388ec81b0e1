"""sfm/convert.py:43-104 of the reference (save_depth_pose / write_depth_pose_from_colmap_format): the model the mapper wrote becomes,
per registered image, a sparse depth map (depths/NAME.npy (h, w) f64 and a display PNG), the world-to-camera pose (poses/NAME.txt) and
the intrinsics (intrinsics/NAME.txt).

The model is read into arrays, never into per-element Python objects: images.bin is one header parse per image and one np.frombuffer
over its `ddq` records; points3D.bin, whose records have variable length, is walked by the library's bounds-checked host scan
(psfm_colmap_points3d_count / _scan).  The maps are made on the device (psfm_sparse_depth, csrc/psfm_sparse_depth.hip) batch by batch;
sparse_depth_host is the same rules in NumPy, the model the tests compare the device with bit for bit.  The rules:
pixel = clip(int32(np.round(xy)), 0, size - 1) from the model's xys; depth = ((r20 X + r21 Y) + r22 Z) + t2, each operation rounded
once; point3D_id -1 is skipped; of several observations of one pixel the last in list order wins; other pixels hold 0.0.

The display PNG (convert.py:26-41, :95) is made either on the host (normalize_depth_for_display, the reference's route) or on the device
(psfm_depth_display, csrc/psfm_depth_display.hip: the RGBA bytes plt.imsave would write, bit for bit; depth_display_host is the same
rule in NumPy), or not at all (png=False).

Only .bin models are read: a .txt model raises NotImplementedError (convert it with COLMAP's model_converter).
"""
import collections
import os
import queue
import struct
import threading
import warnings

import numpy as np

Camera = collections.namedtuple("Camera", ["id", "model", "width", "height", "params"])
ImageHeader = collections.namedtuple("ImageHeader", ["id", "qvec", "tvec", "camera_id", "name"])
ModelArrays = collections.namedtuple("ModelArrays", ["cameras", "images", "obs_off", "xys", "point3D_ids", "ids", "xyz"])
ModelArrays.__doc__ = """cameras {id: Camera}; images [ImageHeader] in file order; image i owns rows obs_off[i]:obs_off[i+1] of xys (n_obs, 2) f64
and point3D_ids (n_obs) i64; ids (n_pts) i64 and xyz (n_pts, 3) f64 in file order."""

# COLMAP's camera models: model_id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5),
                 10: ("THIN_PRISM_FISHEYE", 12)}

IMAGE_DESC = np.dtype([("obs_begin", "<i8"), ("obs_end", "<i8"), ("r20", "<f8"), ("r21", "<f8"), ("r22", "<f8"), ("t2", "<f8"),
                       ("w", "<i4"), ("h", "<i4"), ("out_off", "<i8")])
assert IMAGE_DESC.itemsize == 64
BYTES_PER_PIXEL = 12          # f64 map + u32 winner: what the context's budget counts


# ---- reading the model ---------------------------------------------------------------------------------------------------------------

def _need(buf, pos, n, what):
    if pos + n > len(buf):
        raise ValueError("%s is truncated: %d bytes at offset %d, the file has %d" % (what, n, pos, len(buf)))


def read_cameras_bin(path):
    buf = open(path, "rb").read()
    _need(buf, 0, 8, path)
    n, pos, cameras = struct.unpack_from("<Q", buf, 0)[0], 8, {}
    for _ in range(n):
        _need(buf, pos, 24, path)
        cam_id, model_id, width, height = struct.unpack_from("<iiQQ", buf, pos)
        pos += 24
        if model_id not in CAMERA_MODELS:
            raise ValueError("%s: camera %d has unknown model id %d" % (path, cam_id, model_id))
        name, k = CAMERA_MODELS[model_id]
        _need(buf, pos, 8 * k, path)
        cameras[cam_id] = Camera(cam_id, name, width, height, np.frombuffer(buf, "<f8", k, pos).copy())
        pos += 8 * k
    return cameras


def read_images_bin(path):
    """-> ([ImageHeader], obs_off (n_img + 1) i64, xys (n_obs, 2) f64, point3D_ids (n_obs) i64)."""
    buf = open(path, "rb").read()
    _need(buf, 0, 8, path)
    n, pos = struct.unpack_from("<Q", buf, 0)[0], 8
    headers, where, off = [], [], [0]
    for _ in range(n):
        _need(buf, pos, 64, path)
        v = struct.unpack_from("<idddddddi", buf, pos)
        pos += 64
        end = buf.find(b"\x00", pos)
        if end < 0:
            raise ValueError("%s is truncated: an image name without its terminator at offset %d" % (path, pos))
        name = buf[pos:end].decode("utf-8")
        pos = end + 1
        _need(buf, pos, 8, path)
        k = struct.unpack_from("<Q", buf, pos)[0]
        pos += 8
        _need(buf, pos, 24 * k, path)
        headers.append(ImageHeader(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name))
        where.append(pos)
        off.append(off[-1] + k)
        pos += 24 * k
    obs_off = np.array(off, np.int64)
    xys, ids = np.empty((off[-1], 2), np.float64), np.empty(off[-1], np.int64)
    for i, p in enumerate(where):
        k = off[i + 1] - off[i]
        rec = np.frombuffer(buf, "<f8", 3 * k, p).reshape(k, 3)          # (x, y, id) records: the id's 8 bytes seen as f64
        xys[off[i]:off[i + 1]] = rec[:, :2]
        ids[off[i]:off[i + 1]] = rec[:, 2].view("<i8")
    return headers, obs_off, xys, ids


def read_points3d_bin(path):
    """-> (ids (n) i64, xyz (n, 3) f64) in file order, through the library's host scan (no GPU is touched)."""
    import ctypes
    from point_trajectory import _hip
    buf = np.fromfile(path, np.uint8)
    L, n = _hip.lib(), ctypes.c_uint64(0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    if L.psfm_colmap_points3d_count(p, buf.size, ctypes.byref(n)) != _hip.PSFM_OK:
        raise ValueError("%s: %s" % (path, L.psfm_last_error().decode("utf-8", "replace")))
    ids, xyz = np.empty(n.value, np.uint64), np.empty((n.value, 3), np.float64)
    if L.psfm_colmap_points3d_scan(p, buf.size, ids.ctypes.data_as(ctypes.c_void_p), xyz.ctypes.data_as(ctypes.c_void_p), None, None) != _hip.PSFM_OK:
        raise ValueError("%s: %s" % (path, L.psfm_last_error().decode("utf-8", "replace")))
    if ids.size and int(ids.max()) >= 2 ** 63:
        raise ValueError("%s: a point3D id of 2^63 or more (an observation's id is a signed 64-bit number)" % path)
    return ids.view(np.int64), xyz


def read_model_arrays(path):
    """The model under `path` (cameras.bin, images.bin, points3D.bin) as ModelArrays."""
    has = lambda ext: all(os.path.isfile(os.path.join(path, n + ext)) for n in ("cameras", "images", "points3D"))
    if not has(".bin"):
        if has(".txt"):
            raise NotImplementedError("%s holds a text model; only .bin models are read (colmap model_converter --output_type BIN)" % path)
        raise FileNotFoundError("Could not find a binary COLMAP model at %s" % path)
    cameras = read_cameras_bin(os.path.join(path, "cameras.bin"))
    headers, obs_off, xys, p3d = read_images_bin(os.path.join(path, "images.bin"))
    ids, xyz = read_points3d_bin(os.path.join(path, "points3D.bin"))
    return ModelArrays(cameras, headers, obs_off, xys, p3d, ids, xyz)


def model_from_dicts(cameras, images, points3D):
    """The reference's three dicts (read_write_model.read_model) as ModelArrays; images keep the dict's order."""
    headers, off, xs, ps = [], [0], [], []
    for im in images.values():
        headers.append(ImageHeader(im.id, np.asarray(im.qvec, np.float64), np.asarray(im.tvec, np.float64), im.camera_id, im.name))
        p = np.asarray(im.point3D_ids, np.int64).reshape(-1)
        xs.append(np.asarray(im.xys, np.float64).reshape(len(p), 2))
        ps.append(p)
        off.append(off[-1] + len(p))
    n = len(points3D)
    ids = np.fromiter(points3D.keys(), np.int64, n)
    xyz = np.empty((n, 3), np.float64)
    for k, pt in enumerate(points3D.values()):
        xyz[k] = pt.xyz
    cams = {k: Camera(c.id, c.model, c.width, c.height, np.asarray(c.params, np.float64)) for k, c in cameras.items()}
    return ModelArrays(cams, headers, np.array(off, np.int64), np.concatenate(xs) if xs else np.empty((0, 2)),
                       np.concatenate(ps) if ps else np.empty(0, np.int64), ids, xyz)


# ---- poses, intrinsics, descriptors -------------------------------------------------------------------------------------------------

def qvec2rotmat(q):
    """R of a unit quaternion (w, x, y, z), term by term the reference's expression (read_write_model.py:459-469): same operations on
    the same np.float64 scalars, so R is bit-equal to the reference's."""
    w, x, y, z = q[0], q[1], q[2], q[3]
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


def intrinsics(camera):
    if camera.model == "SIMPLE_PINHOLE":
        f, cx, cy = camera.params
    elif camera.model == "SIMPLE_RADIAL":
        f, cx, cy, _ = camera.params
    else:
        raise NotImplementedError("camera model %s (only SIMPLE_PINHOLE and SIMPLE_RADIAL, as in the reference)" % camera.model)
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])


def image_descriptors(model):
    """One IMAGE_DESC row per image, out_off counted from the model's first image (a batch subtracts its own first offset)."""
    d = np.zeros(len(model.images), IMAGE_DESC)
    out = 0
    for i, im in enumerate(model.images):
        cam = model.cameras[im.camera_id]
        intrinsics(cam)                                                   # (refuses other camera models before any work)
        R = qvec2rotmat(im.qvec)
        d[i] = (model.obs_off[i], model.obs_off[i + 1], R[2, 0], R[2, 1], R[2, 2], im.tvec[2], cam.width, cam.height, out)
        out += int(cam.width) * int(cam.height)
    return d


def batches(desc, budget_bytes):
    """[(first image, one past the last)]: consecutive images whose maps + winner maps fit budget_bytes (0: everything in one batch);
    an image larger than the budget is a batch of its own."""
    n, out, a = len(desc), [], 0
    while a < n:
        b, used = a, 0
        while b < n:
            need = BYTES_PER_PIXEL * int(desc["w"][b]) * int(desc["h"][b])
            if b > a and budget_bytes > 0 and used + need > budget_bytes:
                break
            used += need
            b += 1
        out.append((a, b))
        a = b
    return out


# ---- the NumPy model -------------------------------------------------------------------------------------------------------------------

def coord_ok(v):
    with np.errstate(invalid="ignore"):
        return (np.abs(v) < 2.0 ** 31) & (np.rint(v) < 2.0 ** 31)


def pixels(v, n):
    return np.clip(np.rint(v), 0.0, float(n - 1)).astype(np.int32)


def point_rows(ids, obs_ids):
    """Row of every observation's point (-1 for id -1): stable sort, the last of equal ids.  KeyError(smallest missing id)."""
    order = np.argsort(ids, kind="stable")
    srt = ids[order]
    rows = np.full(len(obs_ids), -1, np.int64)
    v = obs_ids != -1
    g = np.searchsorted(srt, obs_ids[v], side="right") - 1
    found = g >= 0
    found[found] = srt[g[found]] == obs_ids[v][found]
    if not found.all():
        raise KeyError(int(obs_ids[v][~found].min()))
    rows[v] = order[g]
    return rows


def sparse_depth_host(model):
    """Yields (image name, depth (h, w) f64 ndarray) per image: the rules of csrc/psfm_sparse_depth.h in NumPy."""
    desc = image_descriptors(model)
    rows = point_rows(model.ids, model.point3D_ids)
    for i, im in enumerate(model.images):
        a, b = int(desc["obs_begin"][i]), int(desc["obs_end"][i])
        w, h = int(desc["w"][i]), int(desc["h"][i])
        depth = np.zeros(h * w, np.float64)
        r = rows[a:b]
        v = np.flatnonzero(r >= 0)                                        # list order
        if len(v):
            xy = model.xys[a:b][v]
            if not (coord_ok(xy[:, 0]) & coord_ok(xy[:, 1])).all():
                raise ValueError("image %s: a coordinate that is not finite or does not round into int32" % im.name)
            lin = pixels(xy[:, 1], h).astype(np.int64) * w + pixels(xy[:, 0], w)
            X = model.xyz[r[v]]
            d = ((desc["r20"][i] * X[:, 0] + desc["r21"][i] * X[:, 1]) + desc["r22"][i] * X[:, 2]) + desc["t2"][i]
            o = np.argsort(lin, kind="stable")                            # per pixel its observations in list order: the last wins
            s = lin[o]
            last = np.r_[s[1:] != s[:-1], True]
            depth[s[last]] = d[o[last]]
        yield im.name, depth.reshape(h, w)


# ---- the device ------------------------------------------------------------------------------------------------------------------------

def sort_ids_device(ctx, ids_dev):
    """ids (device i64, all in [0, 2^32)) -> (sorted ids i64, rows i32) through the library's record sort."""
    import torch
    from point_trajectory import _hip
    n = ids_dev.numel()
    srt = torch.empty(n, dtype=torch.int64, device=ids_dev.device)
    row = torch.empty(n, dtype=torch.int32, device=ids_dev.device)
    _hip.check(_hip.lib().psfm_sparse_depth_sort_ids(ctx.handle, _hip.ptr(ids_dev), n, _hip.ptr(srt), _hip.ptr(row), _hip.current_stream_ptr(ctx.device)))
    return srt, row


def sort_ids_device64(ctx, ids_dev):
    """ids (device i64, all in [0, 2^63)) -> (sorted ids i64, rows i32) through the library's 64-bit record sort
    (psfm_sort_records64 over the bit length of the largest id).  A negative id is a ValueError."""
    import torch
    from point_trajectory import _hip
    n = ids_dev.numel()
    if n == 0:
        return ids_dev.clone(), torch.empty(0, dtype=torch.int32, device=ids_dev.device)
    lo, hi = int(ids_dev.min()), int(ids_dev.max())
    if lo < 0:
        raise ValueError("sort_ids_device64 needs every id in [0, 2^63): got %d" % lo)
    srt = ids_dev.contiguous().clone()                      # (sorted in place; as u64 keys an id in [0, 2^63) is its own value)
    row = torch.arange(n, dtype=torch.int32, device=ids_dev.device)
    _hip.check(_hip.lib().psfm_sort_records64(ctx.handle, _hip.ptr(srt), _hip.ptr(row), n, max(1, hi.bit_length()),
                                              _hip.current_stream_ptr(ctx.device)))
    return srt, row


def sparse_depth_device(model, ctx=None, sort="auto"):
    """Yields (image name, depth (h, w) f64 torch tensor on the device) batch by batch; a batch is as many consecutive images as the
    context's budget admits (Context.set_sparse_depth; 12 bytes per pixel).  sort: "device" (ids below 2^32: the library's record
    sort), "device64" (ids below 2^63: its 64-bit record sort), "host" (np.argsort, any id), "auto" (device when every id is below
    2^32, else host).  An observation whose id names no point raises KeyError(the smallest such id of the batch), as the reference's
    dict lookup does; the context stays usable."""
    for batch in sparse_depth_batches(model, ctx, sort):
        yield from batch


def sparse_depth_batches(model, ctx=None, sort="auto"):
    """sparse_depth_device one batch at a time: yields [(image name, depth)] whose maps follow each other in one device buffer (what
    depth_display_device takes)."""
    import ctypes
    import torch
    from point_trajectory import _hip
    if ctx is None:
        ctx = _hip.context()
    dev = torch.device("cuda", ctx.device)
    L, sp = _hip.lib(), _hip.current_stream_ptr(ctx.device)
    desc = image_descriptors(model)
    n_pts = len(model.ids)
    small = n_pts == 0 or (int(model.ids.min()) >= 0 and int(model.ids.max()) < 2 ** 32)
    if sort == "auto":
        sort = "device" if small else "host"
    if sort == "device":
        if not small:
            raise ValueError("sort='device' needs every point3D id in [0, 2^32)")
        srt, row = sort_ids_device(ctx, torch.from_numpy(np.ascontiguousarray(model.ids)).to(dev))
    elif sort == "device64":
        if n_pts and int(model.ids.min()) < 0:
            raise ValueError("sort='device64' needs every point3D id in [0, 2^63)")
        srt, row = sort_ids_device64(ctx, torch.from_numpy(np.ascontiguousarray(model.ids, np.int64)).to(dev))
    elif sort == "host":
        order = np.argsort(model.ids, kind="stable")
        srt, row = torch.from_numpy(model.ids[order]).to(dev), torch.from_numpy(order.astype(np.int32)).to(dev)
    else:
        raise ValueError("sort must be 'auto', 'device', 'device64' or 'host'")
    xyz = torch.from_numpy(np.ascontiguousarray(model.xyz, np.float64)).to(dev)
    xys = torch.from_numpy(np.ascontiguousarray(model.xys, np.float64)).to(dev)
    ids = torch.from_numpy(np.ascontiguousarray(model.point3D_ids, np.int64)).to(dev)
    budget = ctypes.c_int64(0)
    _hip.check(L.psfm_ctx_get_sparse_depth_budget(ctx.handle, ctypes.byref(budget)))
    for a, b in batches(desc, int(budget.value)):
        d = desc[a:b].copy()
        d["out_off"] -= d["out_off"][0]
        n_pix = int(d["out_off"][-1]) + int(d["w"][-1]) * int(d["h"][-1])
        out = torch.empty(n_pix, dtype=torch.float64, device=dev)
        missing = ctypes.c_int64(-1)
        st = L.psfm_sparse_depth(ctx.handle, _hip.ptr(xys), _hip.ptr(ids), ids.numel(), d.ctypes.data_as(ctypes.c_void_p), b - a,
                                 _hip.ptr(srt), _hip.ptr(row), _hip.ptr(xyz), n_pts, _hip.ptr(out), ctypes.byref(missing), sp)
        if st == _hip.PSFM_ERR_ARG and b"names 3-D point" in L.psfm_last_error():
            raise KeyError(int(missing.value))
        _hip.check(st)
        batch = []
        for i in range(a, b):
            o, w, h = int(d["out_off"][i - a]), int(d["w"][i - a]), int(d["h"][i - a])
            batch.append((model.images[i].name, out[o:o + h * w].view(h, w)))
        yield batch


# ---- the files ---------------------------------------------------------------------------------------------------------------------------

def normalize_depth_for_display(depth, pc=98, cmap="binary"):
    """The reference's display image (convert.py:26-41): 1 / (d + 1), stretched between its 2nd and 98th percentile over d > 0, through
    a matplotlib colour map, alpha dropped.  None for a map without a positive depth (the reference's percentile fails there)."""
    from matplotlib import pyplot as plt
    valid = depth > 0
    if not valid.any():
        return None
    inv = 1.0 / (depth + 1)
    z1, z2 = np.percentile(inv[valid], pc), np.percentile(inv[valid], 100 - pc)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.clip((inv - z2) / (z1 - z2), 0, 1)
    return plt.get_cmap(cmap)(inv.astype(np.float32))[:, :, :3]


def colour_table(cmap="binary"):
    """-> (table (256, 4) u8, bad (4,) u8): the bytes plt.imsave writes for colour index 0..255 and for NaN.  The map evaluated by
    matplotlib, times 255, truncated; alpha 255 (the reference drops alpha, imsave puts 1.0 back).  Data, not a formula: 'binary' is
    not 255 - i everywhere."""
    from matplotlib import pyplot as plt
    cm = plt.get_cmap(cmap)
    table = (cm(np.arange(256)) * 255).astype(np.uint8)
    bad = (np.asarray(cm(np.float32(np.nan)), np.float64) * 255).astype(np.uint8)
    table[:, 3], bad[3] = 255, 255
    return np.ascontiguousarray(table), np.ascontiguousarray(bad)


def percentile_rank(n, q):
    """np.percentile's 'linear' method on n sorted values -> (j, min(j + 1, n - 1), g): the two order statistics it reads and the
    weight between them, each operation rounded once as NumPy does."""
    vi = np.float64(n - 1) * (np.float64(q) / np.float64(100.0))
    j = int(np.floor(vi))
    return j, min(j + 1, n - 1), vi - np.float64(j)


def percentile_lerp(a, b, g):
    diff = b - a
    return b - diff * (np.float64(1.0) - g) if g >= 0.5 else a + diff * g


def depth_display_host(depth, pc=98, cmap="binary"):
    """The display image of one map by the rules of csrc/psfm_depth_display.h in NumPy, element by element what the reference's
    normalize_depth_for_display followed by plt.imsave's byte conversion gives: -> (rgba (h, w, 4) u8 or None for a map without a
    positive depth, z1, z2).  The model the tests compare the device with bit for bit."""
    depth = np.asarray(depth, np.float64)
    valid = depth > 0
    n = int(np.count_nonzero(valid))
    if n == 0:
        return None, 0.0, 0.0
    table, bad = colour_table(cmap)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (depth + 1.0)
        s = np.sort(inv[valid].view(np.uint64)).view(np.float64)          # (valid inv are >= 0: their bit patterns order like them)
        z = []
        for q in (pc, 100 - pc):
            j, j1, g = percentile_rank(n, q)
            z.append(percentile_lerp(s[j], s[j1], g))
        z1, z2 = z
        v = (inv - z2) / (z1 - z2)
        v = np.where(v < 0, 0.0, v)                                       # (NaN fails both comparisons and stays)
        v = np.where(v > 1, 1.0, v)
        v32 = v.astype(np.float32)
        xa = v32 * np.float32(256.0)
        nan = np.isnan(v32)
        index = np.where(xa == np.float32(256.0), 255, np.where(nan, 0, xa).astype(np.int64))
    rgba = table[index]
    rgba[nan] = bad
    return rgba, float(z1), float(z2)


def depth_display_device(maps, pc=98, cmap="binary", ctx=None):
    """The display images of the device maps of ONE batch of sparse_depth_batches, read where they are: maps = [(h, w) f64 device
    tensor] that follow each other in one buffer.  -> [(rgba (h, w, 4) u8 device tensor or None, z1, z2)] (psfm_depth_display,
    csrc/psfm_depth_display.hip); the images are views of one buffer."""
    import ctypes
    import torch
    from point_trajectory import _hip
    if ctx is None:
        ctx = _hip.context()
    maps = list(maps)
    if not maps:
        return []
    d = np.zeros(len(maps), IMAGE_DESC)
    base, off = maps[0].data_ptr(), 0
    for i, m in enumerate(maps):
        if m.dtype != torch.float64 or m.dim() != 2 or not m.is_contiguous() or m.data_ptr() != base + 8 * off:
            raise ValueError("depth_display_device: map %d is not the next (h, w) f64 map of one batch buffer" % i)
        d[i]["h"], d[i]["w"], d[i]["out_off"] = m.shape[0], m.shape[1], off
        off += m.numel()
    table, bad = colour_table(cmap)
    out = torch.empty((off, 4), dtype=torch.uint8, device=maps[0].device)
    n_valid, z = np.zeros(len(maps), np.int64), np.zeros((len(maps), 2), np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _hip.check(_hip.lib().psfm_depth_display(ctx.handle, base, p(d), len(maps), float(pc), p(table), p(bad), _hip.ptr(out), p(n_valid), p(z),
                                             _hip.current_stream_ptr(ctx.device)))
    res = []
    for i, m in enumerate(maps):
        o = int(d[i]["out_off"])
        res.append((out[o:o + m.numel()].view(m.shape[0], m.shape[1], 4) if n_valid[i] else None, float(z[i, 0]), float(z[i, 1])))
    return res


def _matplotlib():
    try:
        from matplotlib import pyplot as plt
        return plt
    except ImportError:
        warnings.warn("matplotlib is not installed: the depth PNGs are skipped (the .npy maps, poses and intrinsics are written)")
        return None


DEFAULT_DISPLAY = "device"    # display=None under device=True: 9.5 s against the host route's 16.3 s end to end at 101 x 1080p
                              # (profiles/EXPERIMENTS.md, section 21)


def save_model(output_dir, model, device=True, ctx=None, png=True, display=None, writers=1):
    """Writes depths/NAME.npy (+ .png), poses/NAME.txt, intrinsics/NAME.txt for every image of `model`.  device=True: the maps come
    from psfm_sparse_depth (a GPU is required); False: from the NumPy model.  png=False: no display PNG is computed or written.
    display: "host" (normalize_depth_for_display in the writer thread, the reference's route) or "device" (psfm_depth_display on the
    batch's maps in HBM; device=True only; the writer hands the ready RGBA bytes to the same plt.imsave); None: "host" without a
    device, DEFAULT_DISPLAY with one.  The .npy / .png files are written by `writers` threads (zlib releases the GIL; the files do not
    depend on their number) while the device works on the next batch."""
    if display is None:
        display = DEFAULT_DISPLAY if device else "host"
    if display not in ("host", "device"):
        raise ValueError("display must be 'host' or 'device'")
    if display == "device" and not device:
        raise ValueError("display='device' needs device=True: the maps of the NumPy model are not in device memory")
    writers = int(writers)
    if writers < 1:
        raise ValueError("writers must be >= 1")
    depth_dir, pose_dir, intr_dir = (os.path.join(output_dir, n) for n in ("depths", "poses", "intrinsics"))
    for p in (depth_dir, pose_dir, intr_dir):
        os.makedirs(p, exist_ok=True)
    stem = lambda name: os.path.splitext(name)[0]
    for im in model.images:
        np.savetxt(os.path.join(intr_dir, stem(im.name) + ".txt"), intrinsics(model.cameras[im.camera_id]))
    plt = _matplotlib() if png else None
    q, failed = queue.Queue(maxsize=8), []

    def writer():
        while True:
            item = q.get()
            if item is None:
                return
            if failed:
                continue                                                  # (keep draining: the producer must not block)
            try:
                name, depth, img = item
                np.save(os.path.join(depth_dir, stem(name) + ".npy"), depth)
                if img is None and plt is not None and display == "host":
                    img = normalize_depth_for_display(depth)
                if img is not None:
                    plt.imsave(os.path.join(depth_dir, stem(name) + ".png"), img)
            except BaseException as e:                                    # noqa: B902 -- handed to the caller below
                failed.append(e)

    threads = [threading.Thread(target=writer, name="psfm-depth-writer-%d" % k) for k in range(writers)]
    for th in threads:
        th.start()
    try:
        if device:
            for batch in sparse_depth_batches(model, ctx):
                imgs = [None] * len(batch)
                if display == "device" and plt is not None:
                    imgs = [r[0] for r in depth_display_device([d for _, d in batch], ctx=ctx)]
                for (name, depth), img in zip(batch, imgs):
                    q.put((name, depth.cpu().numpy(), None if img is None else img.cpu().numpy()))
        else:
            for name, depth in sparse_depth_host(model):
                q.put((name, depth, None))
    finally:
        for _ in threads:
            q.put(None)
        for th in threads:
            th.join()
    if failed:
        raise failed[0]
    for im in model.images:
        Rt = np.concatenate([qvec2rotmat(im.qvec), np.expand_dims(im.tvec, -1)], -1)
        np.savetxt(os.path.join(pose_dir, stem(im.name) + ".txt"), Rt)


def save_depth_pose(output_dir, cameras, images, points3D, device=True, png=True, display=None, writers=1):
    """The reference's signature: its three dicts (any mappings of objects with the same attributes)."""
    save_model(output_dir, model_from_dicts(cameras, images, points3D), device=device, png=png, display=display, writers=writers)


def write_depth_pose_from_colmap_format(input_dir, output_dir, device=True, png=True, display=None, writers=1):
    save_model(output_dir, read_model_arrays(input_dir), device=device, png=png, display=display, writers=writers)
