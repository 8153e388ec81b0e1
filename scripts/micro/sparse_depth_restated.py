"""The algorithm of the reference's write_depth_pose_from_colmap_format (sfm/convert.py:43-104 over
sfm/colmap_utils/read_write_model.py:225-257, :336-363), restated step for step in this project's own words, as the yardstick of
scripts/micro/sparse_depth.py on machines that do not hold the reference: per-element `struct` reads into dicts of tuples, a Python
loop with a dict lookup per keypoint, matmul, NumPy's indexed assignment, the display PNG, np.savetxt.  Same operations on the same
types, so its maps equal the reference's bit for bit (tests/test_sparse_depth_host.py checks that on the fixtures).  Not used by the
package."""
import os
import struct

import numpy as np

from psfm_sfm.convert import CAMERA_MODELS, qvec2rotmat


def _unpack(fid, n, fmt):
    return struct.unpack("<" + fmt, fid.read(n))


def read_cameras(path):
    cams = {}
    with open(path, "rb") as fid:
        for _ in range(_unpack(fid, 8, "Q")[0]):
            cam_id, model_id, width, height = _unpack(fid, 24, "iiQQ")
            name, k = CAMERA_MODELS[model_id]
            cams[cam_id] = (name, width, height, np.array(_unpack(fid, 8 * k, "d" * k)))
    return cams


def read_images(path, limit=None):
    """limit: stop after that many images (the yardstick is timed on a part of the model)."""
    images = {}
    with open(path, "rb") as fid:
        n = _unpack(fid, 8, "Q")[0]
        for _ in range(n if limit is None else min(n, limit)):
            v = _unpack(fid, 64, "idddddddi")
            name = b""
            ch = fid.read(1)
            while ch != b"\x00":
                name += ch
                ch = fid.read(1)
            k = _unpack(fid, 8, "Q")[0]
            rec = _unpack(fid, 24 * k, "ddq" * k)
            xys = np.column_stack([tuple(map(float, rec[0::3])), tuple(map(float, rec[1::3]))])
            ids = np.array(tuple(map(int, rec[2::3])))
            images[v[0]] = (np.array(v[1:5]), np.array(v[5:8]), v[8], name.decode("utf-8"), xys, ids)
    return images


def read_points(path):
    pts = {}
    with open(path, "rb") as fid:
        for _ in range(_unpack(fid, 8, "Q")[0]):
            v = _unpack(fid, 43, "QdddBBBd")
            length = _unpack(fid, 8, "Q")[0]
            track = _unpack(fid, 8 * length, "ii" * length)
            pts[v[0]] = (np.array(v[1:4]), np.array(v[4:7]), np.array(v[7]), np.array(tuple(map(int, track[0::2]))),
                         np.array(tuple(map(int, track[1::2]))))
    return pts


def display(depth, pc=98):
    from matplotlib import pyplot as plt
    valid = depth > 0
    depth = 1. / (depth + 1)
    z1 = np.percentile(depth[valid], pc)
    z2 = np.percentile(depth[valid], 100 - pc)
    depth = np.clip((depth - z2) / (z1 - z2), 0, 1)
    return np.delete(plt.get_cmap("binary")(depth.astype(np.float32)), 3, 2)


def save(output_dir, cams, images, pts, png=True):
    dirs = [os.path.join(output_dir, n) for n in ("depths", "poses", "intrinsics")]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    for key in images.keys():
        qvec, tvec, cam_id, name, xys, ids = images[key]
        model, w, h, params = cams[cam_id]
        if model == "SIMPLE_PINHOLE":
            f, cx, cy = params
        elif model == "SIMPLE_RADIAL":
            f, cx, cy, _ = params
        else:
            raise NotImplementedError
        K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
        stem = os.path.splitext(name)[0]
        np.savetxt(os.path.join(dirs[2], stem + ".txt"), K)
        R, t = qvec2rotmat(qvec), np.expand_dims(tvec, -1)
        points, valid_xys = [], []
        for i in range(len(ids)):
            idx = ids[i]
            if idx == -1:
                continue
            points.append(pts[idx][0])
            valid_xys.append(xys[i])
        depth = np.zeros(shape=(h, w))
        if points:
            cam = np.matmul(R, np.transpose(np.array(points))) + t
            z = np.transpose(np.matmul(K, cam))[:, -1]
            xy = np.round(np.array(valid_xys)).astype(np.int32)
            xy[:, 0] = np.clip(xy[:, 0], 0, w - 1)
            xy[:, 1] = np.clip(xy[:, 1], 0, h - 1)
            depth[xy[:, 1], xy[:, 0]] = z
        np.save(os.path.join(dirs[0], stem + ".npy"), depth)
        if png:
            from matplotlib import pyplot as plt
            plt.imsave(os.path.join(dirs[0], stem + ".png"), display(depth))
        np.savetxt(os.path.join(dirs[1], stem + ".txt"), np.concatenate([R, t], -1))


def convert(input_dir, output_dir, limit=None, png=True):
    save(output_dir, read_cameras(os.path.join(input_dir, "cameras.bin")), read_images(os.path.join(input_dir, "images.bin"), limit),
         read_points(os.path.join(input_dir, "points3D.bin")), png)
