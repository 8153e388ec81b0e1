#!/usr/bin/env python3
"""Golden vectors for the label merge (motion_seg/main_motion_segmentation.py:89-129) and the match tables built from its
output, produced by the REFERENCE's own functions: main_motion_segmentation.py is imported UNMODIFIED, as a package (its relative
import of load_cut_seq resolves to the reference's file), run on the CPU with a stub network, and the reference's traj_to_matches
(sfm/matches_from_flow.py:51-118) is then run over the track.npy that function wrote.

Stand-ins, on top of oracle/ref_shim.load_consumers() (cv2 / cvbase stubs, the restated TrajectorySet):
  torchvision.transforms.ToTensor   HWC ndarray -> CHW tensor          torch.Tensor.cuda / Module.cuda   identity
  torch.load                        an empty state dict                tqdm.contrib.tzip                  zip
  core.utils.utils                  load_config_file -> model_name "traj_oa_depth", resolution = the case's input size, a
                                    non-empty resume_path; draw_traj_cls -> zeros (H, n * W, 3)
  core.network.traj_oa_depth        a module whose forward returns seeded uniform scores (1,1,K) and records score > 0.5 per call
  cv2.VideoWriter / VideoWriter_fourcc  no-ops;  cv2.imread  blank frames of the case's size
The saved set is the CPU checker's track() on a seeded psfm_synth sequence (bit-exactly what the HIP path produces), length >= 3,
pickled as ref_shim.TrajectorySet like make_consumer_golden.py does.  Only arrays are stored.  Run in the build container, never
on the GPU machine:
    python tests/golden/make_labels_golden.py
"""
import hashlib
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import psfm_synth                     # noqa: E402
from _common import input_hash       # noqa: E402
from oracle import oracle as orc     # noqa: E402
from oracle import ref_shim          # noqa: E402

# name, T, H, W, ratio, seed, sigma, occluders, flow amplitude (px), window, network input size, seed of the stub network's scores
CASES = [("labels_48x64_t23_w10", 23, 48, 64, 2, 311, 0.3, 2, 3.0, 10, (30, 50), 7001),      # (a) three windows, the last overlaps
         ("labels_48x64_t23_full", 23, 48, 64, 2, 311, 0.3, 2, 3.0, 28, (30, 50), 7002),     # (b) window >= length (load_cut_seq.py:51-58)
         # (c) the slow flow of matches_24x32_t27_dyn: trajectories keep more than K = 20 points after the labels drop some
         ("labels_24x32_t27_w10", 27, 24, 32, 2, 302, 0.05, 1, 0.5, 10, (30, 50), 7003)]
MAX_BYTES = 847951      # the largest fixture already in tests/golden


def load_main_motion_segmentation(state):
    """The reference's motion_seg package under an alias, with the stand-ins of the module docstring; `state` carries the case's
    input size, score seed and the recorded predictions."""
    import torch
    ref = ref_shim.load_consumers()           # cv2 / cvbase stubs; core.dataset.data_utils becomes importable
    cv2 = ref.cv2

    class _Writer:
        def __init__(self, *a, **k): pass
        def write(self, img): pass
        def release(self): pass
    cv2.VideoWriter = _Writer
    cv2.VideoWriter_fourcc = lambda *a: 0

    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")

    class ToTensor:
        def __call__(self, a):
            a = np.asarray(a)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    tv.transforms.ToTensor = ToTensor
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.transforms"] = tv.transforms
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.load = lambda *a, **k: {"model_state_dict": {}}

    import tqdm.contrib
    tqdm.contrib.tzip = zip

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    def load_config_file(path):
        return types.SimpleNamespace(model_name="traj_oa_depth", resolution=state["input_size"], resume_path="checkpoint.pth")

    def draw_traj_cls(imgs, traj, mask, pred, gt):
        return np.zeros((state["input_size"][0], len(imgs) * state["input_size"][1], 3))

    class traj_oa_depth(torch.nn.Module):
        def __init__(self, window_size, resolution):
            super().__init__()

        def forward(self, batch):
            K = int(batch["traj"].shape[2])
            score = state["rng"].uniform(size=(1, 1, K))
            state["preds"].append(score[0, 0] > 0.5)
            return torch.from_numpy(score)
    importlib.import_module("core.dataset.data_utils")       # (the namespace package `core` of the reference, loaded by the shim)
    mod("core.utils")
    mod("core.utils.utils", load_config_file=load_config_file, draw_traj_cls=draw_traj_cls)
    mod("core.network")
    mod("core.network.traj_oa_depth", traj_oa_depth=traj_oa_depth)
    alias = "psfm_reference_motion_seg"
    pkg = types.ModuleType(alias)
    pkg.__path__ = [os.path.join(ref_shim.REFERENCE_ROOT, "motion_seg")]
    sys.modules[alias] = pkg
    mms = importlib.import_module(alias + ".main_motion_segmentation")
    return ref, mms


def tables_of(data, names):
    kp_off = np.zeros(len(names) + 1, np.int64)
    kp_xy, p_src, p_tgt, p_off, rows = [], [], [], [0], []
    for i, nme in enumerate(names):
        kp = np.asarray(data[nme].keypoints, np.float64).reshape(-1, 2)
        kp_off[i + 1] = kp_off[i] + len(kp)
        kp_xy.append(kp)
        for key, m in data[nme].match_pairs.items():          # dict order = order of first use
            a, b = key.split("-")
            p_src.append(names.index(a)); p_tgt.append(names.index(b))
            rows.append(np.asarray(m, np.int32).reshape(-1, 2))
            p_off.append(p_off[-1] + len(m))
    return dict(kp_off=kp_off, kp_xy=np.concatenate(kp_xy, 0), pair_src=np.asarray(p_src, np.int32), pair_tgt=np.asarray(p_tgt, np.int32),
                pair_off=np.asarray(p_off, np.int64), rows=np.concatenate(rows or [np.zeros((0, 2), np.int32)], 0))


def main():
    state = {}
    ref, mms = load_main_motion_segmentation(state)
    for name, T, H, W, r, seed, sigma, nocc, amp, window, input_size, score_seed in CASES:
        d = psfm_synth.synth_sequence(T, H, W, seed=seed, amp=amp, sigma=sigma, n_occluders=nocc, stride2=False)
        _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
        R = orc.track(d["flows_f"], occ, r)
        keep = np.flatnonzero(R.length >= 3)
        ts = ref_shim.TrajectorySet({int(i): ref_shim.Trajectory({"frame_ids": list(range(int(R.birth[i]), int(R.birth[i]) + int(R.length[i]))),
                                                                   "locations": list(R.traj(int(i))[1]), "labels": [False] * int(R.length[i])})
                                     for i in keep})
        ref.cv2.imread = lambda nme, flag=1, H=H, W=W: np.zeros((H, W, 3), np.uint8) if flag != -1 else np.zeros((H, W), np.float64)
        state.update(input_size=input_size, rng=np.random.default_rng(score_seed), preds=[])
        out = {}
        with tempfile.TemporaryDirectory() as tmp:
            img_dir, depth_dir, traj_dir, out_dir = (os.path.join(tmp, x) for x in ("images", "depths", "traj", "traj_labeled"))
            for p in (img_dir, depth_dir, traj_dir):
                os.makedirs(p)
            names = ["%05d.png" % i for i in range(T)]
            for nme in names:
                open(os.path.join(img_dir, nme), "w").close()
                open(os.path.join(depth_dir, nme), "w").close()
            np.save(os.path.join(traj_dir, "track.npy"), ts, allow_pickle=True)
            # the windows the reference's loop sees (the same load_cut_seq call main_motion_segmentation makes, :62-63)
            cut = mms.load_cut_seq(img_dir, depth_dir, traj_dir, window, input_size, 10 ** 9)
            mms.main_motion_segmentation(img_dir, depth_dir, traj_dir, out_dir, config_file="unused.yaml", window_size=window,
                                         traj_max_num=10 ** 9)
            time_b, idx_b = cut[5], cut[6]
            assert len(state["preds"]) == len(idx_b)
            out["n_windows"] = len(idx_b)
            for w in range(len(idx_b)):
                assert len(idx_b[w]) == len(state["preds"][w])
                out["w%d_ids" % w] = np.asarray(idx_b[w], np.int32)
                out["w%d_pred" % w] = np.asarray(state["preds"][w], np.uint8)
                out["w%d_frame0" % w] = int(time_b[w][0])
                out["w%d_n_frames" % w] = len(time_b[w])
                assert np.array_equal(time_b[w], np.arange(time_b[w][0], time_b[w][0] + len(time_b[w])))
            trajs = np.load(os.path.join(out_dir, "track.npy"), allow_pickle=True).item()
            assert type(trajs) is dict
            keys = list(trajs)
            cnt = [len(trajs[k]["frame_ids"]) for k in keys]
            off = np.zeros(len(keys) + 1, np.int64)
            np.cumsum(cnt, out=off[1:])
            out["ids"] = np.asarray(keys, np.int32)
            out["off"] = off
            out["frame_ids"] = np.concatenate([np.asarray(trajs[k]["frame_ids"], np.int32) for k in keys])
            out["xy"] = np.concatenate([np.asarray(trajs[k]["locations"], np.float64).reshape(-1, 2) for k in keys], 0)
            out["labels"] = np.concatenate([np.asarray(trajs[k]["labels"]).astype(np.uint8) for k in keys])
            for tag, rd in (("rd1_", True), ("rd0_", False)):
                pairs = os.path.join(tmp, "pairs.txt")
                data = ref.traj_to_matches(img_dir, out_dir, pairs, remove_dynamic=rd)
                for k, v in tables_of(data, names).items():
                    out[tag + k] = v
                out[tag + "pair_file_hash"] = hashlib.sha256(open(pairs).read().encode()).hexdigest()
        n_saved, n_saved_pts = len(keep), int(R.length[keep].sum())
        both = sum(1 for i in range(len(keys)) if len(set(out["labels"][off[i]:off[i + 1]].tolist())) == 2)
        if name == CASES[0][0]:       # without these the fixture pins nothing (tests/test_labels_merge.py re-asserts them)
            assert len(keys) < n_saved and int(off[-1]) < n_saved_pts
            assert both >= 1
            assert not np.all(np.diff(out["ids"]) > 0)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, T=T, H=H, W=W, ratio=r, seed=seed, sigma=sigma, n_occluders=nocc, amp=amp, window=window,
                            input_size=np.asarray(input_size), input_hash=input_hash(d), n_saved=n_saved, n_saved_points=n_saved_pts, **out)
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(name, n_saved, "saved trajectories /", n_saved_pts, "points ->", len(keys), "labelled /", int(off[-1]), "points;", both,
              "with both labels; first key", int(out["ids"][0]), "; windows", [int(len(out["w%d_ids" % w])) for w in range(out["n_windows"])],
              "; keypoints", int(out["rd1_kp_off"][-1]), "/", int(out["rd0_kp_off"][-1]), "; longest kept", int(np.diff(off).max()),
              ";", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
