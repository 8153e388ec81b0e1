"""NumPy statement of the motion-boundary option -- the mask of trajectory.py:39-43 and the step with two bilinear verdicts
(trajectory.py:45-62 with the commented kill rule of :60) -- and the names of its fixtures (tests/golden/make_motion_boundary_golden.py).
Pinned to the reference's fixtures by tests/test_motion_boundary_host.py, beside the header the kernels compile."""
import numpy as np

from _common import golden
from _ground_truth_np import fma32

F = np.float32

MASK_FIXTURE = "motion_boundary_masks"
STEP_FIXTURE = "motion_boundary_steps"
# every mask case is a stack (n,H,W,2) with its masks (n,H,W) at the two thresholds
MASK_CASES = ["m2x2", "m2x5", "m5x2", "m3x7", "m37x53", "m48x64", "stack2_3x5", "nonfinite_12x13", "subnormal_6x7", "zeros_6x6"]
MASK_THRES = {"mb002": 0.02, "mb03": 0.3}
SEQ_TRACK = ["mb_track_48x64x8_r2", "mb_track_37x53x6_r1"]
SEQ_OPT = ["mb_opt_48x64x8_r2"]
# the flows of the whole-sequence cases: the layered scene without its error terms (with them 84-91 % of the pixels are boundaries)
SEQ_SYNTH = dict(err_sigma=0.0, outlier_frac=0.0)


def mask_case(name):
    g = golden(MASK_FIXTURE)
    return g[name + "__flow"], {k: g[name + "__" + k] for k in MASK_THRES}


def motion_boundary_np(flow, thres):
    """(H,W,2) f32 -> (H,W) bool: every operation on f32 arrays, one rounding each."""
    f = np.asarray(flow, F)
    H, W = f.shape[:2]
    t = F(thres)
    with np.errstate(all="ignore"):
        dx, dy = np.zeros((H, W, 2), F), np.zeros((H, W, 2), F)
        dx[:, :W - 1] = np.abs(f[:, :W - 1] - f[:, 1:])
        dy[:H - 1] = np.abs(f[:H - 1] - f[1:])
        gx = (dx[..., 0] + dx[..., 1]) * F(0.5)
        gy = (dy[..., 0] + dy[..., 1]) * F(0.5)
        motion = np.sqrt(gx * gx + gy * gy)
        norm = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
        return motion > t * norm


def taps_np(xy, H, W):
    """The sampler's geometry (psfm_taps: true division): x0, y0 (int64) and the four weights nw, ne, sw, se (f32)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x, y = xy[:, 0].astype(F), xy[:, 1].astype(F)
        cw, ch, one = F((W - 1) / 2.0), F((H - 1) / 2.0), F(1.0)
        ix, iy = ((x / cw - one) + one) * cw, ((y / ch - one) + one) * ch
        fx, fy = np.floor(ix), np.floor(iy)
        w = ix - fx; e = one - w
        n = iy - fy; s = one - n
        x0 = np.clip(fx, -2.0, W + 1.0).astype(np.int64)
        y0 = np.clip(fy, -2.0, H + 1.0).astype(np.int64)
    return x0, y0, (s * e, s * w, n * e, n * w)


def sample_np(values, xy):
    """Bilinear sample (zeros padding, align_corners) of an (H,W) map of f32 values at xy (n,2) f64: (n,) f32, the blend of psfm_blend."""
    v = np.asarray(values, F)
    H, W = v.shape
    x0, y0, (nw, ne, sw, se) = taps_np(xy, H, W)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside, v[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F(0.0)).astype(F)
    with np.errstate(all="ignore"):
        return fma32(tap(x0 + 1, y0 + 1), se, fma32(tap(x0, y0 + 1), sw, fma32(tap(x0 + 1, y0), ne, tap(x0, y0) * nw)))


def step_np(xy, flow, occ, mb, rule):
    """One step of every position: next (n,2) f64 and alive (n,) bool.  rule: "mb" (two verdicts), "shipped" (occlusion only),
    "or" (ONE verdict over occ | mb -- what the option is NOT)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    flow = np.asarray(flow, F)
    H, W = flow.shape[:2]
    occ, mb = np.asarray(occ) != 0, np.asarray(mb) != 0
    fs = np.stack([sample_np(flow[..., 0], xy), sample_np(flow[..., 1], xy)], 1)
    nxt = xy + fs.astype(np.float64)
    valid = (nxt[:, 0] > 0) & (nxt[:, 0] < W - 1) & (nxt[:, 1] > 0) & (nxt[:, 1] < H - 1)
    oc = sample_np(occ.astype(F), xy) > F(0.1)
    if rule == "shipped":
        return nxt, valid & ~oc
    if rule == "or":
        return nxt, valid & ~(sample_np((occ | mb).astype(F), xy) > F(0.1))
    assert rule == "mb"
    return nxt, valid & ~oc & ~(sample_np(mb.astype(F), xy) > F(0.1))
