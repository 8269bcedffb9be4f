"""Case builders shared by the CPU and GPU tests of the instance association (tests/assoc_model.py is the rule)."""
import numpy as np

from conftest import cam_dict

# ---- the value scene: K separated blobs seen by V cameras, every view numbering the blobs its own way ---------------------------------
K, V, PER_BLOB = 6, 5, 80
W, H, F = 160, 120, 100.0
DISC = 10                      # pixels: a blob of radius 0.3 at depth >= 4.5 projects within 6.7 pixels of its centre


def _yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def value_scene():
    """-> positions (n, 3) f32, blob (n,) int, cams, maps (int32, segment ids permuted per view), sizes.  View 2 sees only the
    blobs of the two left columns."""
    rng = np.random.default_rng(6105)
    centres = np.array([[x, y, 5.0] for y in (-1.0, 1.0) for x in (-2.0, 0.0, 2.0)])
    d = rng.normal(size=(K * PER_BLOB, 3))
    d *= (0.3 * rng.uniform(0, 1, (len(d), 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    blob = np.repeat(np.arange(K), PER_BLOB)
    pos = (centres[blob] + d).astype(np.float32)
    poses = [((0.0, 0.0, 0.0), 0.0), ((0.4, -0.2, 0.1), 0.04), ((-2.6, 0.0, 0.0), 0.0), ((-0.5, 0.3, -0.2), -0.05), ((0.2, 0.1, 0.3), 0.02)]
    cams, maps = [], []
    for v, (p, a) in enumerate(poses):
        R = _yaw(a)
        cams.append(cam_dict(F, F, (W, H), R, p, f"value{v}"))
        perm = rng.permutation(K)
        seg = np.full((H, W), -1, np.int32)
        r, c = np.mgrid[0:H, 0:W]
        for k in range(K):
            pc = R @ (centres[k] - np.array(p))
            cx, cy = F * pc[0] / pc[2] + W / 2, F * pc[1] / pc[2] + H / 2
            seg[(c + 0.5 - cx) ** 2 + (r + 0.5 - cy) ** 2 <= DISC ** 2] = perm[k]
        maps.append(seg)
    return pos, blob, cams, maps, [(W, H)] * V


# ---- small scenes on a 40 x 24 frame ---------------------------------------------------------------------------------------------------
MW, MH, MF = 40, 24, 30.0


def small_cam(p=(0.0, 0.0, 0.0), yaw=0.0, name="small"):
    return cam_dict(MF, MF, (MW, MH), _yaw(yaw), p, name)


AWAY = small_cam((0.0, 0.0, 100.0), name="away")        # every Gaussian is behind it


def small_positions(n, seed):
    """a cloud that overflows the frame of small_cam() on every side: about half of it is visible"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(3, 6, n)], axis=1).astype(np.float32)


def block_map(n_segments, seed, w=MW, h=MH, background=True):
    """blocks of 8 x 6 pixels with segment ids drawn per block from [-1 or 0, n_segments)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1 if background else 0, n_segments, ((h + 5) // 6, (w + 7) // 8))
    return np.repeat(np.repeat(ids, 6, axis=0), 8, axis=1)[:h, :w].astype(np.int32)


def small_views(n_views, n_segments, seed, w=MW, h=MH):
    rng = np.random.default_rng(seed)
    cams = [small_cam((rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)), rng.uniform(-0.05, 0.05), f"small{v}")
            for v in range(n_views)]
    return cams, [block_map(n_segments, seed + 1 + v, w, h) for v in range(n_views)]


def grid_positions():
    """128 Gaussians, one per pixel centre of a 16 x 8 grid of the 40 x 24 frame of small_cam(), all at depth 4: after the
    upload's Morton order two whole waves, each Gaussian alone on its pixel - a map can give every lane any key"""
    gx, gy = np.meshgrid(np.arange(16), np.arange(8))
    px, py = 2 * gx.reshape(-1) + 4.5, 2 * gy.reshape(-1) + 4.5
    z = 4.0
    return np.stack([(px - MW / 2) * z / MF, (py - MH / 2) * z / MF, np.full(128, z)], axis=1).astype(np.float32)


def paint(x, y, order, values):
    """the 40 x 24 map, -1 except under the Gaussians order[s], which get values[s]"""
    seg = np.full((MH, MW), -1, np.int32)
    seg[y[order], x[order]] = values
    return seg
