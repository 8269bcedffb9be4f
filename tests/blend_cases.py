"""Scenes placed on the structural edges of the blend kernels (csrc/blend.hip), shared by test_blend_model.py (CPU: the cases
are what they claim) and test_blend_gpu.py.  All use render_cases.cam_identity; frames are under 100 pixels a side (96x48 at
the most), scenes hold at most 7313 splats.  A Scene is plain data: the arguments of upload_splats / oracle.render_scene plus `meta`."""
import functools

import numpy as np

import blend_model
import oracle
from render_cases import SH_C0, cam_identity

TILE = 16
LENGTHS = (0, 1, 256, 128, 17, 319,            # by tile, row-major; the 32x32 bin of tiles (0,0) (1,0) (0,1) (1,1) holds 0 / 1 / 513 / 257
           513, 257, 15, 64, 129, 320,
           16, 63, 65, 127, 255, 321)
WALL_M = (0, 12, 13, 16, 28, 29, 45, 60, 61, 64, 125, 252, 253, 256)
N_LOUD = 300


class Scene:
    def __init__(self, name, W, H):
        self.name, self.W, self.H = name, W, H
        self.cam = cam_identity(W, H)
        self.f = self.cam["fx"]
        self.xyz, self.scale, self.rot, self.opacity, self.f_dc = [], [], [], [], []
        self.meta = {}

    def add(self, u, v, z, sigma_px, quat, alpha8, rgb8):
        """a splat whose centre projects to pixel coordinates (u, v) (image, y down) at depth z; sigma_px: 3 pixel sigmas;
        alpha8, rgb8: the stored bytes.  -> index in upload order"""
        f, W, H = self.f, self.W, self.H
        self.xyz.append(((u - W / 2) * z / f, (v - H / 2) * z / f, z))
        self.scale.append([float(np.log(s * z / f)) for s in sigma_px])
        self.rot.append([float(c) for c in quat])
        p = alpha8 / 255.0                                                   # the logit lands on alpha8 / 255 when stored in 8 bits
        self.opacity.append(float(np.log(p / (1 - p))) if alpha8 < 255 else 30.0)      # sigmoid(30) * 255 rounds to 255
        self.f_dc.append([(c / 255.0 - 0.5) / SH_C0 for c in rgb8])
        return len(self.xyz) - 1

    def arrays(self):
        return (np.asarray(self.xyz, np.float32), np.asarray(self.scale, np.float32), np.asarray(self.rot, np.float32),
                np.asarray(self.opacity, np.float32), np.asarray(self.f_dc, np.float32))

    def args(self):
        return self.arrays() + (self.cam, self.W, self.H)


def unit_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def tile_spot(tx, ty, W, H):
    """Where an in-tile splat of tile (tx, ty) goes: (u, v, sigma_px, centre jitter, scale jitter).  A whole tile: its centre,
    sigma 1.5, +-1 px, scales x0.8..1.2 - the fragment box stays within pixels 2..13.  A tile the frame cuts: sigma 0.45, scales
    x0.95..1.05 (reach 1.21..1.34 px), centred on the visible part or - where that is under 5 pixels wide - 1.3 px into the
    tile, so that the box holds the tile's first pixel column / row and sticks out of the frame, never into the neighbour."""
    w, h = min(TILE, W - tx * TILE), min(TILE, H - ty * TILE)
    if w == TILE and h == TILE:
        return tx * TILE + 8.0, ty * TILE + 8.0, 1.5, 1.0, (0.8, 1.2)
    u = tx * TILE + (8.0 if w == TILE else w / 2 if w >= 5 else 1.3)
    v = ty * TILE + (8.0 if h == TILE else h / 2 if h >= 5 else 1.3)
    return u, v, 0.45, 0.1, (0.95, 1.05)


def add_in_tile(sc, rng, tx, ty, count, z_lo, z_hi, alpha8, rgb=None):
    """`count` splats that stay inside tile (tx, ty): scales jittered per axis, random unit quaternions"""
    u0, v0, sigma, jit, (lo, hi) = tile_spot(tx, ty, sc.W, sc.H)
    out = []
    for _ in range(count):
        a = alpha8(rng) if callable(alpha8) else alpha8
        col = rgb(rng) if callable(rgb) else (rgb if rgb is not None else rng.integers(0, 256, 3))
        out.append(sc.add(u0 + rng.uniform(-jit, jit), v0 + rng.uniform(-jit, jit), rng.uniform(z_lo, z_hi),
                          sigma * rng.uniform(lo, hi, 3), unit_quat(rng), a, col))
    return out


def add_sink(sc, count=1):
    """`count` splats at one depth behind everything else: runSort drops the farthest bucket (65536) and draws splat 0 once more
    for each.  (max - min) * (65536 / (max - min)) can round to just under 65536, in which case the farthest splats are kept:
    the depth is moved until the oracle's runSort drops exactly `count`.  Call last."""
    ids = [sc.add(8.0 + k, 8.0, 6.0, (0.3, 0.3, 0.3), (0.9, 0.1, 0.3, 0.2), 3, (9, 9, 9)) for k in range(count)]
    proj = oracle.proj_matrix(sc.cam["fx"], sc.cam["fy"], sc.W, sc.H)
    vp = oracle.multiply4(proj, oracle.view_matrix(sc.cam))
    for step in range(64):
        z = 6.0 + 0.0137 * step
        for k, i in enumerate(ids):
            sc.xyz[i] = ((8.0 + k - sc.W / 2) * z / sc.f, (8.0 - sc.H / 2) * z / sc.f, z)
        buf, _ = oracle.pack_splats(*sc.arrays())
        if oracle.depth_order(buf, vp)[1] == count:
            return ids
    raise AssertionError("no depth at which runSort drops the sinks")


def lengths():
    """6x3 tiles, tile j holds a list of exactly LENGTHS[j] faint in-tile records: the vote distance (16), the chunks of 64 and
    256, the 256-entry BIN32 fetch and that fetch plus a carried remainder.  alpha 1/255..4/255, at most what keeps the sum of
    a list's alphas near 2: no tile comes near opacity and the last record of the longest list still moves a pixel by > 1e-4."""
    rng = np.random.default_rng(20261)
    sc = Scene("lengths", 96, 48)
    for j, L in enumerate(LENGTHS):
        top = int(np.clip(2.0 * 255 / (0.9 * max(L, 1)), 1, 4))
        add_in_tile(sc, rng, j % 6, j // 6, L, 3.0, 5.0, lambda r, top=top: int(r.integers(1, top + 1)))
    add_sink(sc)
    sc.meta["lengths"] = LENGTHS
    return sc


def needles():
    """the same grid; elongated (axis ratio 10), rotated splats that span several tiles: the bounding-box lists hold many
    (tile, record) pairs without a fragment, and some needles graze a tile's corner pixels near q = 4"""
    rng = np.random.default_rng(20262)
    sc = Scene("needles", 96, 48)
    for _ in range(220):
        t = rng.uniform(0, np.pi)
        q = np.array([np.cos(t / 2), rng.normal() * 0.03, rng.normal() * 0.03, np.sin(t / 2)])
        s = rng.uniform(8.0, 13.0)
        sc.add(rng.uniform(-4, 100), rng.uniform(-4, 52), rng.uniform(3.0, 5.0), (s, s / 10, s / 10), q / np.linalg.norm(q),
               int(rng.integers(16, 49)), rng.integers(0, 256, 3))
    add_sink(sc)
    return sc


def walls(W=80, H=48):
    """Tile j: m_j faint in-tile records, then three frame-filling opaque splats (axes capped at 1024 px) shared by all tiles,
    then 300 loud in-tile records (alpha 255, saturated colours) nobody may show.  m_j mod 16 <= 13: the three walls fall into
    one vote group.  One tile has a HOLE: opaque in-tile discs that leave its corner pixels open stand where the walls stand
    elsewhere, its loud records sit on the corner pixels IN FRONT of the shared walls - the corners must show them.
    Two things differ from a literal "walls replaced" tile, and the GPU test relies on both.  A frame-filling wall covers the
    holed tile too, so there the shared walls come LAST (behind the loud records) instead of being absent.  And a loud record
    that stays inside the tile puts B ~ 0.1 on a corner pixel: 75 per corner leave 1 - dst.a ~ 1e-3..1e-1 there, so the tile
    does not turn opaque by its loud records - it walks its WHOLE list, to the shared walls (test_blend_model.py asserts that
    this count is decided: no vote on the way comes within 5e-6 of the limit).
    The grid is 5x3 (80x48), not the 6x3 of the other families, and the cut frame 65x53: with the axes capped at 1024 px a wall
    leaves 1 - B = 4 d^2 / 1024^2 at distance d from its centre, and three of them pass 1 - 1e-6 only within 51 px.
    A frame-filling wall closes the out-of-frame pixels of a cut tile as well - the kernels blend those lanes like any other -
    so behind walls a vote that forgot `!in ||` would pass all the same.  The tiles of the CUT COLUMN of 65x53 (one pixel
    column in the frame) are therefore closed differently: three opaque vertical needles on that column stand where the walls
    stand elsewhere and touch no other column, the loud records follow, the shared walls come last.  The tile's far
    columns, outside the frame, stay at alpha 0 until the end of the list: only a vote that skips them stops after the needles."""
    rng = np.random.default_rng(20263 + W)
    sc = Scene(f"walls_{W}x{H}", W, H)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    ntiles = tiles_x * tiles_y
    hole = ntiles - tiles_x - 2 if W % 16 == 0 else tiles_x + 1       # a whole tile
    ms = {}
    others = [t for t in range(ntiles) if t != hole]
    for k, t in enumerate(others):
        ms[t] = WALL_M[k % len(WALL_M)]
    ms[hole] = 20
    sat = lambda r: [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255)][int(r.integers(0, 6))]
    tags = {}
    cut = [t for t in range(ntiles) if W % 16 and t % tiles_x == tiles_x - 1]     # the column of tiles the right border cuts
    closers = []
    if cut:
        # 65 = 4 * 16 + 1: one pixel column of these tiles is in the frame.  Three opaque vertical needles on that column
        # (long axis at the 1024-px cap: q < 0.003 along the column; short axis 0.3 px: no pixel centre but the column's)
        # close it and leave the other fifteen columns of the tile untouched.
        closers = [sc.add(W - 0.5 + 0.01 * (k - 1), H / 2 + 0.3 * k, 3.5 + 0.01 * k, (0.3, 30.0 * sc.f / 4.0, 0.01), (1, 0, 0, 0), 255,
                          (200, 120, 30)) for k in range(3)]
    for t in range(ntiles):
        tx, ty = t % tiles_x, t // tiles_x
        if t in cut:
            faint = add_in_tile(sc, rng, tx, ty, ms[t], 3.0, 3.4, lambda r: int(r.integers(1, 5)))
            loud = add_in_tile(sc, rng, tx, ty, N_LOUD, 3.6, 3.9, 255, sat)
            discs = closers
        elif t == hole:
            faint = add_in_tile(sc, rng, tx, ty, ms[t], 3.0, 3.4, lambda r: int(r.integers(1, 5)))
            discs = [sc.add(tx * 16 + 8 + rng.uniform(-0.3, 0.3), ty * 16 + 8 + rng.uniform(-0.3, 0.3), 3.5 + 0.01 * k,
                            2.6 * rng.uniform(0.95, 1.05, 3), unit_quat(rng), 255, (40, 40, 40)) for k in range(3)]
            loud = []
            for k in range(N_LOUD):
                cxo, cyo = (1.1, 14.9)[k & 1], (1.1, 14.9)[(k >> 1) & 1]
                loud.append(sc.add(tx * 16 + cxo + rng.uniform(-0.15, 0.15), ty * 16 + cyo + rng.uniform(-0.15, 0.15),
                                   rng.uniform(3.6, 3.9), 0.4 * rng.uniform(0.9, 1.1, 3), unit_quat(rng), 255, sat(rng)))
        else:
            faint = add_in_tile(sc, rng, tx, ty, ms[t], 3.0, 3.9, lambda r: int(r.integers(1, 5)))
            loud = add_in_tile(sc, rng, tx, ty, N_LOUD, 4.1, 5.0, 255, sat)
            discs = []
        tags[t] = (faint, discs, loud)
    wall_ids = [sc.add(W / 2 + 0.6 + 0.3 * k, H / 2 + 0.5 - 0.2 * k, 4.0 + 0.01 * k, (30.0 * sc.f / 4.0,) * 3, (1, 0, 0, 0), 255,
                       (200, 120, 30)) for k in range(3)]
    add_sink(sc)
    sc.meta.update(m=ms, hole=hole, cut=cut, tags=tags, walls=wall_ids)
    return sc


EDGE_FRAMES = ((33, 33), (47, 36), (48, 37), (33, 40), (47, 41), (48, 44), (33, 45), (47, 47), (17, 17), (31, 17))


def edges(W, H):
    """a frame whose right / bottom border cuts tiles (W % 16 in {1, 15, 0}, H % 16 in {1, 4, 5, 8, 9, 12, 13, 15}): medium-alpha
    splats straddle the right and bottom borders and the tile rows and columns the frame cuts"""
    rng = np.random.default_rng(20264 + 100 * W + H)
    sc = Scene(f"edges_{W}x{H}", W, H)
    cut_x, cut_y = (W - 1) // 16 * 16, (H - 1) // 16 * 16
    for k in range(36):
        where = k % 4
        u = (W - 0.5 + rng.uniform(-3, 3)) if where == 0 else cut_x + rng.uniform(-2, W - cut_x + 1) if where == 2 else rng.uniform(0, W)
        v = (H - 0.5 + rng.uniform(-3, 3)) if where == 1 else cut_y + rng.uniform(-2, H - cut_y + 1) if where == 3 else rng.uniform(0, H)
        sc.add(u, v, rng.uniform(3.0, 5.0), rng.uniform(1.2, 3.5, 3), unit_quat(rng), int(rng.integers(40, 101)),
               rng.integers(0, 256, 3))
    add_sink(sc)
    return sc


def epilogue(k, opaque=False):
    """k splats share the farthest depth exactly: runSort drops them and splat 0 is drawn k more times, last.  Splat 0 (largest
    scale^3 * opacity, not opaque) spans tiles 1..3 x 0..1 of 6x3; tiles (3,0) and (3,1) inside its rectangle hold no other
    record; tiles 0, 4, 5 of every row lie outside it.  opaque=True adds two stacks of wide opaque splats in front - on tile (1,0)
    inside the rectangle and on tile (5,2) outside - that close those tiles within the nearest sixth of the splats, i.e. before
    the last depth phase, and faint records behind them."""
    rng = np.random.default_rng(20265 + k + 10 * opaque)
    sc = Scene(f"epilogue_{k}" + ("_opaque" if opaque else ""), 96, 48)
    zero = sc.add(40.0, 16.0, 2.6, (8.0, 5.0, 25.0), (0.98, 0.02, 0.03, 0.2), 100, (250, 180, 60))
    faint = lambda r: int(r.integers(2, 7))
    for tx, ty, cnt in ((0, 0, 60), (2, 1, 90), (4, 0, 120), (1, 1, 40), (5, 1, 30), (2, 2, 70), (1, 0, 25), (5, 2, 25)):
        add_in_tile(sc, rng, tx, ty, cnt, 3.2, 5.0, faint)
    if opaque:
        for u, v in ((24.0, 8.0), (88.0, 40.0)):
            for _ in range(40):
                sc.add(u + rng.uniform(-0.5, 0.5), v + rng.uniform(-0.5, 0.5), rng.uniform(2.0, 2.2), 7.0 * rng.uniform(0.95, 1.05, 3),
                       unit_quat(rng), 255, rng.integers(0, 256, 3))
    add_sink(sc, count=k)
    sc.meta.update(zero=zero, k=k, opaque=opaque, rect=(1, 3, 0, 1), bare=(3, 9), closed=(1, 17) if opaque else ())
    return sc


def all_cases():
    """name -> builder; `bitwise`: no tile reaches the opacity cut, every kernel and option must give the same bits"""
    cases = {"lengths": lengths, "needles": needles, "walls_80x48": walls, "walls_65x53": lambda: walls(65, 53)}
    for W, H in EDGE_FRAMES:
        cases[f"edges_{W}x{H}"] = lambda W=W, H=H: edges(W, H)
    cases["epilogue_1"] = lambda: epilogue(1)
    cases["epilogue_3"] = lambda: epilogue(3)
    cases["epilogue_3_opaque"] = lambda: epilogue(3, opaque=True)
    return cases


def family(name):
    return name.split("_")[0]


def bitwise(name):
    return family(name) in ("lengths", "needles", "edges") or (family(name) == "epilogue" and not name.endswith("opaque"))


# ---- one model and one oracle frame per case, shared by every test of a session --------------------------------------------
class Prepared:
    """scene, fp64 model, the oracle's frame, ref_dist = max |oracle - model| outside the threshold mask, and the GPU tolerance
    tol = min(8 * ref_dist, 1e-5): the oracle is itself an fp32 evaluation of the model, so its distance measures what fp32
    costs on this very scene; the factor 8 covers __expf against libm's expf (an exp2 of a rounded product: several ulp at
    A = -4); 1e-5 is the kernels' own documented cut and caps it."""

    def __init__(self, name):
        self.name = name
        self.scene = sc = all_cases()[name]()
        self.model = m = blend_model.BlendModel(*sc.args())
        self.ref = oracle.render_scene(*sc.args()).astype(np.float64)
        self.diff = np.abs(self.ref - m.frame).max(axis=2)
        self.ref_dist = float(self.diff[~m.mask].max())
        self.tol = min(8.0 * self.ref_dist, 1.0e-5)
        self.alpha_max = float(m.rec.color[m.rec.drawn, 3].max())
        self.packed = np.argsort(m.rec.order)          # upload index -> packed (importance order) index


prepared = functools.lru_cache(maxsize=None)(Prepared)
