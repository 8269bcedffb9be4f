"""Small scenes, each built to enter named branches of the rasterizer's per-splat pre pass (csrc/render_pre.hip: pre_geom, pre_one,
pre_kernel, pre_multi_kernel, bucket_kernel), shared by test_vertex_model.py (CPU: the model equals the oracle on them and every
scene holds what it was built for) and test_vertex_gpu.py.

A Case is plain data: the arguments of upload_splats, cameras, a frame size and `counts(ev)`, which says per named branch how
many splats of the scene take it (from the model alone); `need` is the least each must reach.  Scenes are made by generating
candidates with fixed seeds and keeping those the model puts into the wanted class, so a seed never has to be lucky.

Frames: 80x48, 65x53, 333x217, 16x16 and, for the rectangle packing, 4096x17 and 17x4096 (256 tiles on one side).  One thing the
kernels cannot do: an axis is capped at 1024 pixels, so no splat spans more than 2049 pixels = 129 tiles; the long frames hold
splats that span 129 tiles from tile 0, up to tile 255 and in between instead of one that covers all 256."""
import functools

import numpy as np

import oracle
import vertex_model as vm
from render_cases import SH_C0

f32 = np.float32
FRAMES = ((80, 48), (65, 53), (333, 217), (16, 16), (4096, 17), (17, 4096))
SMALL_FRAMES = FRAMES[:4]
CULLED = 5                # classes below this index are the five cull comparisons
LARGE_SIZES = (2048 * 256 + 1, 2 * 2048 * 256 + 5)


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def camera(W, H, R=None, p=(0.0, 0.0, 0.0), fx=None, fy=None):
    f = 0.9 * max(W, H)
    return {"fx": float(fx or f), "fy": float(fy or f), "width": int(W), "height": int(H),
            "rotation": np.asarray(np.eye(3) if R is None else R, np.float64).tolist(), "position": [float(v) for v in p]}


def rot_y(th):
    return np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])


def look(d, up=(0.0, 1.0, 0.0)):
    """camera-to-world rotation whose third column (the viewing direction) is d"""
    d = np.asarray(d, np.float64) / np.linalg.norm(d)
    r = np.cross(up, d)
    r = r / np.linalg.norm(r)
    return np.stack([r, np.cross(d, r), d], 1)


def world(cam, pc):
    """camera-space points -> world (view = R^T (x - p), gs.js:81-107)"""
    return np.asarray(pc, np.float64) @ np.asarray(cam["rotation"], np.float64).T + np.asarray(cam["position"], np.float64)


def matrices(cam, W, H):
    view = oracle.view_matrix(cam)
    proj = oracle.proj_matrix(cam["fx"], cam["fy"], W, H)
    return view, proj, oracle.multiply4(proj, view)


def at_ndc(cam, W, H, ndc_x, ndc_y, z):
    """world points that project to GL normalised device coordinates (ndc_x, ndc_y), y up, at camera depth z"""
    x = np.asarray(ndc_x) * z * W / (2 * cam["fx"])
    y = -np.asarray(ndc_y) * z * H / (2 * cam["fy"])
    return world(cam, np.stack([x, y, np.broadcast_to(z, np.shape(x))], 1))


def at_pixel(cam, W, H, u, v, z):
    """world points whose centre lands on image coordinates (u, v) (y down, pixel centres at k + 0.5)"""
    return at_ndc(cam, W, H, 2 * np.asarray(u) / W - 1, 1 - 2 * np.asarray(v) / H, z)


# ---- splats -----------------------------------------------------------------------------------------------------------------
def splats(rng, xyz, log_scale=(-3.5, -2.0), quat=None, alpha=(0.3, 0.95), same_scale=False):
    """attribute arrays for positions xyz: log-scales uniform in log_scale (per axis, or one per splat), random unit quaternions"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = len(xyz)
    s = rng.uniform(log_scale[0], log_scale[1], (m, 1 if same_scale else 3)) * np.ones((1, 3))
    q = rng.normal(size=(m, 4)) if quat is None else np.tile(np.asarray(quat, np.float64), (m, 1))
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    a = rng.uniform(alpha[0], alpha[1], m)
    return [xyz.astype(f32), s.astype(f32), q.astype(f32), np.log(a / (1 - a)).astype(f32),
            ((rng.uniform(0, 1, (m, 3)) - 0.5) / SH_C0).astype(f32)]


def join(parts):
    """[(name, attrs)] -> (attrs, group: name -> source indices)"""
    group, at, out = {}, 0, None
    for name, a in parts:
        m = len(a[0])
        group[name] = np.concatenate([group.get(name, np.zeros(0, np.int64)), np.arange(at, at + m)])
        at += m
        out = a if out is None else [np.concatenate([o, b]) for o, b in zip(out, a)]
    return out, group


def take(a, idx):
    return [x[idx] for x in a]


class Eval:
    """the models on a scene in one view; arrays are per PACKED splat (importance order), src(a) puts one into source order"""

    def __init__(self, attrs, cam, W, H, labels=None, packed=None):
        """packed: (buffer, order, texdata) as the library packed them (Context.render_debug) instead of the oracle's own"""
        self.buf, self.order = oracle.pack_splats(*attrs) if packed is None else packed[:2]
        lab = None if labels is None else np.asarray(labels, np.int32)[self.order]
        self.labels = lab
        self.tex = oracle.texture(self.buf, lab) if packed is None else packed[2]
        self.cam, self.W, self.H = cam, W, H
        self.view, self.proj, self.vp = matrices(cam, W, H)
        self.on(self.tex)

    def on(self, tex):
        """(again) for texel pairs tex: the displaced scene of the label edits; the depth keys stay the buffer's"""
        cam, W, H = self.cam, self.W, self.H
        self.v = vm.vertex(tex, self.view, self.proj, cam["fx"], cam["fy"], W, H)
        self.cls, self.drawn = self.v["cls"], self.v["drawn"]
        self.rect = vm.rect(self.v, W, H)
        self.depth = vm.depth_keys(self.buf, self.vp)
        self.inv = np.empty(len(self.order), np.int64)
        self.inv[self.order] = np.arange(len(self.order))
        return self

    def src(self, a):
        return a[self.inv]


def keep(attrs, cam, W, H, pred, limit):
    """the first `limit` candidates for which pred(Eval) (a mask in source order) holds"""
    ev = Eval(attrs, cam, W, H)
    return take(attrs, np.nonzero(pred(ev))[0][:limit])


class Case:
    def __init__(self, name, attrs, cams, W, H, counts, need, group=None, labels=None, f_rest=None, edits=None, meta=None):
        self.name, self.attrs, self.cams, self.W, self.H = name, attrs, cams, W, H
        self.cam = cams[0]
        self.counts, self.need, self.group = counts, need, group or {}
        self.labels, self.f_rest, self.edits, self.meta = labels, f_rest, edits, meta or {}
        self.n = len(attrs[0])

    @functools.lru_cache(maxsize=None)
    def ev(self, k=0):
        return Eval(self.attrs, self.cams[k], self.W, self.H, self.labels)


def inside_frustum(rng, cam, W, H, m, z=(1.0, 6.0), reach=0.95):
    return at_ndc(cam, W, H, rng.uniform(-reach, reach, m), rng.uniform(-reach, reach, m), rng.uniform(z[0], z[1], m))


# ---- frustum ------------------------------------------------------------------------------------------------------------------
def cull_class(xyz, view, proj):
    """class of bare positions: the five cull comparisons, anything >= CULLED passed them"""
    tex = np.zeros((len(xyz), 8), np.uint32)
    tex[:, :3] = np.asarray(xyz, f32).view(np.uint32)
    return vm.vertex(tex, view, proj, 1.0, 1.0, 1.0, 1.0)["cls"]


def nextafter_pair(view, proj, base, axis, sign, target):
    """walk from `base` along one world axis to the first cull; if it is comparison `target`, bisect down to two positions one
    ulp apart in that coordinate: (kept, culled by `target`), else None"""
    steps = 0.002 * 1.25 ** np.arange(60)
    pts = np.repeat(np.asarray(base, f32)[None], 61, 0)
    pts[1:, axis] += (sign * steps).astype(f32)
    c = cull_class(pts, view, proj)
    out = np.nonzero(c < CULLED)[0]
    if c[0] < CULLED or len(out) == 0 or c[out[0]] != target:
        return None
    lo, hi = pts[out[0] - 1, axis], pts[out[0], axis]

    def cls_at(val):
        p = np.asarray(base, f32).copy()
        p[axis] = val
        return cull_class(p[None], view, proj)[0]

    while np.nextafter(lo, hi) != hi:
        mid = f32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = np.nextafter(lo, hi)
        if cls_at(mid) == target:
            hi = mid
        else:
            lo = mid
    a, b = np.asarray(base, f32).copy(), np.asarray(base, f32).copy()
    a[axis], b[axis] = lo, hi
    return (a, b) if cls_at(lo) >= CULLED and cls_at(hi) == target else None


def frustum(W, H):
    rng = np.random.default_rng(1000 + W)
    cam = camera(W, H, rot_y(0.3), (0.3, -0.2, -1.0), fx=0.9 * max(W, H), fy=0.8 * max(W, H))
    view, proj, _ = matrices(cam, W, H)
    parts, pairs, at = [], [], 0
    # (world axis, direction) whose walk ends in comparison k: z towards the camera, x and y outwards
    walks = {0: (2, -1.0), 1: (0, -1.0), 2: (0, 1.0), 3: (1, 1.0), 4: (1, -1.0)}     # proj[5] < 0: y up is ndc down
    for k, (axis, sign) in walks.items():
        found = []
        while len(found) < 10:
            if k == 0:    # a line along world z that meets the near plane close to the optical axis
                base = world(cam, [[rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004), 0.09]])[0] + np.array([0, 0, rng.uniform(1, 4)])
            else:
                base = inside_frustum(rng, cam, W, H, 1, reach=0.5)[0]
            pr = nextafter_pair(view, proj, base, axis, sign, k)
            if pr is not None:
                found.append(pr)
        xyz = np.array(found).reshape(-1, 3)         # kept, culled, kept, culled ..
        # large enough to reach into the frame from 1.2 of the clip: only a splat with a rectangle shows whether it was culled
        a = splats(rng, xyz, same_scale=True)
        zc = np.maximum((xyz.astype(np.float64) - np.asarray(cam["position"])) @ np.asarray(cam["rotation"])[:, 2], 0.05)
        a[1] = (np.log(0.15 * max(W, H) * zc / cam["fx"])[:, None] * np.ones((1, 3))).astype(f32)
        parts.append((f"pair{k}", a))
        pairs += [(at + 2 * j, at + 2 * j + 1, k, axis) for j in range(len(found))]
        at += len(xyz)
    m = 12
    parts.append(("behind", splats(rng, world(cam, np.stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.uniform(-6, -0.5, m)], 1)))))
    side = np.where(rng.integers(0, 2, 2 * m) == 0, -1.0, 1.0) * rng.uniform(1.04, 1.16, 2 * m)
    other = rng.uniform(-0.8, 0.8, 2 * m)
    ndc = np.where((np.arange(2 * m) % 2 == 0)[:, None], np.stack([side, other], 1), np.stack([other, side], 1))
    parts.append(("margin", splats(rng, at_ndc(cam, W, H, ndc[:, 0], ndc[:, 1], rng.uniform(1, 6, 2 * m)), log_scale=(-5.5, -4.5))))
    parts.append(("inside", splats(rng, inside_frustum(rng, cam, W, H, 40))))
    attrs, group = join(parts)

    def counts(ev):
        c, w = ev.src(ev.cls), ev.src(ev.v["w"])
        cx, cy = ev.src(ev.v["cx"]), ev.src(ev.v["cy"])
        off = (cx < 0) | (cx > W) | (cy < 0) | (cy > H)
        out = {vm.CLASSES[k]: int((c == k).sum()) for k in range(5)}
        out["behind_w_negative"] = int((w[group["behind"]] < 0).sum())
        out["margin_drawn_off_frame"] = int((ev.src(ev.drawn) & off)[group["margin"]].sum())
        out["drawn"] = int(ev.drawn.sum())
        out["pairs_split"] = sum(int(c[a] >= CULLED and c[b] == k) for a, b, k, _ in pairs)
        has = ev.src(ev.rect) != vm.EMPTY_RECT
        out["pairs_kept_side_has_rect"] = sum(int(has[a]) for a, _, _, _ in pairs)
        p2, clip = [ev.src(q) for q in ev.v["p2"]], ev.src(ev.v["clip"])
        lhs, rhs = (p2[2], p2[0], p2[0], p2[1], p2[1]), (-clip, -clip, clip, -clip, clip)
        for k in range(1, 5):      # kept, with a rectangle, and EXACTLY on the boundary: what `>` against `>=` decides
            out[f"exactly_on_{vm.CLASSES[k]}"] = sum(int(has[a] and lhs[k][a] == rhs[k][a]) for a, _, kk, _ in pairs if kk == k)
        return out

    need = dict({vm.CLASSES[k]: 8 for k in range(5)}, behind_w_negative=8, margin_drawn_off_frame=8, drawn=30, pairs_split=len(pairs),
                pairs_kept_side_has_rect=len(pairs), **{f"exactly_on_{vm.CLASSES[k]}": 3 for k in range(1, 5)})
    return Case(f"frustum_{W}x{H}", attrs, [cam], W, H, counts, need, group, meta={"pairs": pairs})


# ---- conics -------------------------------------------------------------------------------------------------------------------
def conics(W, H):
    rng = np.random.default_rng(2000 + W)
    cam = camera(W, H, None, (0.25, -0.15, -0.5))          # identity rotation: c01 == 0 exactly for axis-aligned splats on an axis
    inside = lambda m, **kw: inside_frustum(rng, cam, W, H, m, **kw)
    parts = []
    # needles: one axis stretched by e^6, random orientation; the fp16 truncation leaves some with lambda2 < 0
    cand = splats(rng, inside(1500), log_scale=(-9.0, -5.0))
    cand[1][:, 0] += 6.0
    parts.append(("needle", keep(cand, cam, W, H, lambda ev: ev.src(ev.cls) == vm.CLS["l2_negative"], 16)))
    parts.append(("underflow", splats(rng, inside(40), log_scale=(-40.0, -12.0))))          # 4 Sigma is 0 in fp16 (or what the JS shift leaves)
    parts.append(("overflow", splats(rng, inside(16), log_scale=(5.0, 7.0))))               # .. and infinity
    cand = splats(rng, inside(64, z=(0.3, 1.0)), log_scale=(0.0, 2.0))
    parts.append(("near_large", keep(cand, cam, W, H, lambda ev: ev.src(ev.cls) == vm.CLS["capped"], 16)))
    # identity quaternion, camera x = 0 or y = 0: c01 == 0.  sx == sy: hx == 0 (normalize(0, 0): NaN); sx < sy: drawn; sx > sy: NaN
    for name, sx, sy in (("iso", 1.0, 1.0), ("tall", 0.6, 1.0), ("wide", 1.0, 0.6)):
        m = 10
        z = rng.uniform(1.0, 5.0, m)
        on_x = np.arange(m) % 2 == 0
        pc = np.stack([np.where(on_x, 0.0, rng.uniform(-0.2, 0.2, m) * z), np.where(on_x, rng.uniform(-0.1, 0.1, m) * z, 0.0), z], 1)
        if name == "iso":
            pc[:, :2] = 0.0
        a = splats(rng, world(cam, pc), quat=(1, 0, 0, 0))
        s = np.exp(rng.uniform(-3.5, -2.5, m))
        a[1] = np.log(np.stack([s * sx, s * sy, s], 1)).astype(f32)
        # (the camera position is chosen so that world - p is exact in float32 for these: checked by the counts)
        parts.append((name, a))
    parts.append(("plain", splats(rng, inside(40))))
    attrs, group = join(parts)

    def counts(ev):
        c = ev.src(ev.cls)
        halves = np.stack([vm.half(ev.tex.reshape(-1, 8)[:, 4 + k // 2], k % 2) for k in range(6)], 1)
        zero_cov, inf_cov = ev.src((halves == 0).all(1)), ev.src(np.isinf(halves).any(1))
        c01, hx = ev.src(ev.v["c01"]), ev.src(ev.v["hx"])
        g = group
        return {"l2_negative": int((c == vm.CLS["l2_negative"]).sum()),
                "underflow_degenerate": int((zero_cov & (c == vm.CLS["degenerate"]))[g["underflow"]].sum()),
                "overflow_degenerate": int((inf_cov & (c == vm.CLS["degenerate"]))[g["overflow"]].sum()),
                "capped": int((c == vm.CLS["capped"]).sum()),
                "iso_c01_hx_zero": int(((c01 == 0) & (hx == 0) & (c == vm.CLS["degenerate"]))[g["iso"]].sum()),
                "c01_zero_drawn": int(((c01 == 0) & ev.src(ev.drawn))[g["tall"]].sum()),
                "c01_zero_degenerate": int(((c01 == 0) & (c == vm.CLS["degenerate"]))[g["wide"]].sum()),
                "drawn": int((c == vm.CLS["drawn"]).sum())}

    need = dict(l2_negative=8, underflow_degenerate=8, overflow_degenerate=8, capped=8, iso_c01_hx_zero=8, c01_zero_drawn=8,
                c01_zero_degenerate=8, drawn=30)
    return Case(f"conics_{W}x{H}", attrs, [cam], W, H, counts, need, group)


# ---- pixels -------------------------------------------------------------------------------------------------------------------
def edge_offsets(ev, W, H):
    """per packed splat, float64: how far each side of the box WITHOUT slack lies beyond the pixel centre it would drop first -
    (left, right, top, bottom), positive = that pixel is outside the bare box (and inside it with the slack if < 1/64)"""
    v = ev.v
    ex = np.sqrt(v["major"][:, 0].astype(np.float64) ** 2 + v["minor"][:, 0].astype(np.float64) ** 2)
    ey = np.sqrt(v["major"][:, 1].astype(np.float64) ** 2 + v["minor"][:, 1].astype(np.float64) ** 2)
    cx, top = v["cx"].astype(np.float64), H - v["cy"].astype(np.float64)
    lo = lambda e: e - np.floor(e)              # e = position of the edge in pixel-index units (centre k at k)
    hi = lambda e: np.ceil(e) - e
    return np.stack([lo(cx - ex - 0.5), hi(cx + ex - 0.5), lo(top - ey - 0.5), hi(top + ey - 0.5)], 1)


def pixels(W, H):
    rng = np.random.default_rng(3000 + W)
    cam = camera(W, H)
    f = cam["fx"]
    z = f / 18.0              # a pixel is 1/18 of a world unit at every frame size: fp16 holds the covariances
    px = lambda sigma: np.log(np.asarray(sigma) * z / f)       # log-scale of a sigma given in pixels at depth z
    parts = []
    # tiny splats on pixel corners: drawn, but no pixel centre inside the box
    m = 16
    u, v = rng.integers(1, W, m) + rng.uniform(-0.1, 0.1, m), rng.integers(1, H, m) + rng.uniform(-0.1, 0.1, m)
    a = splats(rng, at_pixel(cam, W, H, u, v, z))
    a[1] = px(rng.uniform(0.02, 0.08, (m, 3))).astype(f32)
    parts.append(("tiny", a))
    # box edges within 1/32 px of the centre of the LAST pixel of a tile (low sides) or the FIRST (high sides): with the
    # slack the box holds that pixel if the edge is less than 1/64 px beyond its centre
    tx, ty = max(1, (W - 1) // 16), max(1, (H - 1) // 16)
    if W > 16 and H > 16:
        m = 28
        for side in range(4):
            a = splats(rng, np.zeros((m, 3)))
            a[1] = px(rng.uniform(1.0, 2.5, (m, 3))).astype(f32)
            bound = 16.0 * rng.integers(1, (tx if side < 2 else ty) + 1, m)     # a tile boundary, in pixels
            want = rng.uniform(-1 / 32, 1 / 32, m)                                # the edge offset to reach
            u = np.where(side < 2, bound, rng.uniform(8, W - 8, m)).astype(np.float64)
            v = np.where(side < 2, rng.uniform(8, H - 8, m), bound).astype(np.float64)
            for _ in range(3):                                                    # the extent moves a little with the centre
                a[0] = at_pixel(cam, W, H, u, v, z).astype(f32)
                ev = Eval(a, cam, W, H)
                vv = ev.v
                ext = ev.src(np.sqrt(vv["major"][:, side // 2].astype(np.float64) ** 2 + vv["minor"][:, side // 2].astype(np.float64) ** 2))
                if side == 0:
                    u = bound - 0.5 + want + ext          # left edge at the centre of pixel bound - 1, + want
                elif side == 1:
                    u = bound + 0.5 - want - ext          # right edge at the centre of pixel bound, - want
                elif side == 2:
                    v = bound - 0.5 + want + ext
                else:
                    v = bound + 0.5 - want - ext
            a[0] = at_pixel(cam, W, H, u, v, z).astype(f32)
            parts.append((f"edge{side}", a))
    # centres outside the frame (between 1.0 and 1.2 of the clip) with boxes that reach in; and boxes that leave it on both sides
    m = 24
    out = rng.uniform(1.02, 1.17, m) * np.where(rng.integers(0, 2, m) == 0, -1.0, 1.0)
    along = rng.uniform(-0.9, 0.9, m)
    horizontal = np.arange(m) % 2 == 0
    a = splats(rng, at_ndc(cam, W, H, np.where(horizontal, out, along), np.where(horizontal, along, out), z), same_scale=True)
    a[1] = (px(np.where(horizontal, W, H) * rng.uniform(0.12, 0.3, m))[:, None] * np.ones((1, 3))).astype(f32)
    parts.append(("reach_in", a))
    m = 12
    a = splats(rng, at_pixel(cam, W, H, rng.uniform(0, W, m), rng.uniform(0, H, m), z), same_scale=True)
    a[1] = (px(np.minimum(max(W, H) * rng.uniform(0.5, 2.0, m), 1500.0))[:, None] * np.ones((1, 3))).astype(f32)
    parts.append(("cover", a))
    # axes at the 1024-pixel cap: 129 tiles of a 4096-pixel side, from tile 0, up to tile 255, in between
    long_x = W >= H
    L = max(W, H)
    pos = np.array([1030.3, L - 1030.6, L / 2 + 7.7, 1035.2, L - 700.9, 0.4 * L, 1500.1, L - 1400.2, 0.3 * L, 0.7 * L])
    mid = np.full(len(pos), (H if long_x else W) / 2.0)
    a = splats(rng, at_pixel(cam, W, H, pos if long_x else mid, mid if long_x else pos, z), same_scale=True)
    a[1] = (px(rng.uniform(400.0, 900.0, len(pos)))[:, None] * np.ones((1, 3))).astype(f32)
    parts.append(("capped", a))
    parts.append(("plain", splats(rng, inside_frustum(rng, cam, W, H, 30), log_scale=(np.log(2.0 * z / f), np.log(6.0 * z / f)))))
    attrs, group = join(parts)

    def counts(ev):
        g = group
        drawn, r = ev.src(ev.drawn), ev.src(ev.rect)
        bare, floored = ev.src(vm.rect(ev.v, W, H, slack=0.0)), ev.src(vm.rect(ev.v, W, H, low=np.floor))
        off = ev.src(edge_offsets(ev, W, H))
        cx, cy = ev.src(ev.v["cx"]), ev.src(ev.v["cy"])
        outside = (cx < 0) | (cx > W) | (cy < 0) | (cy > H)
        t = vm.unpack_rect(r)
        has = r != vm.EMPTY_RECT
        span = np.where(has, np.maximum(t[:, 1] - t[:, 0], t[:, 3] - t[:, 2]) + 1, 0)
        out = {"tiny_drawn_empty": int((drawn & ~has)[g["tiny"]].sum()),
               "reach_in": int((drawn & outside & has)[g["reach_in"]].sum()),
               "both_clamps": int((has & (t[:, 0] == 0) & (t[:, 1] == (W - 1) // 16) & (t[:, 2] == 0) & (t[:, 3] == (H - 1) // 16))[g["cover"]].sum()),
               "floor_low_side_differs": int((floored != r).sum()),
               "rect_tx1_nonzero": int((has & (t[:, 1] > 0)).sum()), "drawn": int(drawn.sum())}
        if "edge0" in g:
            e = np.concatenate([g[f"edge{s}"] for s in range(4)])
            side = np.repeat(np.arange(4), [len(g[f"edge{s}"]) for s in range(4)])
            d = off[e, side]
            out["slack_decides"] = int((bare != r)[e].sum())
            # (a side of 17 pixels has no room for these: the splat that puts an edge on its one tile boundary is culled)
            out["slack_decides_least_per_side"] = min(int((bare != r)[g[f"edge{s}"]].sum()) for s in range(4) if (W, W, H, H)[s] > 40)
            out["edge_inside_anyway"] = int(((d > 1 - 1 / 32) & (bare == r)[e]).sum())      # the edge lies just BEFORE the centre
            out["edge_beyond_slack"] = int(((d > 1 / 64) & (d < 1 / 32) & (bare == r)[e]).sum())
        if max(W, H) == 4096:
            k = (1, 0) if long_x else (3, 2)
            out["capped_129_tiles"] = int((span[g["capped"]] == 129).sum())
            out["tile_255"] = int((has & (t[:, k[0]] == 255)).sum())
            out["low_tile_from_128"] = int((has & (t[:, k[1]] >= 128)).sum())
            out["from_tile_0_over_128"] = int((has & (t[:, k[1]] == 0) & (t[:, k[0]] >= 128)).sum())
        return out

    need = dict(tiny_drawn_empty=8, reach_in=8, both_clamps=8 if max(W, H) < 2048 else 0, floor_low_side_differs=8, rect_tx1_nonzero=8 if W > 16 else 0, drawn=30)
    if W > 16 and H > 16:
        need.update(slack_decides=8, slack_decides_least_per_side=2, edge_inside_anyway=8, edge_beyond_slack=8)
    if max(W, H) == 4096:
        need.update(capped_129_tiles=2, tile_255=2, low_tile_from_128=2, from_tile_0_over_128=2)
    return Case(f"pixels_{W}x{H}", attrs, [cam], W, H, counts, need, group)


# ---- depth --------------------------------------------------------------------------------------------------------------------
def with_first(rng, first_xyz, others, log_scale_first=0.0):
    """scene whose packed splat 0 is the one at first_xyz: by far the largest scale and an opaque alpha (importance order)"""
    a = splats(rng, np.asarray(first_xyz, np.float64).reshape(1, 3), log_scale=(log_scale_first, log_scale_first), alpha=(0.98, 0.99))
    return join([("first", a), ("rest", others)])


def depth_cases():
    W, H = 80, 48
    cam = camera(W, H)
    out = []

    def bucket_counts(extra=None):
        def counts(ev):
            b = vm.buckets(ev.depth, 1, ev.rect)
            c = {"dropped": b["dropped"], "kept": int(b["in_range"].sum()), "first_is_packed_0": int(ev.inv[0] == 0)}
            if extra:
                c.update(extra(ev, b))
            return c
        return counts

    rng = np.random.default_rng(4001)
    z = np.concatenate([rng.uniform(5.3e5, 6.0e6, 12), -rng.uniform(5.3e5, 6.0e6, 12)])
    far = splats(rng, np.stack([rng.uniform(-0.3, 0.3, 24) * np.abs(z), rng.uniform(-0.2, 0.2, 24) * np.abs(z), z], 1), log_scale=(7.0, 9.0))
    attrs, group = join([("far", far), ("plain", splats(rng, inside_frustum(rng, cam, W, H, 40)))])

    def wraps(ev, b):
        pos = ev.buf[:, :12].copy().view(f32).astype(np.float64)
        raw = (ev.vp[2] * pos[:, 0] + ev.vp[6] * pos[:, 1] + ev.vp[10] * pos[:, 2]) * 4096.0
        wrapped = np.abs(raw) > 2.0 ** 31
        return {"keys_wrapped": int(wrapped.sum()), "wrapped_and_kept": int((wrapped & b["in_range"]).sum()),
                "wrapped_sign_flipped": int((wrapped & ((raw > 0) != (ev.depth > 0))).sum())}
    out.append(Case("depth_wrap", attrs, [cam], W, H, bucket_counts(wraps), dict(keys_wrapped=16, wrapped_and_kept=8, wrapped_sign_flipped=4), group))

    rng = np.random.default_rng(4002)
    xyz = at_ndc(cam, W, H, rng.uniform(-0.9, 0.9, 40), rng.uniform(-0.9, 0.9, 40), 3.0)
    attrs, group = join([("plane", splats(rng, xyz))])
    one = lambda ev, b: {"one_key": int(len(np.unique(ev.depth)) == 1), "bucket_0": int((b["bucket"] == 0).sum())}
    out.append(Case("depth_one_plane", attrs, [cam], W, H, bucket_counts(one), dict(one_key=1, bucket_0=40, kept=40), group))

    rng = np.random.default_rng(4003)
    attrs, group = join([("only", splats(rng, at_ndc(cam, W, H, [0.1], [-0.2], 2.5), log_scale=(-2.0, -1.5)))])
    out.append(Case("depth_single", attrs, [cam], W, H, bucket_counts(), dict(kept=1), group))

    first = lambda ev, b: {"first_dropped": int(not b["in_range"][0]), "first_drawn": int(ev.drawn[0]),
                           "first_has_rect": int(ev.rect[0] != vm.EMPTY_RECT), "first_culled": int(ev.cls[0] < CULLED)}
    rng = np.random.default_rng(4004)
    attrs, group = with_first(rng, at_ndc(cam, W, H, [0.2], [0.1], 9.0)[0], splats(rng, inside_frustum(rng, cam, W, H, 60)))
    out.append(Case("depth_first_farthest", attrs, [cam], W, H, bucket_counts(first),
                    dict(first_is_packed_0=1, first_dropped=1, first_drawn=1, first_has_rect=1, dropped=1), group))
    rng = np.random.default_rng(4005)
    attrs, group = with_first(rng, [0.5, 0.3, -2.0], splats(rng, inside_frustum(rng, cam, W, H, 60)))
    out.append(Case("depth_first_culled", attrs, [cam], W, H, bucket_counts(first), dict(first_is_packed_0=1, first_culled=1, dropped=1), group))
    rng = np.random.default_rng(4006)
    attrs, group = with_first(rng, at_ndc(cam, W, H, [-0.3], [0.2], 3.0)[0], splats(rng, inside_frustum(rng, cam, W, H, 60)), -1.0)
    out.append(Case("depth_first_drawn", attrs, [cam], W, H, bucket_counts(first),
                    dict(first_is_packed_0=1, first_drawn=1, first_has_rect=1, dropped=1, kept=60), group))
    # the depth range is reduced over the four waves of a workgroup: the nearest splat in wave w, the farthest in wave 3 - w of a
    # scene of one workgroup (scales fall with the index, so the packed order is the source order)
    for w in range(4):
        rng = np.random.default_rng(4010 + w)
        m = 256
        z = rng.uniform(2.0, 5.0, m)
        near, far = 64 * w + 5, 64 * (3 - w) + 7
        z[near], z[far] = 1.0, 9.0
        a = splats(rng, at_ndc(cam, W, H, rng.uniform(-0.9, 0.9, m), rng.uniform(-0.9, 0.9, m), z), alpha=(0.9, 0.9))
        a[1] = ((-2.0 - 0.004 * np.arange(m))[:, None] * np.ones((1, 3))).astype(f32)
        attrs, group = join([("all", a)])

        def waves(ev, b, w=w):
            return {"packed_in_source_order": int(np.array_equal(ev.order, np.arange(len(ev.order)))),
                    "nearest_in_wave": int(np.argmin(ev.depth) // 64 == w and (ev.depth == ev.depth.min()).sum() == 1),
                    "farthest_in_wave": int(np.argmax(ev.depth) // 64 == 3 - w and (ev.depth == ev.depth.max()).sum() == 1)}
        out.append(Case(f"depth_range_wave{w}", attrs, [cam], W, H, bucket_counts(waves),
                        dict(packed_in_source_order=1, nearest_in_wave=1, farthest_in_wave=1, dropped=1), group))
    return out


# ---- sizes --------------------------------------------------------------------------------------------------------------------
def random_attrs(n, seed):
    """random splats around a rotated camera: a tenth with log-scales in -40..-12, a tenth with one axis stretched by e^6"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-6, 6, (n, 3)).astype(f32)
    scale = rng.uniform(-9, 1.5, (n, 3)).astype(f32)
    scale[:n // 10] = rng.uniform(-40, -12, (n // 10, 3))
    scale[n // 10:n // 5, 0] += 6
    return [xyz, scale, rng.normal(size=(n, 4)).astype(f32), rng.normal(size=n).astype(f32), rng.normal(size=(n, 3)).astype(f32)]


def size_case(n):
    W, H = 65, 53
    cam = camera(W, H, rot_y(0.3), (0.3, -0.2, -1.0), fx=70.0, fy=64.0)
    counts = lambda ev: {"n": len(ev.order), "drawn": int(ev.drawn.sum())}
    return Case(f"size_{n}", random_attrs(n, 5000 + n % 1000), [cam], W, H, counts, dict(n=n, drawn=1 if n > 1000 else 0))


# ---- views --------------------------------------------------------------------------------------------------------------------
def views():
    W, H = 80, 48
    rng = np.random.default_rng(6000)
    n = 1500
    d = rng.normal(size=(n, 3))
    xyz = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 4.0, (n, 1))
    attrs = splats(rng, xyz, log_scale=(-4.0, -2.0))
    dirs = [(1, 0.1, 0.2), (-1, 0.2, -0.1), (0.2, 1, 0.3), (0.1, -1, 0.4), (0.3, 0.2, 1), (-0.2, 0.1, -1)]
    cams = [camera(W, H, look(dd, up=(0, 1, 0) if abs(dd[1]) < 0.9 else (1, 0, 0)), 0.3 * np.asarray(dd, np.float64), fx=70.0 + 3 * k, fy=66.0 - 2 * k)
            for k, dd in enumerate(dirs)]
    labels = rng.integers(0, 12, n).astype(np.int32)
    labels[rng.integers(0, n, 40)] = 2 ** 24 + 3           # rounds to 2^24 + 4 in the texture: the shaders' label differs from the exact one
    labels[rng.integers(0, n, 40)] = -999999
    f_rest = rng.normal(0, 0.25, (n, 45)).astype(f32)
    edits = dict(selected=3, selection_mode=True, colours={5: (0.1, 0.9, 0.2), 2 ** 24 + 4: (0.9, 0.8, 0.1), 7: (0.3, 0.3, 1.0)},
                 custom_colour=(0.25, 0.5, 0.75), displacements={1: (0.4, -0.3, 0.2), 6: (-2.5, 0.0, 1.5), 3: (0.0, 0.05, 0.0)},
                 hidden=(4, 7, 2 ** 24 + 3))

    def counts(ev0):
        want = np.stack([case.ev(k).rect != vm.EMPTY_RECT for k in range(len(cams))], 1)
        k = want.sum(1)
        return {"mixed_want": int(((k > 0) & (k < len(cams))).sum()), "no_view": int((k == 0).sum()), "every_view_draws": int(want.any(0).sum()),
                "least_drawn_per_view": int(want.sum(0).min())}

    case = Case("views", attrs, cams, W, H, counts, dict(mixed_want=n // 10, no_view=n // 100, every_view_draws=6, least_drawn_per_view=30),
                labels=labels, f_rest=f_rest, edits=edits)
    return case


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> Case: everything but the two large sizes (size_case(n) for n in LARGE_SIZES: made on demand)"""
    cases = [frustum(W, H) for W, H in SMALL_FRAMES[:3]] + [conics(W, H) for W, H in SMALL_FRAMES[:3]]
    cases += [pixels(W, H) for W, H in FRAMES] + depth_cases() + [size_case(n) for n in (1, 255, 256, 257)] + [views()]
    return {c.name: c for c in cases}


# ---- the colour path ----------------------------------------------------------------------------------------------------------
def sh_rgb(case, ev, degree, cam):
    """oracle.sh_colors on the packed splats: (n, 3) float32, not yet faded"""
    order = ev.order
    k1 = (degree + 1) ** 2 - 1
    rest = case.f_rest[order].reshape(len(order), 3, 15)[:, :, :k1].reshape(len(order), 3 * k1)   # 3DGS PLY order: f_rest[c * K1 + k - 1]
    xyz = ev.buf[:, :12].copy().view(f32)
    return oracle.sh_colors(xyz, case.attrs[4][order], rest, degree, cam["position"])[:, :3]


def f_rest_for(case, degree):
    """the f_rest argument of upload_sh for a lower degree, cut from the scene's degree-3 coefficients"""
    k1 = (degree + 1) ** 2 - 1
    return np.ascontiguousarray(case.f_rest.reshape(case.n, 3, 15)[:, :, :k1].reshape(case.n, 3 * k1))


def edited(case, ev, k, sh_degree=None, edits=False):
    """What the pre kernels store for view k of `case` under an SH degree and / or the case's edit state: (Eval of the geometry
    the shader sees - the displaced scene with edits - and the records (n, 12) float32).  Colour: fade * rgba8 / 255, or
    fade * oracle.sh_colors (direction from the UNDISPLACED centre); then render_edits_ref's fragment-shader edits; a hidden
    splat's alpha is fade * 0 / 255."""
    import render_edits_ref as ref
    cam, n = case.cams[k], case.n
    tex = ev.tex.reshape(n, 8)
    geo = ev
    if edits:
        st = ref.state(**case.edits)
        vlabel = ref.shader_labels(ev.labels)
        slot = ref.first_match(vlabel, st["displacements"].keys())
        table = np.array([np.asarray(d, f32).reshape(3) for d in st["displacements"].values()], f32)
        d = np.zeros((n, 3), f32)
        d[slot >= 0] = table[slot[slot >= 0]]
        moved = tex.copy()
        moved[:, :3] = (tex[:, :3].copy().view(f32) + d).view(np.uint32)
        geo = Eval(None, cam, case.W, case.H, packed=(ev.buf, ev.order, moved))
        geo.labels = ev.labels
    v = geo.v
    with np.errstate(all="ignore"):
        rgb = v["color"][:, :3] if sh_degree is None else v["fade"][:, None] * sh_rgb(case, ev, sh_degree, cam)
        alpha = None
        if edits:
            rgb, _ = ref.edited_colours(rgb, vlabel, st)
            hidden = np.isin(ev.labels, [h for h in st["hidden"] if h != ref.NO_SELECTION])
            alpha = np.where(hidden, v["fade"] * f32(0.0) / f32(255.0), v["color"][:, 3])
    return geo, vm.record(v, geo.rect, rgb, alpha)
