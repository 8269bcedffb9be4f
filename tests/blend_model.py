"""fp64 model of the fragment + blend stage (csrc/blend.hip), plain numpy, no GPU code.

Inputs are what the oracle exposes: the float32 vertex outputs of oracle.vertex per splat and the draw order of
oracle.pack_splats / texture / depth_order, walked as gsxo_render_view walks it - all n slots of depth_index, the slots runSort
leaves at 0 included (that walk is what draws splat 0 again once per dropped splat).  Per pixel, in fp64:

    d = (x + 0.5 - cx, H - (r + 0.5) - cy);  v = (d.g0, d.g1);  q = |v|^2;  fragment iff q <= 4;  B = exp(-q) * color[3]
    dst += (1 - dst.a) * (B * rgb, B), front to back

The frame is evaluated tile by tile over the list a bounding-box binner holds for the tile (the records whose fragment box
meets it, in draw order) followed by the epilogue's draws of splat 0; test_blend_model.py pins it to oracle.render_scene, which
has a bounding box of its own.  With T_k = prod_{j<k} (1 - B_j) the pixel is sum_k T_k s_k (s_k = (B_k rgb_k, B_k)), so removing
record m changes it by T_m (s_m - B_m R_m), R_m = the blend of everything behind m at full transmittance: leave-one-out in
closed form from a prefix product and a suffix recursion, no second render."""
import numpy as np

import oracle
import vertex_model

TILE = 16
NEAR = 1e-4          # |q - 4| below which fp32 and fp64 may decide `discard` differently
E4 = float(np.exp(-4.0))


class Records:
    """Per packed splat (importance order): the vertex shader's outputs and the binner's pixel box."""

    def __init__(self, xyz, scale, rot, opacity, f_dc, cam, W, H):
        self.W, self.H = W, H
        self.tiles_x, self.tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        buf, self.order = oracle.pack_splats(xyz, scale, rot, opacity, f_dc)
        tex = oracle.texture(buf)
        view = oracle.view_matrix(cam)
        proj = oracle.proj_matrix(cam["fx"], cam["fy"], W, H)
        self.depth_index, self.dropped = oracle.depth_order(buf, oracle.multiply4(proj, view))
        n = self.n = len(buf)
        self.drawn = np.zeros(n, bool)
        self.c = np.zeros((n, 2), np.float32)
        self.g0 = np.zeros((n, 2), np.float32)
        self.g1 = np.zeros((n, 2), np.float32)
        self.major = np.zeros((n, 2), np.float32)
        self.minor = np.zeros((n, 2), np.float32)
        self.color = np.zeros((n, 4), np.float32)
        for i in range(n):
            o = oracle.vertex(tex[8 * i:8 * i + 8], view, proj, cam["fx"], cam["fy"], W, H)
            self.drawn[i] = bool(o.drawn)
            if o.drawn:
                self.c[i] = o.cx, o.cy
                self.g0[i], self.g1[i] = tuple(o.g0), tuple(o.g1)
                self.major[i], self.minor[i] = tuple(o.major), tuple(o.minor)
                self.color[i] = tuple(o.color)
        self.box = self._boxes()

    def _boxes(self):
        """(x0, x1, r0, r1) inclusive per splat, x1 < x0 where it reaches no pixel centre: vertex_model.pixel_box, the binner's
        box on the vertex shader's float32 outputs"""
        return vertex_model.pixel_box(self.c[:, 0], self.c[:, 1], self.major, self.minor, self.drawn, self.W, self.H)


class BlendModel:
    def __init__(self, xyz, scale, rot, opacity, f_dc, cam, W, H):
        R = self.rec = Records(xyz, scale, rot, opacity, f_dc, cam, W, H)
        self.W, self.H, self.tiles_x, self.tiles_y = W, H, R.tiles_x, R.tiles_y
        n, nd = R.n, R.dropped
        # gsxo_render_view's walk: the first n - nd slots are the kept splats front to back, the rest stayed 0
        self.walk = R.depth_index.astype(np.int64)
        assert (self.walk[n - nd:] == 0).all()
        self.n_epilogue = nd
        self.lists = [[] for _ in range(self.tiles_x * self.tiles_y)]
        for i in self.walk[:n - nd]:
            x0, x1, r0, r1 = R.box[i]
            if x1 < x0:
                continue
            for ty in range(r0 // TILE, r1 // TILE + 1):
                for tx in range(x0 // TILE, x1 // TILE + 1):
                    self.lists[ty * self.tiles_x + tx].append(int(i))
        self.lists = [np.asarray(l, np.int64) for l in self.lists]
        self.frame = np.zeros((H, W, 4))
        self.mask = np.zeros((H, W), bool)
        self._cache = {}
        for t in range(len(self.lists)):
            ys, xs, inside = self.tile_pixels(t)
            q, B, s = self.tile_terms(t)
            T = np.cumprod(np.concatenate([np.ones((1,) + B.shape[1:]), 1.0 - B]), 0)[:-1]
            px = (T[..., None] * s).sum(0)
            near = (np.abs(q - 4.0) < NEAR).any(0)
            self.frame[ys[inside], xs[inside]] = px[inside]
            self.mask[ys[inside], xs[inside]] = near[inside]

    def tile_pixels(self, t):
        ty, tx = divmod(t, self.tiles_x)
        ys, xs = np.mgrid[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        return ys, xs, (ys < self.H) & (xs < self.W)

    def sequence(self, t):
        """the tile's list followed by the epilogue's draws of splat 0"""
        return np.concatenate([self.lists[t], np.zeros(self.n_epilogue if self.rec.drawn[0] else 0, np.int64)])

    def tile_terms(self, t):
        """(q, B, s) of the tile's sequence on its 16x16 pixels: (L,16,16), (L,16,16), (L,16,16,4)"""
        if t in self._cache:
            return self._cache[t]
        R = self.rec
        ids = self.sequence(t)
        ys, xs, _ = self.tile_pixels(t)
        c, g0, g1, col = (a[ids].astype(np.float64) for a in (R.c, R.g0, R.g1, R.color))
        dx = (xs + 0.5)[None] - c[:, 0, None, None]
        dy = (self.H - (ys + 0.5))[None] - c[:, 1, None, None]
        vx = dx * g0[:, 0, None, None] + dy * g0[:, 1, None, None]
        vy = dx * g1[:, 0, None, None] + dy * g1[:, 1, None, None]
        q = vx * vx + vy * vy
        B = np.where(q <= 4.0, np.exp(-q) * col[:, 3, None, None], 0.0)
        s = B[..., None] * np.concatenate([col[:, :3], np.ones((len(ids), 1))], 1)[:, None, None, :]
        if len(ids) <= 600 and len(self._cache) < 64:
            self._cache[t] = (q, B, s)
        return q, B, s

    def alpha_after(self, t):
        """(L+1,16,16): dst.a of the tile's pixels after 0, 1, .. L records of its sequence"""
        _, B, _ = self.tile_terms(t)
        return 1.0 - np.cumprod(np.concatenate([np.ones((1,) + B.shape[1:]), 1.0 - B]), 0)

    def has_fragment(self, t):
        """per list position: does the record put a fragment on an in-frame pixel of the tile?"""
        q, _, _ = self.tile_terms(t)
        inside = self.tile_pixels(t)[2]
        return ((q <= 4.0) & inside[None]).any((1, 2))[:len(self.lists[t])]

    def leave_one_out(self, t):
        """per list position: the largest change of any channel of any in-frame pixel of the tile when that record is removed"""
        _, B, s = self.tile_terms(t)
        inside = self.tile_pixels(t)[2]
        L = len(self.lists[t])
        T = np.cumprod(np.concatenate([np.ones((1,) + B.shape[1:]), 1.0 - B]), 0)[:-1]
        out = np.zeros(L)
        Rm = np.zeros(B.shape[1:] + (4,))                       # the blend of the records behind m, at full transmittance
        for m in range(len(B) - 1, -1, -1):
            if m < L:
                out[m] = np.abs(T[m][..., None] * (s[m] - B[m][..., None] * Rm))[inside].max()
            Rm = s[m] + (1.0 - B[m])[..., None] * Rm
        return out

    def rect_min_q(self, t, i):
        """min of q over the RECTANGLE spanned by the tile's 16x16 pixel centres (continuous; q is a convex quadratic: 0 when
        the centre is inside, else the minimum lies on an edge)"""
        R = self.rec
        ty, tx = divmod(t, self.tiles_x)
        cx, cy = (float(v) for v in R.c[i])
        g0, g1 = R.g0[i].astype(np.float64), R.g1[i].astype(np.float64)
        x0, x1 = tx * TILE + 0.5 - cx, tx * TILE + 15.5 - cx
        y1, y0 = self.H - (ty * TILE + 0.5) - cy, self.H - (ty * TILE + 15.5) - cy
        if x0 <= 0 <= x1 and y0 <= 0 <= y1:
            return 0.0
        best = np.inf
        for a, b in (((x0, y0), (x1, y0)), ((x0, y1), (x1, y1)), ((x0, y0), (x0, y1)), ((x1, y0), (x1, y1))):
            a, b = np.array(a), np.array(b)
            u0, du = np.array([a @ g0, a @ g1]), np.array([(b - a) @ g0, (b - a) @ g1])
            den = du @ du
            tt = min(max(-(u0 @ du) / den, 0.0), 1.0) if den > 0 else 0.0
            best = min(best, float(((u0 + tt * du) ** 2).sum()))
        return best

    def consumed(self, t, group, limit=1.0 - 1.0e-5, margin=5.0e-6, inside=None):
        """Records a kernel evaluates that votes "every in-frame pixel has dst.a > limit" after every `group` records of the
        list and stops when the vote passes (the epilogue is not counted).  -> (count, decided): decided is False when some vote
        the walk depends on falls within `margin` of the limit, where fp32 rounding could tip it.  `inside`: the pixels the
        vote waits for, if not the in-frame ones (what a kernel that forgot the frame's border would do)."""
        L = len(self.lists[t])
        if L == 0:
            return 0, True
        if inside is None:
            inside = self.tile_pixels(t)[2]
        a = self.alpha_after(t)
        decided = True
        for k in list(range(group, L, group)) + [L]:
            lo = a[k][inside].min()
            if abs(lo - limit) < margin:
                decided = False
            if lo > limit:
                return k, decided
        return L, decided
