"""numpy models of the rasterizer's per-splat pre pass (csrc/render_pre.hip: pre_geom, pre_one, pre_kernel, pre_multi_kernel,
bucket_kernel), no GPU code.

vertex       the vertex shader (gs.js:696-750) as oracle/render_oracle.c:gsxo_vertex evaluates it: float32, ONE numpy operation
             per C operation in the C's order, fp16 read through np.float16, fminf with its NaN rule.  numpy rounds every
             float32 operation once (no contraction, correctly rounded division and square root), as the C compiled with
             -ffp-contract=off does: the agreement with oracle.vertex is bit for bit (test_vertex_model.py).
pixel_box    the bounding box of the ellipse in pixels whose centre it holds, float32 (shared with blend_model.Records)
rect         that box as the kernels pack it: tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24, 1 where the splat reaches no pixel centre
depth_keys   runSort's keys (gs.js:436-441), fp64: ToInt32((vp2 x + vp6 y + vp10 z) * 4096)
buckets      the 16-bit depth bucket (gs.js:443-447), the level-1 sort key in both `compact` forms, the dropped splats
record       the 12 floats the pre kernels store per splat, colour path (rgba8 / SH / label edits) included"""
import numpy as np

f32 = np.float32
EMPTY_RECT = 1
SLACK = 0.015625        # 1/64 px on every side of the box
CLASSES = ("cull_z", "cull_x_lo", "cull_x_hi", "cull_y_lo", "cull_y_hi", "l2_negative", "degenerate", "capped", "drawn")
CLS = {name: k for k, name in enumerate(CLASSES)}


def js_toint32(x):
    """`x | 0` on float64: NaN and the infinities give 0, everything else is truncated and wrapped modulo 2^32"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isfinite(x), np.trunc(x), 0.0)
        m = np.fmod(t, 4294967296.0)                      # exact
    m = np.where(m < 0, m + 4294967296.0, m)
    return m.astype(np.uint64).astype(np.uint32).view(np.int32)


def half(words, high):
    """unpackHalf2x16: one half of each uint32 as float32 (exact)"""
    h = (words >> np.uint32(16)) if high else (words & np.uint32(0xffff))
    return h.astype(np.uint16).view(np.float16).astype(f32)


def fminf(a, b):
    """C fminf: the other operand where one is NaN"""
    return np.where(np.isnan(a), b, np.minimum(a, b))


def vertex(tex, view, proj, fx, fy, W, H):
    """tex: (8n,) or (n, 8) uint32 texel pairs; view, proj: 16 numbers each (rounded to float32 here, as gl.uniformMatrix4fv
    does).  -> dict of per-splat arrays: drawn (bool), cx, cy, g0 (n,2), g1, major, minor, fade, color (n,4) - valid where drawn -
    cls (index into CLASSES: the FIRST test of the shader that rejects the splat, `capped` = drawn with an axis at the
    1024-pixel cap) and, for the scenes' own assertions, the conic's c01, hx, l2, the clip position p2 and clip = 1.2 w."""
    tex = np.ascontiguousarray(tex, np.uint32).reshape(-1, 8)
    c = tex[:, :3].copy().view(f32)
    view, proj = np.asarray(view).astype(f32), np.asarray(proj).astype(f32)
    fx, fy, W, H = f32(fx), f32(fy), f32(W), f32(H)
    one, zero, two = f32(1.0), f32(0.0), f32(2.0)
    with np.errstate(all="ignore"):
        cam = [view[k] * c[:, 0] + view[4 + k] * c[:, 1] + view[8 + k] * c[:, 2] + view[12 + k] * one for k in range(4)]
        p2 = [proj[k] * cam[0] + proj[4 + k] * cam[1] + proj[8 + k] * cam[2] + proj[12 + k] * cam[3] for k in range(4)]
        clip = f32(1.2) * p2[3]
        culls = [p2[2] < -clip, p2[0] < -clip, p2[0] > clip, p2[1] < -clip, p2[1] > clip]
        u1x, u1y = half(tex[:, 4], 0), half(tex[:, 4], 1)
        u2x, u2y = half(tex[:, 5], 0), half(tex[:, 5], 1)
        u3x, u3y = half(tex[:, 6], 0), half(tex[:, 6], 1)
        V = [[u1x, u1y, u2x], [u1y, u2y, u3x], [u2x, u3x, u3y]]
        ja = fx / cam[2]
        jb = -(fx * cam[0]) / (cam[2] * cam[2])
        jc = -fy / cam[2]
        jd = (fy * cam[1]) / (cam[2] * cam[2])
        t0 = [view[4 * i] * ja + view[4 * i + 1] * zero + view[4 * i + 2] * jb for i in range(3)]
        t1 = [view[4 * i] * zero + view[4 * i + 1] * jc + view[4 * i + 2] * jd for i in range(3)]
        a0 = [t0[0] * V[k][0] + t0[1] * V[k][1] + t0[2] * V[k][2] for k in range(3)]
        a1 = [t1[0] * V[k][0] + t1[1] * V[k][1] + t1[2] * V[k][2] for k in range(3)]
        c00 = a0[0] * t0[0] + a0[1] * t0[1] + a0[2] * t0[2]
        c01 = a1[0] * t0[0] + a1[1] * t0[1] + a1[2] * t0[2]
        c11 = a1[0] * t1[0] + a1[1] * t1[1] + a1[2] * t1[2]
        mid = (c00 + c11) / two
        hx = (c00 - c11) / two
        radius = np.sqrt(hx * hx + c01 * c01)
        l1, l2 = mid + radius, mid - radius
        neg = l2 < zero
        dx, dy = c01, l1 - c00
        dl = np.sqrt(dx * dx + dy * dy)
        ux, uy = dx / dl, dy / dl
        s1 = fminf(np.sqrt(two * l1), f32(1024.0))
        s2 = fminf(np.sqrt(two * l2), f32(1024.0))
        mx, my, nx, ny = s1 * ux, s1 * uy, s2 * uy, s2 * -ux
        fade = p2[2] / p2[3] + one
        fade = np.where(fade < zero, zero, np.where(fade > one, one, fade))
        rgba = tex[:, 7]
        color = np.stack([fade * ((rgba >> np.uint32(8 * k)) & np.uint32(0xff)).astype(f32) / f32(255.0) for k in range(4)], 1)
        cx = (p2[0] / p2[3] + one) * f32(0.5) * W
        cy = (p2[1] / p2[3] + one) * f32(0.5) * H
        m2, n2 = mx * mx + my * my, nx * nx + ny * ny
        sound = (m2 > zero) & (n2 > zero) & np.isfinite(m2) & np.isfinite(n2) & np.isfinite(cx) & np.isfinite(cy)
        g0 = np.stack([two * mx / m2, two * my / m2], 1)
        g1 = np.stack([two * nx / n2, two * ny / n2], 1)
    culled = np.zeros(len(tex), bool)
    cls = np.full(len(tex), CLS["drawn"], np.int64)
    capped = (s1 == f32(1024.0)) | (s2 == f32(1024.0))
    cls[capped] = CLS["capped"]
    cls[~sound] = CLS["degenerate"]
    cls[neg] = CLS["l2_negative"]
    for k in range(4, -1, -1):
        cls[culls[k]] = k
        culled |= culls[k]
    drawn = ~culled & ~neg & sound
    return dict(drawn=drawn, cls=cls, cx=cx, cy=cy, g0=g0, g1=g1, major=np.stack([mx, my], 1), minor=np.stack([nx, ny], 1),
                fade=fade, color=color, c01=c01, hx=hx, l2=l2, w=p2[3], p2=p2, clip=clip)


def pixel_box(cx, cy, major, minor, drawn, W, H, slack=SLACK, low=np.ceil):
    """Pixels whose CENTRE lies in the bounding box of the ellipse with half-axes major, minor (+ slack px), clipped to the frame:
    (n, 4) int64 (x0, x1, r0, r1) inclusive, image rows; (1, 0, 1, 0) where the splat is not drawn or reaches no pixel centre.
    float32, as a binner that works on the vertex shader's outputs sees them.  (slack, low: what a binner without the slack, or
    one that rounds the low side down, would hold - for the scenes' own assertions.)"""
    Wf, Hf = f32(W), f32(H)
    with np.errstate(all="ignore"):
        ex = np.sqrt(major[:, 0] * major[:, 0] + minor[:, 0] * minor[:, 0]) + f32(slack)
        ey = np.sqrt(major[:, 1] * major[:, 1] + minor[:, 1] * minor[:, 1]) + f32(slack)
        top = Hf - cy
        clampx = lambda v: np.minimum(np.maximum(v, f32(-1.0)), Wf)
        clampy = lambda v: np.minimum(np.maximum(v, f32(-1.0)), Hf)
        edges = [low(clampx(cx - ex - f32(0.5))), np.floor(clampx(cx + ex - f32(0.5))),
                 low(clampy(top - ey - f32(0.5))), np.floor(clampy(top + ey - f32(0.5)))]
        x0, x1, r0, r1 = (np.where(drawn & np.isfinite(e), e, 0).astype(np.int64) for e in edges)
    x0, r0 = np.maximum(x0, 0), np.maximum(r0, 0)
    x1, r1 = np.minimum(x1, int(W) - 1), np.minimum(r1, int(H) - 1)
    box = np.stack([x0, x1, r0, r1], 1)
    box[~drawn | (x1 < x0) | (r1 < r0)] = (1, 0, 1, 0)
    return box


def pack_rect(box):
    """(n, 4) pixel boxes -> the kernels' uint32 tile rectangles"""
    t = box >> 4
    r = (t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)).astype(np.uint32)
    r[box[:, 1] < box[:, 0]] = EMPTY_RECT
    return r


def rect(v, W, H, slack=SLACK, low=np.ceil):
    """the tile rectangle per splat from vertex()'s result"""
    return pack_rect(pixel_box(v["cx"], v["cy"], v["major"], v["minor"], v["drawn"], W, H, slack, low))


def unpack_rect(r):
    r = np.asarray(r, np.uint32)
    return np.stack([r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24], 1).astype(np.int64)


def depth_keys(buffer, viewproj):
    """buffer: (n, 32) uint8 .splat rows (or (n, 3) float32 positions); viewproj: proj * view, 16 float64"""
    b = np.ascontiguousarray(buffer)
    pos = (b[:, :12].copy().view(f32) if b.dtype == np.uint8 else b.astype(f32)).astype(np.float64)
    vp = np.asarray(viewproj, np.float64)
    with np.errstate(all="ignore"):
        return js_toint32((vp[2] * pos[:, 0] + vp[6] * pos[:, 1] + vp[10] * pos[:, 2]) * 4096.0)


def buckets(depth, compact, rect_in):
    """-> dict: bucket (65536 = dropped), in_range, key (the level-1 sort key), dropped (count), rect (dropped ones cleared)"""
    d = np.asarray(depth, np.int32).astype(np.float64)
    lo, hi = d.min(), d.max()
    with np.errstate(all="ignore"):
        inv = np.float64(65536.0) / np.float64(hi - lo)
        b = js_toint32((d - lo) * inv).astype(np.int64)
    in_range = (b >= 0) & (b < 65536)
    bucket = np.where(in_range, b, 65536).astype(np.uint32)
    rect_in = np.asarray(rect_in, np.uint32)
    seen = in_range & (rect_in != EMPTY_RECT)
    key = np.where(seen, bucket, np.uint32(0xffffffff)) if compact else np.where(in_range, bucket, np.uint32(65535))
    return dict(bucket=bucket, in_range=in_range, key=key.astype(np.uint32), dropped=int((~in_range).sum()),
                rect=np.where(in_range, rect_in, np.uint32(EMPTY_RECT)).astype(np.uint32), min=int(lo), max=int(hi))


def depth_index(bucket):
    """runSort's depthIndex from the buckets: the kept splats, stably sorted, then the slots the JS never writes (0)"""
    keep = np.nonzero(bucket < 65536)[0]
    di = np.zeros(len(bucket), np.uint32)
    di[:len(keep)] = keep[np.argsort(bucket[keep], kind="stable")]
    return di


def record(v, r, rgb=None, alpha=None):
    """The 12 floats of a splat's record, (n, 12) float32: (cx, cy, g0, g1, r, g, b, a, 0, 0) where the splat has a rectangle,
    zeros elsewhere (what splat 0 gets without one).  rgb: (n, 3) replaces the rgba8 colour (already faded), alpha likewise."""
    n = len(r)
    out = np.zeros((n, 12), f32)
    has = r != EMPTY_RECT
    col = v["color"].copy()
    if rgb is not None:
        col[:, :3] = rgb
    if alpha is not None:
        col[:, 3] = alpha
    full = np.concatenate([v["cx"][:, None], v["cy"][:, None], v["g0"], v["g1"], col, np.zeros((n, 2), f32)], 1).astype(f32)
    out[has] = full[has]
    return out
