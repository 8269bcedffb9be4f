"""Reference-side composition of the viewer's label edits from the UNCHANGED oracle pieces (test infrastructure, shared by
tests/golden/make_golden_gl_edits.py and the render-edit tests).

What the reference does with an edit state (gs.js = Web_Viewer_Gaussians_Selection/gaussians_selection.js):
  hidden labels   worker, gs.js:302-307, 320: the alpha byte of the texture is multiplied by 0 (exact int32 label; NO_SELECTION is
                  never hidden, gs.js:619)
  displacement    vertex shader, gs.js:686-704: the first matching table row is added, in fp32, to the centre the shader reads; the
                  depth order (runSort, gs.js:417-462) stays that of the undisplaced buffer
  colours         fragment shader, gs.js:772-797: table colour mix(vColor.rgb, c, 0.6), then u_customColor, then the highlight
                  mix(., (1,0,0), 0.5); the shaders compare int(float(label))
`compose` builds that from oracle.texture / depth_order / render_view(override_color=...).  override_color is multiplied by the
depth fade, a table colour and u_customColor are not: the composition equals the reference only on frames whose colour-edited,
visible splats all have fade == 1 (`applies`)."""
import numpy as np

import oracle

NO_SELECTION = -999999


def state(selected=None, selection_mode=False, colours=None, custom_colour=None, displacements=None, hidden=()):
    """An edit state in the form of Context.set_render_edits's arguments (dict order = table order)."""
    return dict(selected=selected, selection_mode=bool(selection_mode), colours=dict(colours or {}), custom_colour=custom_colour,
                displacements=dict(displacements or {}), hidden=tuple(int(h) for h in hidden))


def shader_labels(labels_packed):
    """int(uintBitsToFloat(cen.w)): the label after its round trip through fp32 (gs.js:314, 699)."""
    return np.asarray(labels_packed, np.int32).astype(np.float32).astype(np.int64)


def first_match(vlabel, table):
    """Slot of the FIRST table entry whose label matches (the shaders' loops), -1 without one."""
    slot = np.full(len(vlabel), -1, np.int64)
    for k, lab in reversed(list(enumerate(table))):
        slot[vlabel == int(lab)] = k
    return slot


def edited_colours(base_rgb, vlabel, st):
    """Fragment shader gs.js:786-797 on per-splat colours `base_rgb` (n,3) float32 = vColor.rgb -> (rgb (n,3), edited mask)."""
    f = np.float32
    rgb = np.array(base_rgb, np.float32)
    edited = np.zeros(len(rgb), bool)
    slot = first_match(vlabel, st["colours"].keys())
    if len(st["colours"]):
        table = np.array([np.asarray(c, np.float32).reshape(3) for c in st["colours"].values()], np.float32)
        m = slot >= 0
        rgb[m] = rgb[m] * (f(1.0) - f(0.6)) + table[slot[m]] * f(0.6)
        edited |= m
    sel = vlabel == (NO_SELECTION if st["selected"] is None else int(st["selected"]))
    if st["custom_colour"] is not None:
        rgb[sel] = np.asarray(st["custom_colour"], np.float32).reshape(3)
        edited |= sel
    if st["selection_mode"]:
        rgb[sel] = rgb[sel] * f(0.5) + np.array([1, 0, 0], np.float32) * f(0.5)
        edited |= sel
    return rgb, edited


def compose(xyz, scale, rot, opacity, f_dc, labels, cam, W, H, st):
    """-> (frame (H, W, 4) float32, applies).  labels: int32 per splat in SOURCE order, or None (a PLY without labels)."""
    buf, order = oracle.pack_splats(xyz, scale, rot, opacity, f_dc)
    n = len(buf)
    lab = np.full(n, NO_SELECTION, np.int32) if labels is None else np.asarray(labels, np.int32)[order]
    tex = oracle.texture(buf, lab).reshape(n, 8).copy()
    vp = oracle.multiply4(oracle.proj_matrix(cam["fx"], cam["fy"], W, H), oracle.view_matrix(cam))
    di, _ = oracle.depth_order(buf, vp)                      # the UNEDITED buffer: the depth order does not move
    vlabel = shader_labels(lab)
    if len(st["displacements"]):                             # u_enableDisplacement = displacementMap.size > 0, gs.js:919
        slot = first_match(vlabel, st["displacements"].keys())
        table = np.array([np.asarray(d, np.float32).reshape(3) for d in st["displacements"].values()], np.float32)
        d = np.zeros((n, 3), np.float32)
        d[slot >= 0] = table[slot[slot >= 0]]
        pos = tex[:, :3].copy().view(np.float32)
        with np.errstate(invalid="ignore"):
            tex[:, :3] = (pos + d).astype(np.float32).view(np.uint32)
    hidden = np.isin(lab, [h for h in st["hidden"] if h != NO_SELECTION]) if len(st["hidden"]) else np.zeros(n, bool)
    tex[hidden, 7] &= np.uint32(0x00ffffff)
    base = np.stack([((tex[:, 7] >> np.uint32(8 * k)) & np.uint32(255)).astype(np.float32) / np.float32(255.0) for k in range(3)], axis=1)
    rgb, edited = edited_colours(base, vlabel, st)
    # fade of the colour-edited splats that can show: the composition multiplies their colour by it, the reference does not
    view32 = oracle.view_matrix(cam).astype(np.float32)
    proj32 = oracle.proj_matrix(cam["fx"], cam["fy"], W, H).astype(np.float32)
    applies = True
    for i in np.nonzero(edited & ~hidden)[0]:
        v = oracle.vertex(tex[i], view32, proj32, np.float32(cam["fx"]), np.float32(cam["fy"]), np.float32(W), np.float32(H))
        if v.drawn and v.fade != 1.0:
            applies = False
            break
    col = np.zeros((n, 4), np.float32)
    col[:, :3] = rgb
    frame = oracle.render_view(tex.reshape(-1), di, cam, W, H, override_color=col)
    return frame, applies


def fixture_calls(path):
    """tests/golden/render_gl_edits.npz -> [dict(id, attrs (xyz, scale, rot, opacity, f_dc), labels or None, cam, W, H, state,
    frame, applies, note)]."""
    z = np.load(path)
    notes = [str(s) for s in z["notes"]]
    out = []
    for i in (int(v) for v in z["calls"]):
        j = int(z[f"c{i}_scene"])
        fx, fy, W, H = (float(v) for v in z[f"c{i}_cam"])
        cam = {"img_name": f"edits{i}", "fx": fx, "fy": fy, "width": int(W), "height": int(H), "rotation": z[f"c{i}_R"].tolist(),
               "position": z[f"c{i}_p"].tolist()}
        mode, selected, custom_on = (int(v) for v in z[f"c{i}_select"])
        st = state(selected=selected, selection_mode=bool(mode), custom_colour=tuple(z[f"c{i}_custom"]) if custom_on else None,
                   colours={int(l): tuple(c) for l, c in zip(z[f"c{i}_colour_labels"], z[f"c{i}_colours"])},
                   displacements={int(l): tuple(d) for l, d in zip(z[f"c{i}_disp_labels"], z[f"c{i}_disps"])},
                   hidden=[int(h) for h in z[f"c{i}_hidden"]])
        out.append(dict(id=f"call{i}", attrs=[z[f"s{j}_{k}"] for k in ("xyz", "scale", "rot", "opacity", "f_dc")],
                        labels=z[f"s{j}_labels"] if f"s{j}_labels" in z.files else None, cam=cam, W=int(W), H=int(H), state=st,
                        frame=z[f"c{i}_frame"], applies=bool(z[f"c{i}_applies"]), note=notes[i], scene=j))
    return out
