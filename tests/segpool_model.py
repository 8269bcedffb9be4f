"""The pool form of one segmentation map, every byte of its stride, restated in numpy for all four layouts of map_layout()
(csrc/host_pack.cpp), written from the layout comments of csrc/host_pack.hpp and csrc/handover.hip alone: it neither calls
oracle.pack_map_numpy nor the host packer, and it builds the strips by reshaping padded planes where those scatter by index.

A map of w x h pixels holds, from its 256-byte aligned start:

  tiled (seg_tiled = 1)   the full-resolution level: u8 bins (label + 1) in strips of 16 pixel columns, a strip = 16 bytes per
                          pixel row, rows padded to a multiple of 8 (one band); ceil(w / 16) strips of ceil(h / 8) * 128 bytes.
  row-major               the bins row by row, w * h bytes, and four tail bytes.
  coarse (tiled only,     at the next multiple of 256: one byte per 4 x 4 cell, in strips of 16 cells, cell rows padded to a
  <= 254 classes)         multiple of 8: the bin the cell's 16 pixels share, 255 where they differ or the cell sticks out of the
                          map.  With 255 classes bin 255 is a class, so there is no coarse level.

The stride to the next map is the map's size rounded up to 256.  Every byte that is neither a pixel nor a cell is 0: the
columns and rows a strip holds past the map, the cells and cell rows a coarse strip holds past the cell grid, the gap before
the coarse level, the gap before the next map, the row-major tail."""
import numpy as np

PAD, PIXEL, COARSE = 0, 1, 2          # kinds of byte, see pool_kinds()
KIND_NAMES = {PAD: "padding", PIXEL: "pixel", COARSE: "coarse"}

STRIP_COLS, BAND_ROWS = 16, 8         # the full-resolution level
CELL = 4
CSTRIP_CELLS, CBAND_ROWS = 16, 8      # the coarse level


def _up(v, m):
    return (v + m - 1) // m * m


def _strips(plane, cols, band):
    """plane (rows, columns) -> bytes: strips of `cols` columns side by side, inside a strip row after row, rows padded to a
    multiple of `band`, columns to whole strips; the padding is 0."""
    r, c = plane.shape
    full = np.zeros((_up(r, band), _up(c, cols)), plane.dtype)
    full[:r, :c] = plane
    return full.reshape(full.shape[0], full.shape[1] // cols, cols).transpose(1, 0, 2).reshape(-1)


def has_coarse(n_classes, tiled=True, coarse=True):
    return bool(tiled and coarse and n_classes + 1 <= 255)


def geometry(w, h, n_classes, tiled=True, coarse=True):
    """-> dict(fine_bytes, coarse_off, map_bytes, stride): coarse_off is None when the layout has no coarse level"""
    fine = _up(h, BAND_ROWS) * STRIP_COLS * (_up(w, STRIP_COLS) // STRIP_COLS) if tiled else w * h + 4
    cw, ch = _up(w, CELL) // CELL, _up(h, CELL) // CELL
    if has_coarse(n_classes, tiled, coarse):
        coff = _up(fine, 256)
        size = coff + _up(ch, CBAND_ROWS) * CSTRIP_CELLS * (_up(cw, CSTRIP_CELLS) // CSTRIP_CELLS)
    else:
        coff, size = None, fine
    return {"fine_bytes": fine, "coarse_off": coff, "map_bytes": size, "stride": _up(size, 256)}


def bins_of(seg, packed_u8=False):
    """the u8 bin of every pixel: label + 1, or the map itself for a uint8 map that already holds bins"""
    seg = np.asarray(seg)
    if seg.ndim != 2:
        raise ValueError("a map is 2-D")
    if packed_u8:
        if seg.dtype != np.uint8:
            raise ValueError("packed_u8 maps are uint8")
        return seg.copy()
    b = seg.astype(np.int64) + 1
    if b.min() < 0 or b.max() > 255:
        raise ValueError("label outside [-1, 254]")
    return b.astype(np.uint8)


def coarse_cells(bins):
    """(ch, cw) uint8: the bin a 4 x 4 cell's pixels share; 255 where they differ, or where the cell sticks out of the map"""
    h, w = bins.shape
    ch, cw = _up(h, CELL) // CELL, _up(w, CELL) // CELL
    lo = np.full((ch * CELL, cw * CELL), 0, np.int32)       # outside the map: lo = 0 and hi = 256 never meet
    hi = np.full((ch * CELL, cw * CELL), 256, np.int32)
    lo[:h, :w] = bins
    hi[:h, :w] = bins
    lo = lo.reshape(ch, CELL, cw, CELL).min(axis=(1, 3))
    hi = hi.reshape(ch, CELL, cw, CELL).max(axis=(1, 3))
    return np.where(lo == hi, lo, 255).astype(np.uint8)


def _assemble(fine_plane, cell_plane, w, h, n_classes, tiled, coarse):
    g = geometry(w, h, n_classes, tiled, coarse)
    out = np.zeros(g["stride"], fine_plane.dtype)
    level = _strips(fine_plane, STRIP_COLS, BAND_ROWS) if tiled else fine_plane.reshape(-1)
    out[:level.size] = level
    assert level.size == (g["fine_bytes"] if tiled else g["fine_bytes"] - 4)
    if g["coarse_off"] is not None:
        clevel = _strips(cell_plane, CSTRIP_CELLS, CBAND_ROWS)
        assert g["coarse_off"] + clevel.size == g["map_bytes"]
        out[g["coarse_off"]:g["map_bytes"]] = clevel
    return out


def pool_bytes(seg, n_classes, tiled=True, coarse=True, packed_u8=False):
    """-> uint8[stride]: the complete bytes of the map's pool stride"""
    bins = bins_of(seg, packed_u8)
    if int(bins.max()) > n_classes:
        raise ValueError("label outside [-1, n_classes - 1]")
    h, w = bins.shape
    return _assemble(bins, coarse_cells(bins), w, h, n_classes, tiled, coarse)


def pool_kinds(w, h, n_classes, tiled=True, coarse=True):
    """-> uint8[stride]: PIXEL where pool_bytes holds a pixel's bin, COARSE where it holds a cell, PAD everywhere else"""
    ch, cw = _up(h, CELL) // CELL, _up(w, CELL) // CELL
    return _assemble(np.full((h, w), PIXEL, np.uint8), np.full((ch, cw), COARSE, np.uint8), w, h, n_classes, tiled, coarse)


def check_map(got, seg, n_classes, tiled=True, coarse=True, packed_u8=False, what=""):
    """asserts that got (the stride's bytes, or its first map_bytes) equals the model, and says which kind of byte does not"""
    want = pool_bytes(seg, n_classes, tiled, coarse, packed_u8)
    h, w = np.asarray(seg).shape
    got = np.asarray(got)
    assert got.size in (want.size, geometry(w, h, n_classes, tiled, coarse)["map_bytes"]), f"{what}: {got.size} bytes for a stride of {want.size}"
    msg = describe_mismatch(got, want[:got.size], pool_kinds(w, h, n_classes, tiled, coarse)[:got.size])
    assert not msg, f"{what} {w}x{h} tiled={tiled} coarse={coarse}: {msg}"


# ---- the maps both test files use ---------------------------------------------------------------------------------------------
EDGE_WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)      # cell, strip and coarse-strip edges at -1 / 0 / +1
EDGE_HEIGHTS = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33)        # cell, band and coarse-band edges at -1 / 0 / +1
EXTRA_SHAPES = ((65, 61), (33, 70), (322, 181))         # 17 x 16 = 272 cells, just over one workgroup of 256; 16 x 24 padded cells, one
                                                        # and a half; a mid-size map
BIG_SHAPE = (1920, 1080)
NOISE = (0.0, 0.02, 0.6)
DTYPES = ("i32", "i64", "u8", "u8p")

# ---- the maps of the compact hand-over's tests (tests/test_handover_expand_gpu.py, and their host chain in tests/test_segpool_model.py)
RANK_SHAPE = (1040, 8)                                  # 260 cells per cell row - one round of 256 threads and four more - in one band
RANK_CASES = (                                          # mixed cells as {cell row: cell columns}: the ranks at the wave and round edges
    {0: [63]}, {0: [64]}, {0: [63, 64], 1: [0]}, {0: range(256)}, {0: [255, 256]}, {0: list(range(256)) + [257]}, {1: [256, 259]},
    {0: range(260), 1: range(260)})
RANK_BLOCKS = (1, 1, 3, 256, 2, 257, 2, 520)            # mixed cells = 16-byte blocks of each case
UNIT_SHAPES = tuple((w, h) for w in (1020, 1024, 1028) for h in (8, 9)) + ((2044, 5), (2048, 8), (2052, 5), (4100, 4))
LONG_SHAPES = ((65535, 1), (1, 65535))                  # the largest sides the library takes
DTYPE_SHAPES = ((61, 35), (130, 71), (1028, 9))


def rank_case_cells(case):
    return [(cy, cx) for cy, cols in sorted(case.items()) for cx in cols]


def blocky_labels(rng, w, h, n_classes, p_noise, lowest=-1):
    """int64 labels in [lowest, n_classes - 1]: 8 x 8 blocks of one random label with per-pixel noise, so that uniform cells,
    mixed cells and (at ragged sizes) cells that stick out of the map all occur"""
    blocks = rng.integers(lowest, n_classes, size=((h + 7) // 8, (w + 7) // 8))
    lab = np.repeat(np.repeat(blocks, 8, 0), 8, 1)[:h, :w].astype(np.int64)
    noise = rng.random((h, w)) < p_noise
    lab[noise] = rng.integers(lowest, n_classes, size=int(noise.sum()))
    return lab


def mixed_cells_map(w, h, cells, base, n_classes=150):
    """int64 labels: `base` everywhere, and one odd pixel in each of the listed (cell row, cell column) cells, so that exactly those
    cells are mixed (given that no cell sticks out of the map: w and h are multiples of 4).  The k-th listed cell gets a label and
    a place in the cell that no other of the first 16 * (n_classes - 1) cells has: a block expanded from another cell's rank shows."""
    assert w % CELL == 0 and h % CELL == 0 and 0 <= base < n_classes
    odd = [v for v in range(n_classes) if v != base]
    cells = list(cells)
    assert len(set(cells)) == len(cells) <= CELL * CELL * len(odd)
    lab = np.full((h, w), base, np.int64)
    for k, (cy, cx) in enumerate(cells):
        dy, dx = divmod((k // len(odd)) % (CELL * CELL), CELL)
        assert 0 <= cy < h // CELL and 0 <= cx < w // CELL
        lab[cy * CELL + dy, cx * CELL + dx] = odd[k % len(odd)]
    return lab


def record_bytes(seg, stream_off, packed_u8=False):
    """bytes of the map's compact record (csrc/host_pack.hpp): the table and the coarse level (stream_off, which the host hook
    tells) and one 16-byte block per cell whose coarse byte is 255"""
    return int(stream_off) + 16 * int((coarse_cells(bins_of(seg, packed_u8)) == 255).sum())


def as_dtype(lab, dtype):
    """labels (>= 0 for "u8") -> (array of that seg dtype, packed_u8)"""
    if dtype == "i32":
        return lab.astype(np.int32), False
    if dtype == "i64":
        return lab.astype(np.int64), False
    if dtype == "u8":
        assert lab.min() >= 0
        return lab.astype(np.uint8), False
    assert dtype == "u8p"
    return (lab + 1).astype(np.uint8), True


def describe_mismatch(got, want, kinds, limit=8):
    """'' when got == want, else which kinds of byte differ and the first offsets of each (with got / want values)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return ""
    parts = []
    kind = np.where(np.isin(kinds, (PIXEL, COARSE)), kinds, PAD)      # whatever is no pixel and no cell is padding
    for k, name in KIND_NAMES.items():
        idx = bad[kind[bad] == k]
        if idx.size:
            first = ", ".join(f"{int(i)}: {int(got[i])} != {int(want[i])}" for i in idx[:limit])
            parts.append(f"{idx.size} {name} bytes differ (offset: got != want: {first})")
    return "; ".join(parts)
