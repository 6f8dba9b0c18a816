"""Oracle of COCO polygon annotations on the device (include/cvlm.h: cvlm_mask_poly_decode): the definition of §21 in
doubles -- Python floats and numpy float64, every product, sum and quotient one IEEE operation rounded on its own --, and, to hold it
against, the published maskApi.c's sort / difference / zero-merging loop written out literally and decoded by rle.decode.  pycocotools
is not a dependency of this project and is not installed where these tests were written: the restatement is the reference.  The
runner puts every output into sentinel-filled tensors with guard bands and checks the bands.  Importable without a GPU."""
import math

import numpy as np
import torch

import gt_oracle as GO
import sized_oracle as SO

MAX_COORD = 65536.0
MAX_VERTS = 65535
MAX_POINTS = 1 << 24
MAX_POLYS = 4096
SHAPES = [(1, 1), (1, 32), (5, 4), (33, 31), (32, 63), (65, 97), (130, 517)]

# (polygon, h, w, the set pixels as rows of (y, [x ...])) of the issue that asked for this feature
KNOWN = [
    ([1, 1, 4, 1, 4, 4, 1, 4], 6, 6, {y: [1, 2, 3] for y in (1, 2, 3)}),
    ([1, 1, 1, 1, 4, 1, 4, 4, 4, 4, 1, 4], 6, 6, {y: [1, 2, 3] for y in (1, 2, 3)}),
    ([0.5, 0.5, 5.5, 0.5, 3, 5.5], 7, 7, {1: [1, 2, 3, 4], 2: [2, 3, 4], 3: [2, 3], 4: [3]}),
    ([1, 1, 3, 3, 5, 1, 5, 5, 1, 5], 7, 7, {1: [1, 4], 2: [1, 2, 3, 4], 3: [1, 2, 3, 4], 4: [1, 2, 3, 4]}),
    ([-3, -3, 10, -3, 10, 10, -3, 10], 4, 5, {y: [0, 1, 2, 3, 4] for y in range(4)}),
    ([2, 2, 2, 2, 2, 2], 5, 5, {}),
]


def known_plane(rows, h, w):
    m = np.zeros((h, w), dtype=bool)
    for y, xs in rows.items():
        m[y, xs] = True
    return m


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------
def polygon_ok(xy) -> bool:
    """The project's own bounds (§21): an even number of doubles, 3 .. 65535 vertices, finite, |c| <= 65536, at most 2^24 walk points."""
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 1 or xy.size % 2 or not 6 <= xy.size <= 2 * MAX_VERTS:
        return False
    if not np.isfinite(xy).all() or np.abs(xy).max() > MAX_COORD:
        return False
    X, Y = scaled(xy)
    return int((np.maximum(np.abs(np.diff(X)), np.abs(np.diff(Y))) + 1).sum()) <= MAX_POINTS


def scaled(xy):
    """Step 1: (int)(5.0 * c + 0.5), closed."""
    xy = np.asarray(xy, dtype=np.float64)
    s = (5.0 * xy + 0.5).astype(np.int64)                             # two ufuncs, two roundings; astype truncates toward zero
    X, Y = s[0::2], s[1::2]
    return np.append(X, X[0]), np.append(Y, Y[0])


def walk(xy):
    """Steps 2 and 3: the points of all edges as one sequence -> (u, v) int64."""
    X, Y = scaled(xy)
    us, vs = [], []
    for j in range(len(X) - 1):
        xs, ys, xe, ye = int(X[j]), int(Y[j]), int(X[j + 1]), int(Y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, ys, xe, ye = xe, ye, xs, ys
        if dx == 0 and dy == 0:
            us.append(np.asarray([xs], dtype=np.int64))
            vs.append(np.asarray([ys], dtype=np.int64))
            continue
        n = max(dx, dy)
        d = np.arange(n + 1, dtype=np.int64)
        t = n - d if flip else d
        if dx >= dy:
            s = float(ye - ys) / float(dx)
            us.append(t + xs)
            vs.append(((float(ys) + s * t.astype(np.float64)) + 0.5).astype(np.int64))
        else:
            s = float(xe - xs) / float(dy)
            vs.append(t + ys)
            us.append(((float(xs) + s * t.astype(np.float64)) + 0.5).astype(np.int64))
    return np.concatenate(us), np.concatenate(vs)


def candidates(xy, h: int, w: int, uv=None) -> list:
    """Step 4, in doubles as maskApi.c has it: the boundary positions x * h + y, in the order of the walk.  uv: points to take in
    place of the walk's (what another arithmetic would have walked)."""
    u, v = walk(xy) if uv is None else uv
    out = []
    for j in np.nonzero(u[1:] != u[:-1])[0] + 1:
        a, b = int(u[j]), int(u[j - 1])
        xd = float(a if a < b else a - 1)
        xd = (xd + 0.5) / 5.0 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        c, e = int(v[j]), int(v[j - 1])
        yd = float(c if c < e else e)
        yd = (yd + 0.5) / 5.0 - 0.5
        yd = 0.0 if yd < 0 else float(h) if yd > h else yd
        out.append(int(xd) * h + int(math.ceil(yd)))
    return out


def plane_of(xy, h: int, w: int, uv=None) -> np.ndarray:
    """Step 5: pixel j = x * h + y is set iff an odd number of candidates lie at or before it -> bool (h, w)."""
    hits = np.zeros(h * w + 1, dtype=np.int64)
    np.add.at(hits, np.asarray(candidates(xy, h, w, uv), dtype=np.int64), 1)
    return (np.cumsum(hits[:h * w]) & 1).astype(bool).reshape(w, h).T.copy()


def counts_literal(xy, h: int, w: int) -> list:
    """The tail of maskApi.c's rleFrPoly written out: append h * w, sort, take differences, merge across zero counts."""
    a = sorted(candidates(xy, h, w) + [h * w])
    p = 0
    for j in range(len(a)):
        a[j], p = a[j] - p, a[j]
    k, j, b = len(a), 1, [a[0]]
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def expected(polys, h: int, w: int):
    """Step 6: the union of the polygons' planes, or None where a polygon is outside the bounds or the list is no list of 1 .. 4096."""
    if not 1 <= len(polys) <= MAX_POLYS or not all(polygon_ok(xy) for xy in polys):
        return None
    out = np.zeros((h, w), dtype=bool)
    for xy in polys:
        out |= plane_of(xy, h, w)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def circle(n: int, cx: float, cy: float, r: float) -> list:
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).reshape(-1).tolist()


def kinds(h: int, w: int) -> dict:
    """The polygon kinds on a plane of h x w: name -> one polygon."""
    W, H = float(w), float(h)
    out = {f"known_{i}": list(map(float, k[0])) for i, k in enumerate(KNOWN)}
    out["rect_int"] = [1.0, 1.0, max(2.0, W - 1), 1.0, max(2.0, W - 1), max(2.0, H - 1), 1.0, max(2.0, H - 1)]
    out["rect_half"] = [0.5, 0.5, W - 0.5, 0.5, W - 0.5, H - 0.5, 0.5, H - 0.5]
    out["tri_ccw"] = [0.0, 0.0, W * 0.9, H * 0.2, W * 0.3, H * 0.95]
    out["tri_cw"] = [0.0, 0.0, W * 0.3, H * 0.95, W * 0.9, H * 0.2]
    out["concave"] = [0.0, 0.0, W, 0.0, W, H, W * 0.5, H * 0.25, 0.0, H]
    out["bow_tie"] = [0.0, 0.0, W, H, W, 0.0, 0.0, H]
    out["outside_left"] = [-W - 3, 0.0, -1.0, 0.0, -1.0, H, -W - 3, H]
    out["outside_right"] = [W + 1, 0.0, 2 * W + 3, 0.0, 2 * W + 3, H, W + 1, H]
    out["outside_above"] = [0.0, -H - 3, W, -H - 3, W, -1.0, 0.0, -1.0]
    out["outside_below"] = [0.0, H + 1, W, H + 1, W, 2 * H + 3, 0.0, 2 * H + 3]
    out["covers"] = [-7.0, -7.0, W + 7, -7.0, W + 7, H + 7, -7.0, H + 7]
    out["on_the_far_sides"] = [W, H, W, -2.5, -2.5, -2.5, -2.5, H]
    out["collinear"] = [0.0, 0.0, W / 2, 0.0, W, 0.0, W, H / 2, W, H, W / 2, H, 0.0, H, 0.0, H / 2]
    out["repeated"] = [0.0, 0.0, 0.0, 0.0, W * 0.8, H * 0.1, W * 0.8, H * 0.1, W * 0.8, H * 0.1, W * 0.4, H * 0.9, W * 0.4, H * 0.9, 0.0, 0.0]
    out["all_equal"] = [W / 2, H / 2] * 4
    out["sliver_down"] = [W / 2, -1.0, W / 2, H + 1, W / 2 + 0.3, H + 1, W / 2 + 0.3, -1.0]
    out["sliver_across"] = [-1.0, H / 2, W + 1, H / 2, W + 1, H / 2 + 0.3, -1.0, H / 2 + 0.3]
    out["circle_1500"] = circle(1500, W * 0.5, H * 0.5, min(W, H) * 0.45)
    return out


def orientation_pairs(h: int, w: int):
    k = kinds(h, w)
    return k["tri_ccw"], k["tri_cw"]


def random_family(name: str, n: int, seed: int):
    """n planes of at most 40 x 40 with one polygon of 3 .. 8 vertices each -> [(polys, h, w)]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        k = int(rng.integers(3, 9))
        if name == "uniform":
            xy = rng.uniform(-5.0, 45.0, 2 * k)
        elif name == "tenths":
            xy = rng.integers(-50, 451, 2 * k) / 10.0
        else:
            xy = rng.integers(-5, 46, 2 * k).astype(np.float64)
        out.append(([xy.tolist()], h, w))
    return out


def union_items():
    """Planes of 2, 3 and 17 polygons, overlapping and disjoint, one inside another, ragged with single-polygon planes: nine planes."""
    rng = np.random.default_rng(21)
    r = lambda x0, y0, x1, y1: [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]
    items = [([r(1, 1, 20, 20), r(10, 10, 30, 28)], 33, 31),                                      # two, overlapping
             ([r(1, 1, 10, 10)], 33, 31),
             ([r(1, 1, 8, 8), r(12, 3, 20, 9), r(30, 40, 60, 60)], 65, 97),                      # three, disjoint
             ([r(2, 2, 60, 30), r(10, 8, 30, 20)], 32, 63),                                      # one inside another: XOR would cut a hole
             ([circle(12, 16 + 14 * (i % 5), 12 + 14 * (i // 5), 9.5) for i in range(17)], 65, 97),   # seventeen, overlapping in chains
             ([[0.5, 0.5, 3.5, 0.5, 2.0, 3.5]], 5, 4),
             ([rng.uniform(-5, 135, 10).tolist() for _ in range(3)], 130, 517),
             ([[0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0]], 1, 1),      # the same polygon twice: OR, not XOR
             ([r(0, 0, 32, 1), r(3, 0, 9, 1)], 1, 32)]
    return items


# ---- the runner --------------------------------------------------------------------------------------------------------------------------------
def tables(items, W: int = GO.WORD_GUARD):
    """items = [(polys, h, w)] -> (xy float64 with W sentinel doubles at both ends, poly_offsets, plane_polys)."""
    polys = [np.asarray(xy, dtype=np.float64) for ps, _, _ in items for xy in ps]
    flat = np.concatenate([np.full(W, 1e300)] + polys + [np.full(W, 1e300)])
    po = np.zeros(len(polys) + 1, dtype=np.int64)
    po[1:] = np.cumsum([p.size for p in polys])
    pp = np.zeros(len(items) + 1, dtype=np.int32)
    pp[1:] = np.cumsum([len(ps) for ps, _, _ in items])
    return flat, po + W, pp


def run_poly(entry, items, dev="cpu", *, guard: int = GO.GUARD, poly_offsets=None, plane_polys=None, total=None, bit_offsets=None,
             nbytes=None, max_pixels=None, ws_planes=None, stats=True, dims=None):
    """One call of hip.mask_poly_decode (or its host twin) for items = [(polys, h, w), ...] into ONE sentinel-filled uint8 tensor with
    `guard` bytes before the first plane and behind the last; the coordinates lie between sentinel doubles of 1e300, which no check
    lets through.  The keyword tables override the real ones (the refusal tests); ws_planes: the workspace holds that many planes.  ->
    (each plane's rows or None where its slice is no plane, area, box, status); every byte outside the planes' own slices and every
    band around area and box must still hold the sentinel."""
    from camouflaged_vlm_amd import hip
    P = len(items)
    sizes = [(h, w) for _, h, w in items]
    d, off, nb, _ = SO.tables(sizes, guard)
    if dims is not None:
        d = np.asarray(dims, dtype=np.int32).reshape(-1, 2)
    if bit_offsets is not None:
        off = np.asarray(bit_offsets, dtype=np.int64)
    flat, po, pp = tables(items)
    po = po if poly_offsets is None else np.asarray(poly_offsets, dtype=np.int64)
    pp = pp if plane_polys is None else np.asarray(plane_polys, dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xy = t(flat)
    xy = xy if total is None else xy[:total]
    bits = torch.full((nb,), GO.FILL, dtype=torch.uint8, device=dev)
    area_all, area = GO.guarded(P, dev) if stats else (None, None)
    box_all, box = GO.guarded((P, 4), dev) if stats else (None, None)
    status = torch.full((1,), -3, dtype=torch.int32, device=dev)
    mp = max(h * w for h, w in sizes) if max_pixels is None else max_pixels
    use = bits if nbytes is None else bits[:nbytes]
    if dev == "cpu":
        entry(xy, t(po), t(pp), t(d), t(off), mp, use, area, box, status)
    else:
        ws = torch.empty(hip.mask_poly_decode_workspace_bytes(P if ws_planes is None else ws_planes, mp), dtype=torch.uint8, device=dev)
        entry(xy, t(po), t(pp), t(d), t(off), mp, use, area, box, status, ws)
        torch.cuda.synchronize()
    raw = bits.cpu().numpy()
    keep = np.ones(nb, dtype=bool)
    out = []
    limit = nb if nbytes is None else nbytes
    for p in range(P):
        h, w = int(d[p, 0]), int(d[p, 1])
        n = 4 * h * ((w + 31) // 32)
        good = 1 <= h <= 16384 and 1 <= w <= 16384 and off[p] >= 0 and off[p] % 4 == 0 and off[p + 1] - off[p] == n and off[p + 1] <= limit
        if good:
            keep[off[p]:off[p + 1]] = False
            out.append(raw[off[p]:off[p + 1]].reshape(h, -1))
        else:
            out.append(None)
    assert (raw[keep] == GO.FILL).all(), "a byte outside the planes was overwritten"
    if stats:
        assert GO.bands_whole(area_all) and GO.bands_whole(box_all), "an element outside area / box was overwritten"
    return out, None if area is None else area.cpu().numpy(), None if box is None else box.cpu().numpy(), int(status.cpu().item())


def check_items(entry, items, dev="cpu", want=None, **over):
    """One call: status 0 and every plane the definition's, bit for bit, with its area and box -> the planes' rows."""
    got, area, box, status = run_poly(entry, items, dev=dev, **over)
    assert status == 0
    for p, (polys, h, w) in enumerate(items):
        m = expected(polys, h, w) if want is None else want[p]
        assert m is not None
        GO.check_plane(got[p], None if area is None else area[p], None if box is None else box[p], m, h, w)
    return got
