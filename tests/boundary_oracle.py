"""Boundary IoU as published, in plain numpy: `boundary_radius` is boundary_iou_api's radius, `erode` the window
definition -- ero(y, x) = AND of X over |y' - y| <= d, |x' - x| <= d with every pixel outside the plane clear, which is
cv2.copyMakeBorder(1, constant 0) + d erosions by ones((3, 3)) + the crop --, `boundary` = X & ~ero, `boundary_iou` the IoU of two
boundaries, and `evaluate_group` COCOeval.evaluateImg (tests/match_oracle.py) over min(mask IoU, boundary IoU).  `run` calls
cvlm_mask_boundary_sized or its host entry on a list of planes inside guard bands; `run_match` cvlm_coco_match_boundary or its host
entry through match_oracle.run_entry."""
import numpy as np

import match_oracle as MO

GUARD = 16                    # sentinel bytes before the first and behind the last plane, inside bits / out_bits (offsets stay multiples of 4)
BAND = 64                     # sentinel bytes around the workspace and elements around out_area
FILL = 0xA5
MAX_RADIUS = 16384


def boundary_radius(h, w, ratio=0.02):
    return max(1, int(round(ratio * np.sqrt(h ** 2 + w ** 2))))


def erode(x: np.ndarray, d: int) -> np.ndarray:
    """The window definition, one loop per axis over the 2 d + 1 offsets of a plane padded with d clear pixels on every side (an AND
    over a product of ranges is the AND over one of the ANDs over the other).  A loop ends early only when nothing is left."""
    h, w = x.shape
    pad = np.zeros((h + 2 * d, w + 2 * d), dtype=bool)
    pad[d:d + h, d:d + w] = x
    rows = np.ones((h + 2 * d, w), dtype=bool)
    for dx in range(-d, d + 1):
        rows &= pad[:, d + dx:d + dx + w]
        if not rows.any():
            break
    out = np.ones((h, w), dtype=bool)
    for dy in range(-d, d + 1):
        out &= rows[d + dy:d + dy + h]
        if not out.any():
            break
    return out


def boundary(x: np.ndarray, d: int) -> np.ndarray:
    x = np.asarray(x, dtype=bool)
    return x & ~erode(x, d)


def boundary_iou(a: np.ndarray, b: np.ndarray, d: int) -> float:
    ba, bb = boundary(a, d), boundary(b, d)
    inter, union = int((ba & bb).sum()), int((ba | bb).sum())
    return inter / union if inter else 0.0


# ---- cvlm_mask_boundary_sized on lists of planes ---------------------------------------------------------------------------------------------
def tables(sizes, guard: int = GUARD):
    """-> dims int32 (P, 2), offsets int64 (P + 1) starting at `guard`, the byte length (guard behind the last plane too), the largest
    word count."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    offsets = guard + np.concatenate([[0], np.cumsum(4 * words)]).astype(np.int64)
    return dims, offsets, int(offsets[-1]) + guard, int(words.max())


def pack(plane: np.ndarray) -> np.ndarray:
    """bool (h, w) -> uint8 (h, 4 * ceil(w / 32)): numpy.packbits' order, pad bits 0."""
    h, w = plane.shape
    ws = (w + 31) // 32
    full = np.zeros((h, 32 * ws), dtype=np.uint8)
    full[:, :w] = plane
    return np.packbits(full, axis=1)


def unpack(rows: np.ndarray, w: int):
    """uint8 (h, 4 ws) -> (bool (h, w), True if a pad bit is set)."""
    bits = np.unpackbits(rows, axis=1).astype(bool)
    return bits[:, :w], bool(bits[:, w:].any())


def run(fn, planes, radii, dev="cpu", area=True, shift=0, outs=None, offsets=None, dims=None, dirty_pads=False):
    """One call of hip.mask_boundary_sized / its host twin on `planes` (bool arrays) at `radii`.  bits and out_bits are sentinel-filled
    tensors with GUARD bytes before the first and behind the last plane; the workspace and out_area lie between BAND sentinels.  shift:
    bytes by which the base of bits is moved off its allocation.  outs: the tensors of an earlier call, to be used again.  offsets /
    dims: doctored tables (the refusal tests).  dirty_pads: the input's pad bits are set.  -> dict(planes: each plane's bool array or
    None where its slice is refused, raw: each plane's output bytes, area, status, outs); every band is checked."""
    import torch
    sizes = [p.shape for p in planes]
    good_dims, good_off, nbytes, max_words = tables(sizes)
    src = np.full(nbytes, FILL, dtype=np.uint8)
    for p, plane in enumerate(planes):
        rows = pack(plane)
        if dirty_pads:
            h, w = plane.shape
            full = np.ones((h, rows.shape[1] * 8), dtype=np.uint8)
            full[:, :w] = plane
            rows = np.packbits(full, axis=1)
        src[good_off[p]:good_off[p + 1]] = rows.reshape(-1)
    P = len(planes)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    holder = torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)
    bits = holder[shift:shift + nbytes]
    bits.copy_(dv(src))
    fresh = outs is None
    if fresh:
        outs = dict(out=torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev),
                    ws=torch.full((nbytes + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    area=torch.full((P + 2 * BAND,), -7, dtype=torch.int32, device=dev),
                    status=torch.full((1,), 77, dtype=torch.int32, device=dev))
    use_off = good_off if offsets is None else np.asarray(offsets, dtype=np.int64)
    use_dims = good_dims if dims is None else np.asarray(dims, dtype=np.int32).reshape(P, 2)
    fn(bits, dv(use_off), dv(use_dims), dv(np.asarray(radii, dtype=np.int32)), max_words, outs["ws"][BAND:BAND + nbytes], outs["out"],
       outs["area"][BAND:BAND + P] if area else None, outs["status"])
    raw = outs["out"].cpu().numpy()
    ws = outs["ws"].cpu().numpy()
    ar = outs["area"].cpu().numpy()
    assert (raw[:GUARD] == FILL).all() and (raw[nbytes - GUARD:] == FILL).all(), "out_bits: a guard band was written"
    assert (ws[:BAND] == FILL).all() and (ws[BAND + nbytes:] == FILL).all(), "workspace: a guard band was written"
    assert (ar[:BAND] == -7).all() and (ar[BAND + P:] == -7).all(), "out_area: a guard band was written"
    assert area or not fresh or (ar == -7).all(), "out_area was written although it was NULL"
    got, rows_of = [], []
    for p, (h, w) in enumerate(sizes):
        rows = raw[good_off[p]:good_off[p + 1]].reshape(h, -1)
        plane, dirty = unpack(rows, w)
        assert not dirty or (rows == FILL).all(), f"plane {p}: a pad bit is set"
        got.append(plane)
        rows_of.append(rows)
    return dict(planes=got, raw=rows_of, area=ar[BAND:BAND + P].copy(), status=int(outs["status"].cpu().numpy()[0]), outs=outs)


def check(res, planes, radii, refused=(), untouched=(), area=True):
    """The outputs of `run` against the oracle, every bit and count; a refused plane is zero bytes, or -- `untouched`: its slice is
    no range of whole words inside the buffer -- the sentinel it held."""
    for p, (plane, d) in enumerate(zip(planes, radii)):
        if p in refused or p in untouched:
            assert (res["raw"][p] == (FILL if p in untouched else 0)).all(), p
            assert not area or res["area"][p] == 0, p
            continue
        want = boundary(plane, int(d))
        assert np.array_equal(res["planes"][p], want), (p, plane.shape, d, int((res["planes"][p] != want).sum()))
        assert not area or res["area"][p] == int(want.sum()), (p, res["area"][p], int(want.sum()))


# ---- planes -------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 129, 257)
HEIGHTS = (1, 2, 33, 130)
RAGGED = [(1, 1), (70, 33), (5, 65), (33, 31), (1, 32), (97, 131), (2, 64)]          # DESIGN.md §19's seven


def radii_of(h: int, w: int):
    """1, 2, 16, 17, the published radius, and the three radii around 2 d + 1 = min(h, w) -- those that are radii."""
    m = min(h, w)
    rs = {1, 2, 16, 17, boundary_radius(h, w), (m - 1) // 2, (m - 1) // 2 + 1, (m - 1) // 2 - 1}
    return sorted(r for r in rs if 1 <= r <= MAX_RADIUS)


def contents(h: int, w: int, seed: int):
    """(name, plane) of every kind of content the issue lists, at one size."""
    rng = np.random.default_rng(seed)
    full = np.ones((h, w), dtype=bool)
    out = [("full", full), ("empty", np.zeros((h, w), dtype=bool))]
    for name, (y, x) in (("hole in a corner", (0, w - 1)), ("hole in the middle", (h // 2, w // 2))):
        m = full.copy()
        m[y, x] = False
        out.append((name, m))
    m = np.zeros((h, w), dtype=bool)
    m[h // 2, w // 3] = True
    out.append(("one pixel", m))
    for name, (ys, xs) in (("rectangle at the top", (slice(0, max(1, 2 * h // 3)), slice(w // 5, max(w // 5 + 1, 4 * w // 5)))),
                           ("rectangle at the bottom", (slice(h // 3, h), slice(w // 5, max(w // 5 + 1, 4 * w // 5)))),
                           ("rectangle at the left", (slice(h // 5, max(h // 5 + 1, 4 * h // 5)), slice(0, max(1, 2 * w // 3)))),
                           ("rectangle at the right", (slice(h // 5, max(h // 5 + 1, 4 * h // 5)), slice(w // 3, w)))):
        m = np.zeros((h, w), dtype=bool)
        m[ys, xs] = True
        out.append((name, m))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", (yy + xx) % 2 == 0))
    out.append(("random 0.5", rng.random((h, w)) < 0.5))
    out.append(("random 0.98", rng.random((h, w)) < 0.98))
    return out


# ---- the matching ---------------------------------------------------------------------------------------------------------------------------------
def with_boundary(group: dict, seed: int) -> dict:
    """A group of tests/test_match_cpu.py with independently drawn boundary integers: areas 1 .. 40, intersections 0 .. min of the
    two, some exactly 0 and some -1 (a refused pair)."""
    rng = np.random.default_rng(seed)
    D, G = len(group["scores"]), len(group["gt_area"])
    dab, gab = rng.integers(1, 41, D), rng.integers(1, 41, G)
    ib = np.array([[rng.integers(0, min(dab[d], gab[g]) + 1) for g in range(G)] for d in range(D)], dtype=np.int64).reshape(D, G)
    kind = rng.random((D, G))
    ib[kind < 0.15] = 0
    ib[kind > 0.93] = -1
    return dict(group, inter_b=ib, det_area_b=dab, gt_area_b=gab)


def ious_min(group: dict) -> np.ndarray:
    return np.minimum(MO.ious_of(group["inter"], group["det_area"], group["gt_area"], group["iscrowd"]),
                      MO.ious_of(group["inter_b"], group["det_area_b"], group["gt_area_b"], group["iscrowd"]))


def evaluate_group(group, iou_thrs=MO.IOU_THRS, area_rngs=MO.AREA_RNGS, max_det=100, form=MO.evaluate_img):
    """match_oracle.evaluate_group with ious = min(mask IoU, boundary IoU); the area ranges keep the mask's areas."""
    ra = group["gt_area"] if group.get("range_area") is None else group["range_area"]
    ious = ious_min(group)
    return [form(ious, group["det_area"], group["scores"], ra, group["iscrowd"], rng, max_det, iou_thrs) for rng in area_rngs]


def boundary_tables(groups):
    cat = lambda key: np.concatenate([np.asarray(g[key], dtype=np.int32).reshape(-1) for g in groups] + [np.zeros(0, dtype=np.int32)])
    return dict(inter_b=cat("inter_b"), det_area_b=cat("det_area_b"), gt_area_b=cat("gt_area_b"))


def run_match(fn, groups, tabs=None, btabs=None, **kw):
    """match_oracle.run_entry on hip.coco_match_boundary / its host twin: the three boundary tables go in behind max_det."""
    import torch
    btabs = boundary_tables(groups) if btabs is None else btabs
    dev = kw.get("dev", "cpu")
    extra = [torch.from_numpy(np.ascontiguousarray(btabs[k])).to(dev) for k in ("inter_b", "det_area_b", "gt_area_b")]
    return MO.run_entry(lambda *a: fn(*a[:12], *extra, *a[12:]), MO.tables(groups) if tabs is None else tabs, **kw)


def check_groups(res, groups, iou_thrs=MO.IOU_THRS, area_rngs=MO.AREA_RNGS, max_det=100, refused=()):
    """match_oracle.check_groups against this module's evaluate_group."""
    d_off = np.concatenate([[0], np.cumsum([len(g["scores"]) for g in groups])])
    g_off = np.concatenate([[0], np.cumsum([len(g["gt_area"]) for g in groups])])
    for e, grp in enumerate(groups):
        d0, d1, g0, g1 = d_off[e], d_off[e + 1], g_off[e], g_off[e + 1]
        if e in refused:
            assert (res["dt_order"][d0:d1] == -1).all() and (res["dt_match"][:, :, d0:d1] == -1).all()
            assert (res["dt_ignore"][:, :, d0:d1] == 1).all() and (res["gt_match"][:, :, g0:g1] == -1).all()
            assert (res["gt_ignore"][:, g0:g1] == 1).all()
            continue
        want = evaluate_group(grp, iou_thrs, area_rngs, max_det)
        full = evaluate_group(grp, iou_thrs, area_rngs[:1], 1 << 30)[0]["order"]
        assert np.array_equal(res["dt_order"][d0:d1], d0 + full), e
        for a, w in enumerate(want):
            R = len(w["order"])
            assert np.array_equal(res["dt_match"][a, :, d0:d0 + R], np.where(w["dtm"] >= 0, g0 + w["dtm"], -1)), (e, a)
            assert np.array_equal(res["dt_ignore"][a, :, d0:d0 + R], w["dt_ig"].astype(np.uint8)), (e, a)
            assert (res["dt_match"][a, :, d0 + R:d1] == -1).all() and (res["dt_ignore"][a, :, d0 + R:d1] == 1).all(), (e, a)
            assert np.array_equal(res["gt_match"][a, :, g0:g1], np.where(w["gtm"] >= 0, d0 + w["gtm"], -1)), (e, a)
            assert np.array_equal(res["gt_ignore"][a, g0:g1], w["gt_ig"].astype(np.uint8)), (e, a)
