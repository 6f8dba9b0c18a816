"""Rendering restated in numpy: the blend rule, the three layer kinds, demo.py:51-56, one ragged scene and the exhaustive
(c, col) table; and the runners that hand a scene to cvlm_render / cvlm_debug_render_host with garbage-filled, guarded outputs.

The blend is float32 step by step -- numpy rounds every product and the sum on its own -- then np.rint (half to even) and a clip.  cv2 is
not needed: at alpha 0.5 the rule is cv2.addWeighted's documented saturate(round((c + col) / 2)), which `demo_overlay` writes in float64."""
import numpy as np
import torch

BITS, LEVELS, LABELS = 0, 1, 2
EDGES, INVERT = 1, 2
GUARD, GARBAGE = 64, 0xA5
ALPHAS = [0.0, 0.25, 0.3, 0.5, 0.7, 1.0]                               # of the exhaustive (c, col) table
SIZES = [(1, 1), (2, 3), (7, 5), (3, 31), (2, 32), (5, 33), (4, 37), (3, 65)]


def blend(c, col, a):
    """uint8 c and col, float32 a, broadcast against each other -> uint8."""
    a = np.asarray(a, dtype=np.float32)
    b = np.float32(1.0) - a
    p = np.asarray(c).astype(np.float32) * b
    q = np.asarray(col).astype(np.float32) * a
    return np.clip(np.rint(p + q), 0, 255).astype(np.uint8)


def demo_overlay(image: np.ndarray, mask: np.ndarray, color=(0, 255, 0)) -> np.ndarray:
    """demo.py:51-56: overlay = image.copy(); overlay[mask] = color; cv2.addWeighted(image, 0.5, overlay, 0.5, 0) -- on uint8 that is
    saturate(round half to even(image * 0.5 + overlay * 0.5)), formed here in float64 where every step is exact."""
    overlay = image.copy()
    overlay[mask] = color
    return np.clip(np.rint(image.astype(np.float64) * 0.5 + overlay.astype(np.float64) * 0.5), 0, 255).astype(np.uint8)


def pack_rows(mask: np.ndarray, dirty: bool = False) -> np.ndarray:
    """A bool (h, w) mask as the bytes of a sized plane: rows of ceil(w / 32) words in numpy.packbits' order; dirty: every pad bit 1."""
    h, w = mask.shape
    ws = (w + 31) // 32
    full = np.full((h, 32 * ws), dirty, dtype=bool)
    full[:, :w] = mask
    return np.packbits(full, axis=1).reshape(-1)


def image_tables(sizes):
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    nbytes = (3 * dims[:, 0].astype(np.int64) * dims[:, 1] + 3) // 4 * 4
    return dims, np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)


def image_of(sc, flat: np.ndarray, b: int) -> np.ndarray:
    h, w = sc["sizes"][b]
    lo = int(sc["img_offsets"][b])
    return flat[lo:lo + 3 * h * w].reshape(h, w, 3)


def edges_of(ids: np.ndarray) -> np.ndarray:
    e = np.zeros(ids.shape, dtype=bool)
    e[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    e[:, :-1] |= ids[:, :-1] != ids[:, 1:]
    e[1:, :] |= ids[1:, :] != ids[:-1, :]
    e[:-1, :] |= ids[:-1, :] != ids[1:, :]
    return e


def paint(sc, im: np.ndarray, row) -> np.ndarray:
    """One layer over one (h, w, 3) image -> the new image."""
    kf, src, first, rows = (int(v) for v in row)
    kind, flags = kf & 0xff, kf >> 8
    h, w = im.shape[:2]
    if kind == BITS:
        ws = (w + 31) // 32
        m = np.unpackbits(sc["bits"][src:src + 4 * h * ws].reshape(h, 4 * ws), axis=1)[:, :w].astype(bool)
        sel = ~m if flags & INVERT else m
        idx = np.full((h, w), first)
    elif kind == LEVELS:
        sel = np.ones((h, w), dtype=bool)
        idx = first + sc["levels"][src:src + h * w].reshape(h, w).astype(np.int64)
    else:
        ids = sc["labels"][src:src + h * w].reshape(h, w)
        sel = (ids >= 0) & (ids < rows)
        if flags & EDGES:
            sel &= edges_of(ids)
        idx = first + np.where(sel, ids, 0).astype(np.int64)
    out = blend(im, sc["rgb"][idx], sc["alpha"][idx][..., None])
    return np.where(sel[..., None], out, im)


def render_oracle(sc, skip=(), refused=()) -> np.ndarray:
    """The whole output buffer the entry must leave: garbage where nothing is written (pad bytes, refused images), every other image
    with its layers applied in order; `skip`: layer rows taken as absent."""
    out = np.full(sc["img"].size, GARBAGE, dtype=np.uint8)
    for b in range(len(sc["sizes"])):
        if b in refused:
            continue
        im = image_of(sc, sc["img"], b).copy()
        for l in range(int(sc["layer_offsets"][b]), int(sc["layer_offsets"][b + 1])):
            if l not in skip:
                im = paint(sc, im, sc["layers"][l])
        image_of(sc, out, b)[...] = im
    return out


class _Builder:
    """Source buffers and the colour table of a scene, each started with a few bytes of junk so that no src is 0."""

    def __init__(self, rng):
        self.rng = rng
        self.bits, self.levels, self.labels = [np.full(4, 0xff, np.uint8)], [np.full(3, 7, np.uint8)], [np.full(1, 5, np.int32)]
        self.rgb, self.alpha, self.rows = [np.array([[9, 9, 9]], np.uint8)], [np.float32([0.25])], []

    def _table(self, rgb, alpha):
        first = sum(len(a) for a in self.alpha)
        self.rgb.append(np.asarray(rgb, np.uint8).reshape(-1, 3))
        self.alpha.append(np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float32), self.rgb[-1].shape[:1])))
        return first

    def fill(self, mask, color, alpha, invert=False):
        src = sum(a.size for a in self.bits)
        self.bits.append(pack_rows(mask, dirty=True))
        self.rows.append((BITS | (INVERT if invert else 0) << 8, src, self._table(color, [alpha]), 1))

    def heat(self, levels, lut, alpha):
        src = sum(a.size for a in self.levels)
        self.levels.append(levels.astype(np.uint8).reshape(-1))
        self.rows.append((LEVELS, src, self._table(lut, alpha), 256))

    def classes(self, ids, pal, alpha, edges=False):
        src = sum(a.size for a in self.labels)
        self.labels.append(ids.astype(np.int32).reshape(-1))
        self.rows.append((LABELS | (EDGES if edges else 0) << 8, src, self._table(pal, alpha), len(pal)))


def _finish(sizes, images, per_image, bld) -> dict:
    dims, offsets = image_tables(sizes)
    img = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for b, im in enumerate(images):
        img[int(offsets[b]):int(offsets[b]) + im.size] = im.reshape(-1)
    return dict(sizes=list(sizes), dims=dims, img_offsets=offsets, img=img, max_pixels=int((dims[:, 0].astype(np.int64) * dims[:, 1]).max()),
                layer_offsets=np.concatenate([[0], np.cumsum(per_image)]).astype(np.int32),
                layers=np.asarray(bld.rows, dtype=np.int64).reshape(-1, 4), bits=np.concatenate(bld.bits), levels=np.concatenate(bld.levels),
                labels=np.concatenate(bld.labels), rgb=np.concatenate(bld.rgb), alpha=np.concatenate(bld.alpha))


def scene(seed: int = 31) -> dict:
    """The ragged scene of DESIGN.md §31: widths that make 4-pixel runs straddle row ends (3, 5, 31, 33, 37, 65) and word ends (33, 37,
    65), an image without layers, one with all three kinds, INVERT and EDGES, two overlapping fills whose order matters, alphas 0 and
    1, every pad bit of every plane 1, ids -1, rows and 2^31 - 1, EDGES pixels on all four borders."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    bld, per_image = _Builder(rng), []
    mask = lambda b, p=0.5: rng.random(SIZES[b]) < p
    count = lambda: len(bld.rows)

    def ids_of(b, n):
        ids = rng.integers(0, n, SIZES[b]).astype(np.int32)
        flat = ids.reshape(-1)
        flat[rng.permutation(flat.size)[:3]] = [-1, n, 2 ** 31 - 1]  # void ids: below, at and far above the table
        return ids

    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    lut_alpha = rng.random(256).astype(np.float32)
    lut_alpha[::7], lut_alpha[3::7] = 0.0, 1.0
    pal = rng.integers(0, 256, (6, 3), dtype=np.uint8)
    for b in range(len(SIZES)):
        n0 = count()
        if b == 0:
            bld.fill(np.ones((1, 1), bool), (0, 255, 0), 0.5)
        elif b == 2:                                                  # all three kinds
            bld.heat(rng.integers(0, 256, SIZES[b]), lut, lut_alpha)
            bld.fill(mask(b), (200, 10, 30), 0.3, invert=True)
            bld.classes(ids_of(b, 6), pal, [0.7, 0.0, 1.0, 0.5, 0.25, 0.7])
            bld.classes(ids_of(b, 3), pal[:3], 1.0, edges=True)
        elif b == 3:                                                  # the order matters: alpha 1, then 0.5 over a part of it
            m = mask(b, 0.7)
            bld.fill(m, (255, 0, 0), 1.0)
            bld.fill(m & mask(b, 0.6) | mask(b, 0.1), (0, 0, 255), 0.5)
        elif b == 4:
            bld.fill(mask(b), (1, 2, 3), 0.7)
            bld.fill(mask(b), (250, 251, 252), 0.25, invert=True)
        elif b == 5:
            bld.fill(mask(b), (0, 255, 0), 0.5)
            bld.classes(ids_of(b, 6), pal, 0.7)
        elif b == 6:
            bld.heat(rng.integers(0, 256, SIZES[b]), lut, 0.3)
            bld.fill(mask(b), (77, 77, 77), 0.0)
            bld.fill(mask(b), (12, 200, 99), 1.0)
        elif b == 7:
            bld.fill(mask(b), (0, 255, 0), 0.5)
            bld.classes(ids_of(b, 4), pal[:4], 1.0, edges=True)
        per_image.append(count() - n0)
    return _finish(SIZES, images, per_image, bld)


def table_scene(a: float) -> dict:
    """All 65 536 (c, col) pairs at one alpha: a 256 x 256 image with c = the row index in all channels under one LEVELS layer with v =
    the column and rgb[v] = (v, v, v)."""
    c = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    bld = _Builder(None)
    v = np.arange(256, dtype=np.uint8)
    bld.heat(np.repeat(v[None, :], 256, axis=0), np.stack([v, v, v], axis=1), np.full(256, a, np.float32))
    return _finish([(256, 256)], [np.stack([c, c, c], axis=2)], [1], bld)


def run(hip, sc, dev=None, in_place: bool = False, **over) -> dict:
    """One call of cvlm_render (dev) or cvlm_debug_render_host (dev None) on the scene, tables overridden by `over` (a None source goes
    as NULL) -> dict(out, status, bands): the output buffer pre-filled with garbage -- with the images for in_place -- between two guard
    bands of 64 bytes, and whether the bands are intact."""
    t = dict(sc, **over)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev or "cpu")
    n = t["img"].size
    guarded = np.full(n + 2 * GUARD, GARBAGE, dtype=np.uint8)
    if in_place:
        guarded[GUARD:GUARD + n] = t["img"]
    guarded = to(guarded)
    out = guarded[GUARD:GUARD + n]
    status = to(np.full(1, -1, np.int32))
    layers = to(t["layers"]) if len(t["layers"]) else None
    hip.render(out if in_place else to(t["img"]), to(t["img_offsets"]), to(t["dims"]), t["max_pixels"], to(t["layer_offsets"]), layers,
               to(t["bits"]), to(t["levels"]), to(t["labels"]), to(t["rgb"]), to(t["alpha"]), out, status, host=dev is None)
    g = guarded.cpu().numpy()
    bands = bool((g[:GUARD] == GARBAGE).all() and (g[GUARD + n:] == GARBAGE).all())
    return dict(out=g[GUARD:GUARD + n].copy(), status=int(status.cpu().item()), bands=bands)


def in_place_expected(sc, **kw) -> np.ndarray:
    """render_oracle for an in-place call: what is not written holds the input's bytes."""
    want = render_oracle(sc, **kw)
    untouched = np.ones(want.size, dtype=bool)
    refused = kw.get("refused", ())
    for b, (h, w) in enumerate(sc["sizes"]):
        if b not in refused:
            lo = int(sc["img_offsets"][b])
            untouched[lo:lo + 3 * h * w] = False
    return np.where(untouched, sc["img"], want)


def refusal_cases(sc):
    """(name, overrides, status, layers taken as absent, images refused) for every refusal of the contract."""
    L, T = len(sc["layers"]), len(sc["alpha"])
    rows = sc["layers"]
    first_of = lambda kind, flags=0: next(l for l, r in enumerate(rows) if int(r[0]) == kind | flags << 8)
    fill_l, heat_l, cls_l, edge_l = first_of(BITS), first_of(LEVELS), first_of(LABELS), first_of(LABELS, EDGES)
    cases = []

    def layer(name, l, col, value, **more):
        t = rows.copy()
        t[l, col] = value
        cases.append((name, dict(layers=t, **more), 2, (l,), ()))

    def image(name, b, **over):
        cases.append((name, over, 1, (), (b,)))

    dims = lambda b, h, w: dict(dims=np.concatenate([sc["dims"][:b], [[h, w]], sc["dims"][b + 1:]]).astype(np.int32))
    image("h = 0", 2, **dims(2, 0, 5))
    image("w above 16384", 2, **dims(2, 1, 16385))
    image("h negative", 0, **dims(0, -1, 1))
    off = sc["img_offsets"]
    shift = lambda b, d: dict(img_offsets=np.concatenate([off[:b], [off[b] + d], off[b + 1:]]).astype(np.int64))
    cases.append(("an offset off a multiple of 4", shift(3, 2), 1, (), (2, 3)))
    cases.append(("offsets that run backwards", shift(4, -400), 1, (), (3, 4)))          # image 3 ends before it starts, image 4 is too long
    image("a slice that leaves img_bytes", 7, **shift(8, 4))
    cases.append(("a slice too short for 3 h w", shift(7, -4), 1, (), (6, 7)))
    lo = sc["layer_offsets"]
    lshift = lambda b, v: dict(layer_offsets=np.concatenate([lo[:b], [v], lo[b + 1:]]).astype(np.int32))
    image("a layer range that runs backwards", 7, **lshift(8, int(lo[7]) - 1))
    image("a layer range that leaves L", 7, **lshift(8, L + 1))
    image("a negative layer offset", 0, **lshift(0, -1))
    layer("an unknown kind", fill_l, 0, 3)
    layer("an unknown flag", fill_l, 0, BITS | 4 << 8)
    layer("EDGES on BITS", fill_l, 0, BITS | EDGES << 8)
    layer("INVERT on LEVELS", heat_l, 0, LEVELS | INVERT << 8)
    layer("INVERT on LABELS", cls_l, 0, LABELS | INVERT << 8)
    layer("a negative kind word", cls_l, 0, -1)
    layer("a NULL bits", fill_l, 1, rows[fill_l, 1])
    cases[-1] = ("a NULL bits", dict(bits=None), 2, tuple(l for l, r in enumerate(rows) if int(r[0]) & 0xff == BITS), ())
    cases.append(("a NULL levels", dict(levels=None), 2, tuple(l for l, r in enumerate(rows) if int(r[0]) & 0xff == LEVELS), ()))
    cases.append(("a NULL labels", dict(labels=None), 2, tuple(l for l, r in enumerate(rows) if int(r[0]) & 0xff == LABELS), ()))
    layer("a negative src", fill_l, 1, -4)
    layer("a BITS src off a multiple of 4", fill_l, 1, rows[fill_l, 1] + 2)
    layer("a BITS slice that does not fit", fill_l, 1, sc["bits"].size)
    layer("a LEVELS slice that does not fit", heat_l, 1, sc["levels"].size - 3)
    layer("a LABELS slice that does not fit", edge_l, 1, sc["labels"].size - 1)
    layer("a src beyond 2^62", cls_l, 1, 2 ** 62)
    layer("a negative first", fill_l, 2, -1)
    layer("first + rows beyond T", heat_l, 2, T - 255)
    layer("first beyond T", fill_l, 2, T + 1)
    layer("rows beyond T", cls_l, 3, T + 1)
    layer("negative rows", cls_l, 3, -1)
    layer("BITS with two rows", fill_l, 3, 2)
    layer("LEVELS with 255 rows", heat_l, 3, 255)
    for bad in (np.nan, -0.001, 1.001, np.inf):
        a = sc["alpha"].copy()
        a[int(rows[fill_l, 2])] = bad
        cases.append((f"a fill's alpha {bad}", dict(alpha=a), 4, (fill_l,), ()))
    return cases
