"""Thinning of sized planes from its definition, written without a look at csrc/thin_logic.h: Guo & Hall's
two-subiteration rule as Lam, Lee & Suen state it, on bool arrays, everything outside the plane clear.  Two forms: `thin` evaluates G1,
G2, G3 and G3' as written, on the eight shifted copies of the plane; `thin_lut` codes each neighbourhood as a byte with
scipy.ndimage.correlate (weights 1, 2, 4 .. 128 for x1 .. x8) and looks it up in two 256-entry tables that `lut` fills one configuration
at a time with plain Python integers.  clDice is plain loops over pixels.  Beside them the harness that runs hip.mask_thin_sized or its
host twin on lists of planes between guard bands, and the planes of the tests."""
import numpy as np

import boundary_oracle as BO

GUARD, BAND, FILL = BO.GUARD, BO.BAND, BO.FILL
SENT = -7                     # the sentinel of the int32 tables
MAX_ITER = 1 << 30
MAX_STEPS = 1024
LDS_BUDGET = 4 * 38 * 1024    # bytes of the resident kernel's bordered plane


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------
def neighbours(x: np.ndarray) -> list:
    """[None, x1 .. x8, x9 = x1] as bool arrays: counter-clockwise from east, rows growing downwards, the outside clear."""
    p = np.pad(np.asarray(x, dtype=bool), 1)
    c = slice(1, -1)
    up, down, left, right = slice(0, -2), slice(2, None), slice(0, -2), slice(2, None)
    xs = [None, p[c, right], p[up, right], p[up, c], p[up, left], p[c, left], p[down, left], p[down, c], p[down, right]]
    return xs + [xs[1]]


def subiteration(x: np.ndarray, second: bool) -> np.ndarray:
    x = np.asarray(x, dtype=bool)
    xs = neighbours(x)
    xh = sum((~xs[2 * i - 1] & (xs[2 * i] | xs[2 * i + 1])).astype(np.int64) for i in range(1, 5))
    n1 = sum((xs[2 * k - 1] | xs[2 * k]).astype(np.int64) for k in range(1, 5))
    n2 = sum((xs[2 * k] | xs[2 * k + 1]).astype(np.int64) for k in range(1, 5))
    low = np.minimum(n1, n2)
    g1, g2 = xh == 1, (low >= 2) & (low <= 3)
    g3 = ~((xs[6] | xs[7] | ~xs[4]) & xs[5]) if second else ~((xs[2] | xs[3] | ~xs[8]) & xs[1])
    return x & ~(g1 & g2 & g3)


def iteration(x: np.ndarray) -> np.ndarray:
    return subiteration(subiteration(x, False), True)


def thin(x: np.ndarray, max_iter: int = 0):
    """-> (the thinned plane, the iterations that cleared a pixel); max_iter = 0: until an iteration clears nothing."""
    x, n = np.asarray(x, dtype=bool).copy(), 0
    while max_iter == 0 or n < max_iter:
        y = iteration(x)
        if np.array_equal(x, y):
            break
        x, n = y, n + 1
    return x, n


_LUT = {}


def lut(second: bool) -> np.ndarray:
    """bool (256,): the configurations, bit i - 1 = x_i, in which the centre pixel is cleared -- one at a time, on Python integers."""
    if second not in _LUT:
        t = np.zeros(256, dtype=bool)
        for code in range(256):
            v = [None] + [(code >> i) & 1 for i in range(8)]
            v.append(v[1])
            xh = sum(1 for i in range(1, 5) if v[2 * i - 1] == 0 and (v[2 * i] == 1 or v[2 * i + 1] == 1))
            n1 = sum(v[2 * k - 1] | v[2 * k] for k in range(1, 5))
            n2 = sum(v[2 * k] | v[2 * k + 1] for k in range(1, 5))
            g3 = ((v[6] | v[7] | (1 - v[4])) & v[5]) == 0 if second else ((v[2] | v[3] | (1 - v[8])) & v[1]) == 0
            t[code] = xh == 1 and 2 <= min(n1, n2) <= 3 and g3
        _LUT[second] = t
    return _LUT[second]


def thin_lut(x: np.ndarray, max_iter: int = 0):
    """`thin` by correlation and lookup (needs scipy)."""
    from scipy import ndimage
    # correlate: out(y, x) = sum over (dy, dx) of weights[1 + dy, 1 + dx] * in(y + dy, x + dx)
    weights = np.array([[8, 4, 2], [16, 0, 1], [32, 64, 128]], dtype=np.int32)      # x4 x3 x2 / x5 . x1 / x6 x7 x8
    x, n = np.asarray(x, dtype=bool).copy(), 0
    while max_iter == 0 or n < max_iter:
        y = x
        for second in (False, True):
            code = ndimage.correlate(y.astype(np.int32), weights, mode="constant", cval=0)
            y = y & ~lut(second)[code]
        if np.array_equal(x, y):
            break
        x, n = y, n + 1
    return x, n


def components8(x: np.ndarray) -> int:
    from scipy import ndimage
    return int(ndimage.label(np.asarray(x, dtype=bool), structure=np.ones((3, 3), dtype=bool))[1])


def cldice_counts(a: np.ndarray, b: np.ndarray) -> dict:
    """|S_A|, |S_A & B|, |S_B|, |S_B & A| with S_X the plane thinned to its fixed point: plain loops."""
    sa, sb = thin(a)[0], thin(b)[0]
    out = dict(skel_a=0, skel_a_in_b=0, skel_b=0, skel_b_in_a=0)
    h, w = a.shape
    for y in range(h):
        for x in range(w):
            if sa[y, x]:
                out["skel_a"] += 1
                out["skel_a_in_b"] += 1 if b[y, x] else 0
            if sb[y, x]:
                out["skel_b"] += 1
                out["skel_b_in_a"] += 1 if a[y, x] else 0
    return out


def cldice(c: dict) -> float:
    """clDice from the four counts: both masks empty 1, exactly one empty 0, Tprec + Tsens = 0 gives 0."""
    if c["skel_a"] == 0 and c["skel_b"] == 0:
        return 1.0
    if c["skel_a"] == 0 or c["skel_b"] == 0:
        return 0.0
    tp, ts = c["skel_a_in_b"] / c["skel_a"], c["skel_b_in_a"] / c["skel_b"]
    return 0.0 if tp + ts == 0 else 2 * tp * ts / (tp + ts)


def box_of(x: np.ndarray) -> list:
    if not x.any():
        return [-1, -1, -1, -1]
    ys, xs = np.nonzero(x)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def lds_bytes(h: int, w: int) -> int:
    return 4 * (h + 2) * ((w + 31) // 32 + 2)


# ---- cvlm_mask_thin_sized on lists of planes ---------------------------------------------------------------------------------------------------
def ws_need(nbytes: int, P: int, steps: int) -> int:
    r16 = lambda v: (v + 15) // 16 * 16
    return r16(nbytes) + r16(4 * P * steps)


def run(fn, planes, max_iters, dev="cpu", mode=0, steps=64, stats=True, shift=0, outs=None, offsets=None, dims=None, dirty_pads=False):
    """One call of hip.mask_thin_sized / its host twin on `planes` (bool arrays) at `max_iters`.  bits and out_bits are sentinel-filled
    with GUARD bytes before the first and behind the last plane; the workspace lies between BAND sentinel bytes and every int32 table
    between BAND sentinel entries.  shift: bytes by which the base of bits is moved off its allocation.  outs: the tensors of an earlier
    call, used again.  offsets / dims: doctored tables (the refusal tests).  dirty_pads: the input's pad bits are set.  -> dict(planes,
    raw, area, box, iters, done, status, outs); every band is checked."""
    import torch
    sizes = [p.shape for p in planes]
    good_dims, good_off, nbytes, max_words = BO.tables(sizes)
    src = np.full(nbytes, FILL, dtype=np.uint8)
    for p, plane in enumerate(planes):
        rows = BO.pack(plane)
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
    need = ws_need(nbytes, P, steps)
    fresh = outs is None
    if fresh:
        table = lambda n: torch.full((n + 2 * BAND,), SENT, dtype=torch.int32, device=dev)
        outs = dict(out=torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev),
                    ws=torch.full((ws_need(nbytes, P, MAX_STEPS) + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    area=table(P), box=table(4 * P), iters=table(P), done=table(P),
                    status=torch.full((1,), 77, dtype=torch.int32, device=dev))
    use_off = good_off if offsets is None else np.asarray(offsets, dtype=np.int64)
    use_dims = good_dims if dims is None else np.asarray(dims, dtype=np.int32).reshape(P, 2)
    fn(bits, dv(use_off), dv(use_dims), dv(np.asarray(max_iters, dtype=np.int32)), max_words, mode, steps, outs["ws"][BAND:BAND + need],
       outs["out"], outs["area"][BAND:BAND + P] if stats else None, outs["box"][BAND:BAND + 4 * P].view(P, 4) if stats else None,
       outs["iters"][BAND:BAND + P], outs["done"][BAND:BAND + P], outs["status"])
    raw = outs["out"].cpu().numpy()
    ws = outs["ws"].cpu().numpy()
    assert (raw[:GUARD] == FILL).all() and (raw[nbytes - GUARD:] == FILL).all(), "out_bits: a guard band was written"
    assert (ws[:BAND] == FILL).all() and (ws[BAND + need:] == FILL).all(), "workspace: a guard band was written"
    tabs = {}
    for k, n in (("area", P), ("box", 4 * P), ("iters", P), ("done", P)):
        t = outs[k].cpu().numpy()
        assert (t[:BAND] == SENT).all() and (t[BAND + n:] == SENT).all(), f"out_{k}: a guard band was written"
        assert stats or not fresh or k in ("iters", "done") or (t == SENT).all(), f"out_{k} was written although it was NULL"
        tabs[k] = t[BAND:BAND + n].copy()
    got, rows_of = [], []
    for p, (h, w) in enumerate(sizes):
        rows = raw[good_off[p]:good_off[p + 1]].reshape(h, -1)
        plane, dirty = BO.unpack(rows, w)
        assert not dirty or (rows == FILL).all(), f"plane {p}: a pad bit is set"
        got.append(plane)
        rows_of.append(rows)
    return dict(planes=got, raw=rows_of, area=tabs["area"], box=tabs["box"].reshape(P, 4), iters=tabs["iters"], done=tabs["done"],
                status=int(outs["status"].cpu().numpy()[0]), outs=outs)


def check(res, planes, max_iters, want=None, refused=(), untouched=(), stats=True, done=None):
    """The outputs of `run` against the oracle, every bit and count; a refused plane is zero bytes, or -- `untouched`: its slice is no
    range of whole words inside the buffer -- the sentinel it held, with area 0, box -1, iters 0 and done 0.  want: (plane, iters) per
    plane where the caller has them already.  done: what out_done must hold (None: 1 everywhere)."""
    for p, (plane, m) in enumerate(zip(planes, max_iters)):
        if p in refused or p in untouched:
            assert (res["raw"][p] == (FILL if p in untouched else 0)).all(), p
            assert res["iters"][p] == 0 and res["done"][p] == 0, p
            assert not stats or (res["area"][p] == 0 and res["box"][p].tolist() == [-1] * 4), p
            continue
        ref, n = thin(plane, int(m)) if want is None else want[p]
        bad = res["planes"][p] != ref
        assert not bad.any(), (p, plane.shape, int(m), int(bad.sum()), np.argwhere(bad)[:3].tolist())
        assert res["iters"][p] == n, (p, plane.shape, int(res["iters"][p]), n)
        assert res["done"][p] == (1 if done is None else done[p]), (p, int(res["done"][p]))
        assert not stats or (res["area"][p] == int(ref.sum()) and res["box"][p].tolist() == box_of(ref)), (p, res["area"][p], res["box"][p])


# ---- planes -------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 129)
HEIGHTS = (1, 2, 3, 33, 130)
RAGGED = BO.RAGGED                                                    # DESIGN.md §19's seven
PATTERNS = ("empty", "full", "corners", "one clear", "row", "column", "diagonal", "checkerboard", "ring", "r0.3", "r0.5", "r0.9", "r0.98")


def contents(h: int, w: int, seed: int) -> list:
    """The issue's patterns of one size, in the order of PATTERNS."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((h, w), dtype=bool)
    yy, xx = np.mgrid[0:h, 0:w]
    corners = z()
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
        corners[y, x] = True
    hole = ~z()
    hole[h // 2, w // 2] = False
    row, col = z(), z()
    row[h // 2, :] = True
    col[:, w // 2] = True
    diag = (xx - yy == 0) | (xx - yy == 1)
    ring = z()
    ring[h // 6:h - h // 6, w // 6:w - w // 6] = True
    ring[h // 3:h - h // 3, w // 3:w - w // 3] = False
    return [z(), ~z(), corners, hole, row, col, diag, (yy + xx) % 2 == 0, ring] + [rng.random((h, w)) < d for d in (0.3, 0.5, 0.9, 0.98)]


def gpu_list():
    """(planes, max_iters) of the device tests: every width x height x pattern, max_iter 1, 2 and unlimited mixed through the list."""
    planes, max_iters = [], []
    for h in HEIGHTS:
        for w in WIDTHS:
            for i, plane in enumerate(contents(h, w, 1000 * h + w)):
                planes.append(plane)
                max_iters.append((0, 1, 2)[(len(planes) + i) % 3])
    return planes, max_iters


def limb_planes():
    """A body with four thin legs, and the same with one leg cut off: the pair clDice is meant to tell apart."""
    a = np.zeros((48, 70), dtype=bool)
    a[8:24, 10:60] = True
    for x in (14, 28, 42, 54):
        a[24:44, x:x + 3] = True
    b = a.copy()
    b[24:44, 42:45] = False
    return a, b
