"""Oracle of the masks at each image's own size (include/cvlm.h: cvlm_mask_pack_sized): oracle/metrics_oracle.py's own
`resize_linear_f32(sigmoid_f32(.))` -- imported, not copied -- `* 255 >= level`, packed row by row, an fp64 restatement of the same
taps that says where 255 v lies within rounding of the level, the comparison rule of the tests, the inputs, and the runner of the two
entries into sentinel-filled outputs with guard bands inside the same tensor.  Importable without a GPU."""
import numpy as np
import torch

from oracle import metrics_oracle as M

NEAR = 2.5e-4                 # levels: a pixel is left out of the exact comparison only where |255 v (fp64) - level| <= NEAR
GUARD = 16                    # sentinel bytes before the first and behind the last plane (offsets stay multiples of 4)
FILL = 0xA5
LEVELS = (1, 128, 254)
# (source, target) of the arithmetic cases
ARITH = [((64, 64), (97, 131)), ((96, 128), (50, 201)), ((64, 64), (33, 31)), ((64, 96), (64, 96)), ((32, 32), (1, 1)),
         ((32, 64), (70, 33)), ((320, 320), (213, 320)), ((320, 320), (480, 641))]
RAGGED = [(1, 1), (70, 33), (5, 65), (33, 31), (1, 32), (97, 131), (2, 64)]


def field(src, dst) -> np.ndarray:
    """tests/test_evaltail.py's field for a source size, seeded as there by the two sizes."""
    rng = np.random.default_rng(src[0] + dst[1])
    yy, xx = np.mgrid[0:src[0], 0:src[1]]
    return (6 * np.sin(yy / 17.0) * np.cos(xx / 23.0) + rng.normal(0, 1.5, src)).astype(np.float32)


def mask(logits: np.ndarray, h: int, w: int, level: int) -> np.ndarray:
    """f32 (Hs, Ws) -> bool (h, w): the reference's float mask * 255 >= level, all in float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = M.resize_linear_f32(M.sigmoid_f32(logits), h, w)
        return (v * np.float32(255)) >= np.float32(level)


def levels_f64(logits: np.ndarray, h: int, w: int) -> np.ndarray:
    """255 v in float64 from the same taps and the same (float32) weights: sigmoid, products and sums in double."""
    Hs, Ws = logits.shape
    x0, x1, a0, a1 = M._axis_table(Ws, w, True)
    y0, y1, b0, b1 = M._axis_table(Hs, h, False)
    with np.errstate(over="ignore", invalid="ignore"):
        p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
        rows = p[:, x0] * a0.astype(np.float64)[None, :] + p[:, x1] * a1.astype(np.float64)[None, :]
        return 255.0 * (rows[y0] * b0.astype(np.float64)[:, None] + rows[y1] * b1.astype(np.float64)[:, None])


def pack_rows(m: np.ndarray) -> np.ndarray:
    """bool (h, w) -> uint8 (h, 4 * ceil(w / 32)): every row packed on its own, pad bits 0."""
    h, w = m.shape
    wide = np.zeros((h, 32 * ((w + 31) // 32)), dtype=bool)
    wide[:, :w] = m
    return np.packbits(wide, axis=1)


def unpack_rows(rows: np.ndarray, w: int) -> np.ndarray:
    return np.unpackbits(rows, axis=1)[:, :w].astype(bool)


def stats(m: np.ndarray):
    """(area, box) under cvlm_mask_pack's conventions."""
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return 0, [-1, -1, -1, -1]
    return int(ys.size), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def tables(sizes, guard: int = GUARD):
    """-> dims int32 (P, 2), offsets int64 (P + 1) starting at `guard`, the tensor's byte length (guard behind the last plane too),
    the largest word count."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    off = np.full(len(sizes) + 1, guard, dtype=np.int64)
    off[1:] += np.cumsum(4 * words)
    return dims, off, int(off[-1]) + guard, int(words.max())


def run(entry, logits, sizes, level: int, dev="cpu", offsets=None, nbytes=None, stats_out=True):
    """One call of hip.mask_pack_sized (or its host twin) on logits (P, Hs, Ws) into ONE sentinel-filled uint8 tensor: GUARD bytes
    before the first plane and behind the last.  offsets / nbytes override the table (the refusal tests).  -> (the raw bytes, each
    plane's rows or None where its slice is no plane, area, box, status); every byte outside the planes' own slices -- the bands,
    and the slices of refused planes -- must still hold the sentinel."""
    dims, off, total, max_words = tables(sizes)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
    P = len(sizes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bits = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
    area = torch.full((P,), -7, dtype=torch.int32, device=dev) if stats_out else None
    box = torch.full((P, 4), -7, dtype=torch.int32, device=dev) if stats_out else None
    status = torch.full((1,), -3, dtype=torch.int32, device=dev)
    src = logits if isinstance(logits, torch.Tensor) else t(logits)
    use = bits if nbytes is None else bits[:nbytes]
    entry(src, t(dims), t(off), level, use, max_words, area, box, status)
    if dev != "cpu":
        torch.cuda.synchronize()
    raw = bits.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    planes = []
    limit = total if nbytes is None else nbytes
    for p, (h, w) in enumerate(sizes):
        n = 4 * h * ((w + 31) // 32)
        good = off[p] >= 0 and off[p] % 4 == 0 and off[p + 1] - off[p] == n and off[p + 1] <= limit
        if good:
            keep[off[p]:off[p + 1]] = False
            planes.append(raw[off[p]:off[p + 1]].reshape(h, -1))
        else:
            planes.append(None)
    assert (raw[keep] == FILL).all(), "a byte outside the planes was overwritten"
    return raw, planes, None if area is None else area.cpu().numpy(), None if box is None else box.cpu().numpy(), int(status.cpu().item())


def compare(rows: np.ndarray, area, box, logits: np.ndarray, h: int, w: int, level: int, exact: bool = False) -> int:
    """The rule of the tests.  rows uint8 (h, 4 ws): the pad bits are 0; a pixel may differ from the float32 oracle only where the fp64
    value of 255 v lies within NEAR of the level, and at most max(2, 1e-4 h w) pixels of a plane may be left out that way (exact: none is);
    the oracle itself agrees with the fp64 restatement everywhere else; area differs by at most the pixels left out; the box is held
    only when none were.  -> the number of pixels left out."""
    ws = (w + 31) // 32
    assert rows.shape == (h, 4 * ws) and rows.dtype == np.uint8
    wide = np.unpackbits(rows, axis=1)
    assert not wide[:, w:].any(), "pad bits"
    got = wide[:, :w].astype(bool)
    want = mask(logits, h, w, level)
    lv = levels_f64(logits, h, w)
    near = np.abs(lv - level) <= NEAR
    left = int(near.sum())
    print(f"{logits.shape} -> {(h, w)} level {level}: left out {left} of {h * w}, differing {int((got != want).sum())}, set {int(got.sum())}")
    if exact:                                                         # every bit is held: sigmoid(+-30) is 1.0f or 1e-13, nothing to leave out
        left, held = 0, np.ones((h, w), dtype=bool)                   # (level 255 meets 255.0f itself, which fp64 puts 1e-11 below)
    else:
        held = ~near
    assert left <= max(2, 1e-4 * h * w), left
    with np.errstate(invalid="ignore"):
        assert np.array_equal((lv >= level)[~near], want[~near]), "the float32 oracle against its fp64 restatement"
    assert np.array_equal(got[held], want[held]), int((got != want)[held].sum())
    if area is not None:
        a, b = stats(got)
        assert int(area) == a and list(box) == b, "area and box are those of the plane's own bits"
        assert abs(int(area) - int(want.sum())) <= left
        if left == 0:
            assert list(box) == stats(want)[1]
    return left


# ---- geometry: blocky planes of +-30, where sigmoid is 1.0f or about 1e-13 and the result depends on taps and weights alone ------------
def blocky(Hs: int, Ws: int, seed: int, block: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    coarse = rng.random((-(-Hs // block), -(-Ws // block))) < 0.5
    m = np.kron(coarse, np.ones((block, block), dtype=bool))[:Hs, :Ws]
    return np.where(m, np.float32(30), np.float32(-30)).astype(np.float32)


def single(Hs: int, Ws: int, y: int, x: int) -> np.ndarray:
    a = np.full((Hs, Ws), -30, dtype=np.float32)
    a[y, x] = 30
    return a


GEOMETRY_WIDTHS = (1, 31, 32, 33, 63, 64, 65, 97)
GEOMETRY_HEIGHTS = (1, 2, 33)
GEOMETRY_LEVELS = (1, 128, 254, 255)


def geometry_cases():
    """-> list of (name, logits (Hs, Ws), (h, w)): every width x height from a 24 x 40 blocky source, single pixels at the four source
    corners, one source row, one source column, +-inf logits, a NaN plane."""
    out = []
    for w in GEOMETRY_WIDTHS:
        for h in GEOMETRY_HEIGHTS:
            out.append((f"blocky_{h}x{w}", blocky(24, 40, 100 * h + w), (h, w)))
    for y, x in ((0, 0), (0, 39), (23, 0), (23, 39)):
        out.append((f"corner_{y}_{x}_up", single(24, 40, y, x), (33, 65)))
        out.append((f"corner_{y}_{x}_down", single(24, 40, y, x), (7, 31)))
    out.append(("one_row", blocky(1, 40, 7), (33, 97)))
    out.append(("one_column", blocky(24, 1, 8), (33, 33)))
    inf = blocky(24, 40, 9)
    inf = np.where(inf > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    out.append(("inf", inf, (33, 65)))
    out.append(("nan", np.full((24, 40), np.nan, dtype=np.float32), (33, 65)))
    return out


# ---- run-length encoding with a true width -----------------------------------------------------------------------------------------------
RLE_SIZES = [(1, 1), (1, 31), (8, 33), (33, 31), (32, 63), (33, 65), (65, 97)]


def rle_cases(H: int, Wt: int) -> dict:
    rng = np.random.default_rng(1000 * H + Wt)
    z = lambda: np.zeros((H, Wt), dtype=bool)
    out = {"empty": z(), "full": ~z(), "last_pixel": z(), "first_pixel": z()}
    out["last_pixel"][H - 1, Wt - 1] = True
    out["first_pixel"][0, 0] = True
    out["checker"] = (np.add.outer(np.arange(H), np.arange(Wt)) & 1).astype(bool)
    for d in (0.01, 0.5, 0.99):
        out[f"random_{d}"] = rng.random((H, Wt)) < d
    return out


def pack_planes(planes: np.ndarray, garbage: bool = False, seed: int = 0) -> np.ndarray:
    """bool (P, H, Wt) -> uint8 (P, H * 4 ws) of padded rows; garbage: random pad bits in place of zeros."""
    P, H, Wt = planes.shape
    W = 32 * ((Wt + 31) // 32)
    wide = np.zeros((P, H, W), dtype=bool)
    if garbage:
        wide[:] = np.random.default_rng(seed).random((P, H, W)) < 0.5
    wide[:, :, :Wt] = planes
    return np.packbits(wide.reshape(P, -1), axis=1)
