"""Oracle of COCO annotations on the device (include/cvlm.h: cvlm_mask_rle_decode, cvlm_mask_inter_sized): decoding is
the definition in camouflaged_vlm_amd/rle.py (`decode`), held here against a plain pixel loop; an intersection is unpackbits, `&`, sum;
the IoU is pycocotools' rleIou written out in numpy.  pycocotools is not a dependency of this project: the definition is the reference.
The runners put every output into sentinel-filled tensors with guard bands and check the bands.  Importable without a GPU."""
import numpy as np
import torch

import sized_oracle as SO

GUARD = 16                    # sentinel bytes before the first and behind the last plane
FILL = 0xA5
WORD_GUARD = 3                # sentinel elements around area, box, inter and the counts
SHAPES = [(1, 1), (1, 31), (1, 32), (8, 33), (33, 31), (32, 63), (33, 65), (65, 97), (130, 517)]
INTER_SHAPES = [(1, 1), (1, 32), (33, 31), (97, 131), (480, 641)]


def decode_loop(counts, h: int, w: int) -> np.ndarray:
    """Run counts -> bool (h, w) by a pixel loop: walk the columns, the value flips at the end of every run."""
    out = np.zeros((h, w), dtype=bool)
    j, value = 0, False
    for c in counts:
        for _ in range(int(c)):
            out[j % h, j // h] = value
            j += 1
        value = not value
    assert j == h * w
    return out


def planes(h: int, w: int) -> dict:
    """The decode cases on a plane of h x w: name -> bool (h, w)."""
    rng = np.random.default_rng(1000 * h + w)
    z = lambda: np.zeros((h, w), dtype=bool)
    out = {"empty": z(), "full": ~z(), "first_pixel": z(), "last_pixel": z()}
    out["first_pixel"][0, 0] = True
    out["last_pixel"][h - 1, w - 1] = True
    out["checker"] = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)
    out["stripes_down"] = np.broadcast_to((np.arange(h) & 1).astype(bool)[:, None], (h, w)).copy()     # period 2 down a column: most counts
    out["stripes_across"] = np.broadcast_to((np.arange(w) & 1).astype(bool)[None, :], (h, w)).copy()
    for d in (0.01, 0.5, 0.99):
        out[f"random_{d}"] = rng.random((h, w)) < d
    return out


def with_zeros(counts: np.ndarray, kind: str, seed: int) -> np.ndarray:
    """Counts with zero counts inserted at a random place: "one", "two" or "three" in a row, or a "trailing" 0.  The sum stays; the
    plane they describe is whatever the definition says -- an odd number of zeros flips what follows."""
    rng = np.random.default_rng(seed)
    c = [int(v) for v in counts]
    if kind == "trailing":
        return np.asarray(c + [0], dtype=np.int64)
    at = int(rng.integers(0, len(c) + 1))
    return np.asarray(c[:at] + [0] * {"one": 1, "two": 2, "three": 3}[kind] + c[at:], dtype=np.int64)


ZERO_KINDS = ("one", "two", "three", "trailing")


def expected(counts, h: int, w: int):
    """The definition's plane, or None where the definition refuses the counts."""
    from camouflaged_vlm_amd import rle
    try:
        return rle.decode(counts, h, w)
    except ValueError:
        return None


def guarded(n_shape, dev, dtype=torch.int32, fill=-7):
    """A sentinel-filled tensor with WORD_GUARD elements (rows) around the view that is handed out -> (whole, view)."""
    shape = (n_shape,) if isinstance(n_shape, int) else tuple(n_shape)
    whole = torch.full((shape[0] + 2 * WORD_GUARD,) + shape[1:], fill, dtype=dtype, device=dev)
    return whole, whole[WORD_GUARD:WORD_GUARD + shape[0]]


def bands_whole(whole: torch.Tensor, fill=-7) -> bool:
    w = whole.cpu()
    return bool((w[:WORD_GUARD] == fill).all()) and bool((w[-WORD_GUARD:] == fill).all())


def run_decode(entry, items, dev="cpu", *, guard: int = GUARD, run_offsets=None, total=None, bit_offsets=None, nbytes=None,
               max_pixels=None, ws_planes=None, stats=True, dims=None):
    """One call of hip.mask_rle_decode (or its host twin) for items = [(counts, h, w), ...] into ONE sentinel-filled uint8 tensor with
    `guard` bytes before the first plane and behind the last.  The counts lie in one tensor with WORD_GUARD elements of -9 before and
    behind them.  run_offsets / total / bit_offsets / nbytes / max_pixels / dims override the tables (the refusal tests); ws_planes: the
    workspace holds that many planes.  -> (each plane's rows or None where its slice is no plane, area, box, status); every byte outside
    the planes' own slices and every band around area and box must still hold the sentinel."""
    from camouflaged_vlm_amd import hip
    P = len(items)
    sizes = [(h, w) for _, h, w in items]
    d, off, nb, _ = SO.tables(sizes, guard)
    if dims is not None:
        d = np.asarray(dims, dtype=np.int32).reshape(-1, 2)
    if bit_offsets is not None:
        off = np.asarray(bit_offsets, dtype=np.int64)
    flat = np.concatenate([np.full(WORD_GUARD, -9, dtype=np.int64)] + [np.asarray(c, dtype=np.int64) for c, _, _ in items]
                          + [np.full(WORD_GUARD, -9, dtype=np.int64)])
    assert np.abs(flat).max() < 2 ** 31
    ro = np.zeros(P + 1, dtype=np.int64)
    ro[1:] = np.cumsum([len(c) for c, _, _ in items])
    ro += WORD_GUARD
    if run_offsets is not None:
        ro = np.asarray(run_offsets, dtype=np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    counts = t(flat.astype(np.int32))
    counts = counts if total is None else counts[:total]
    bits = torch.full((nb,), FILL, dtype=torch.uint8, device=dev)
    area_all, area = guarded(P, dev) if stats else (None, None)
    box_all, box = guarded((P, 4), dev) if stats else (None, None)
    status = torch.full((1,), -3, dtype=torch.int32, device=dev)
    mp = max(h * w for h, w in sizes) if max_pixels is None else max_pixels
    use = bits if nbytes is None else bits[:nbytes]
    if dev == "cpu":
        entry(counts, t(ro), t(d), t(off), mp, use, area, box, status)
    else:
        ws = torch.empty(hip.mask_rle_decode_workspace_bytes(P if ws_planes is None else ws_planes, mp), dtype=torch.uint8, device=dev)
        entry(counts, t(ro), t(d), t(off), mp, use, area, box, status, ws)
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
    assert (raw[keep] == FILL).all(), "a byte outside the planes was overwritten"
    if stats:
        assert bands_whole(area_all) and bands_whole(box_all), "an element outside area / box was overwritten"
    return out, None if area is None else area.cpu().numpy(), None if box is None else box.cpu().numpy(), int(status.cpu().item())


def check_plane(rows, area, box, want, h: int, w: int):
    """A decoded plane = the definition: every bit, the pad bits 0, area and box; want None: a refused plane -- zero, area 0, box -1."""
    m = np.zeros((h, w), dtype=bool) if want is None else want
    assert rows.shape == (h, 4 * ((w + 31) // 32))
    assert np.array_equal(rows, SO.pack_rows(m)), int((np.unpackbits(rows, axis=1) != np.unpackbits(SO.pack_rows(m), axis=1)).sum())
    if area is not None:
        a, b = SO.stats(m)
        assert int(area) == a and list(box) == b


# ---- intersections ------------------------------------------------------------------------------------------------------------------------
def pack_sized(ms, garbage: bool = False, seed: int = 0, guard: int = GUARD):
    """bool planes of any sizes -> (uint8 bytes of a sized tensor with `guard` sentinel bytes at both ends, dims, offsets, largest word
    count); garbage: random pad bits in place of zeros."""
    rng = np.random.default_rng(seed)
    d, off, nb, max_words = SO.tables([m.shape for m in ms], guard)
    raw = np.full(nb, FILL, dtype=np.uint8)
    for p, m in enumerate(ms):
        h, w = m.shape
        wide = rng.random((h, 32 * ((w + 31) // 32))) < 0.5 if garbage else np.zeros((h, 32 * ((w + 31) // 32)), dtype=bool)
        wide[:, :w] = m
        raw[off[p]:off[p + 1]] = np.packbits(wide, axis=1).reshape(-1)
    return raw, d, off, max_words


def inter_oracle(A, B, pairs) -> np.ndarray:
    """unpackbits, &, sum -- on the bool planes themselves; -1 for a pair that is out of range or of two sizes."""
    out = []
    for a, b in pairs:
        if not (0 <= a < len(A) and 0 <= b < len(B)) or A[a].shape != B[b].shape:
            out.append(-1)
        else:
            out.append(int((A[a] & B[b]).sum()))
    return np.asarray(out, dtype=np.int64)


def run_inter(entry, A, B, pairs, dev="cpu", *, garbage=False, a_tables=None, b_tables=None, max_words=None):
    """One call of hip.mask_inter_sized (or its host twin): A and B lists of bool planes, B None: the same tensors serve as both.
    a_tables / b_tables = (dims, offsets, nbytes) override the tables (the refusal tests) -> (inter, status)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ra, da, oa, wa = pack_sized(A, garbage, seed=1)
    ta = [t(ra), t(oa), t(da)]
    if B is None:
        tb, wb = list(ta), wa
    else:
        rb, db, ob, wb = pack_sized(B, garbage, seed=2)
        tb = [t(rb), t(ob), t(db)]
    for tabs, over in ((ta, a_tables), (tb, b_tables)):
        if over is not None:
            dims, offs, nbytes = over
            tabs[2] = tabs[2] if dims is None else t(np.asarray(dims, dtype=np.int32).reshape(-1, 2))
            tabs[1] = tabs[1] if offs is None else t(np.asarray(offs, dtype=np.int64))
            tabs[0] = tabs[0] if nbytes is None else tabs[0][:nbytes]
    pr = t(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    whole, inter = guarded(pr.shape[0], dev)
    status = torch.full((1,), -3, dtype=torch.int32, device=dev)
    entry(ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], pr, max(wa, wb) if max_words is None else max_words, inter, status)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bands_whole(whole), "an element outside inter was overwritten"
    return inter.cpu().numpy().astype(np.int64), int(status.cpu().item())


def iou_formula(inter, area_a, area_b, crowd) -> np.ndarray:
    """pycocotools' rleIou, element by element."""
    out = []
    for i, a, b, c in zip(inter, area_a, area_b, crowd):
        if i < 0:
            out.append(-1.0)
        elif i == 0:
            out.append(0.0)
        else:
            out.append(float(i) / float(a if c else a + b - i))
    return np.asarray(out, dtype=np.float64)


def inter_planes(h: int, w: int) -> list:
    """Planes of one size for the intersection cases: random densities, two disjoint halves, a full and an empty one."""
    rng = np.random.default_rng(7 * h + w)
    out = [rng.random((h, w)) < d for d in (0.05, 0.5, 0.95)]
    left = np.zeros((h, w), dtype=bool)
    left[:, :max(1, w // 2)] = w > 1
    out += [left, ~left, np.ones((h, w), dtype=bool), np.zeros((h, w), dtype=bool)]
    return out


def disc(h: int, w: int, cy: float, cx: float, r: float) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
