"""Oracle of mask NMS on the device (include/cvlm.h: cvlm_mask_nms_inter, cvlm_mask_nms), in plain numpy: unpackbits,
box-restricted `&` and sum, the textbook greedy loop, and the Matrix NMS formulas (Wang et al., SOLOv2, §3.3) in float64 -- plus the one
ragged scene every test of the feature runs, and the runner of the two entries on host or device tensors."""
from __future__ import annotations

import numpy as np
import torch

GUARD = 64                        # int32 words in front of and behind `inter`
FILL = -7
MEASURES = {"iou": 0, "min": 1}
METHODS = {"greedy": 0, "linear": 1, "gaussian": 2}
BELOW_HALF = float(np.nextafter(0.5, 0.0))


# ---- sized planes ------------------------------------------------------------------------------------------------------------------------
def pack_rows(plane: np.ndarray, dirty: bool = False, seed: int = 0) -> np.ndarray:
    """A bool plane (h, w) as the bytes of a sized plane: rows of ceil(w / 32) words in numpy.packbits' order; dirty: the pad bits set
    at random."""
    h, w = plane.shape
    ws = (w + 31) // 32
    full = np.zeros((h, 32 * ws), bool)
    full[:, :w] = plane
    if dirty:
        full[:, w:] = np.random.default_rng(seed).random((h, 32 * ws - w)) < 0.7
    return np.packbits(full, axis=1).reshape(-1)


def tables(sizes):
    dims = np.asarray(sizes, np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(4 * words, out=off[1:])
    return dims, off


def stats(plane: np.ndarray):
    ys, xs = np.nonzero(plane)
    if ys.size == 0:
        return 0, (-1, -1, -1, -1)
    return int(ys.size), (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def unpack(flat: np.ndarray, h: int, w: int) -> np.ndarray:
    """The bytes of a sized plane with its pad columns: bool (h, 32 ws)."""
    return np.unpackbits(flat.reshape(h, -1), axis=1).astype(bool)


def groups_of(image):
    """member, group_offsets, pair_offsets of one group per image id, sorted ids, the caller's order inside: what nms_request builds."""
    rows = {}
    for q, b in enumerate(image):
        rows.setdefault(int(b), []).append(q)
    keys = sorted(rows)
    D = [len(rows[k]) for k in keys]
    member = np.asarray([q for k in keys for q in rows[k]], np.int32)
    goff = np.concatenate([[0], np.cumsum(D)]).astype(np.int32)
    poff = np.concatenate([[0], np.cumsum([d * (d - 1) // 2 for d in D])]).astype(np.int64)
    return keys, member, goff, poff


def pair_at(i: int, j: int, D: int) -> int:
    return i * D - i * (i + 1) // 2 + (j - i - 1)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def inter_pair(bits_a: np.ndarray, box_a, area_a, bits_b: np.ndarray, box_b, area_b, h: int, w: int) -> int:
    """Set pixels of A & B inside the intersection of the two boxes, from the stored bytes (pad bits and all)."""
    if area_a < 1 or area_b < 1 or tuple(box_a) == (-1,) * 4 or tuple(box_b) == (-1,) * 4:
        return 0
    x0, y0 = max(box_a[0], box_b[0]), max(box_a[1], box_b[1])
    x1, y1 = min(box_a[2], box_b[2]), min(box_a[3], box_b[3])
    if x0 > x1 or y0 > y1:
        return 0
    a, b = unpack(bits_a, h, w), unpack(bits_b, h, w)
    return int((a[y0:y1 + 1, x0:x1 + 1] & b[y0:y1 + 1, x0:x1 + 1]).sum())


def inter_oracle(sc: dict) -> np.ndarray:
    """Every group's triangle.  Groups of more than 16 instances have true boxes (asserted), where the box-restricted count is the whole
    intersection: one integer matrix product of the unpacked planes."""
    flat, off, dims, area, box = sc["bits"], sc["offsets"], sc["dims"], sc["area"], sc["box"]
    member, goff, poff = sc["member"], sc["group_offsets"], sc["pair_offsets"]
    out = np.full(int(poff[-1]), FILL, np.int32)
    for g in range(len(goff) - 1):
        rows = member[goff[g]:goff[g + 1]]
        D = len(rows)
        if D < 2:
            continue
        h, w = (int(v) for v in dims[rows[0]])
        iu = np.triu_indices(D, 1)                                    # row-major: (0, 1), (0, 2) ... -- the triangle's order
        if D > 16:
            X = np.stack([unpack(flat[off[r]:off[r + 1]], h, w)[:, :w].reshape(-1) for r in rows]).astype(np.int32)
            for k, r in enumerate(rows):
                assert stats(X[k].reshape(h, w).astype(bool)) == (int(area[r]), tuple(int(v) for v in box[r]))
            out[poff[g]:poff[g + 1]] = (X @ X.T)[iu]
        else:
            for i, j in zip(*iu):
                a, b = rows[i], rows[j]
                out[poff[g] + pair_at(i, j, D)] = inter_pair(flat[off[a]:off[a + 1]], box[a], area[a], flat[off[b]:off[b + 1]], box[b], area[b], h, w)
    return out


def measure_matrix(tri: np.ndarray, area: np.ndarray, cat, measure: str) -> np.ndarray:
    """m(i, j) of one group as a symmetric float64 (D, D) (the diagonal is not used)."""
    D = len(area)
    I = np.zeros((D, D), np.int64)
    iu = np.triu_indices(D, 1)
    I[iu] = tri
    I = I + I.T
    a = area.astype(np.int64)
    den = (a[:, None] + a[None, :] - I) if measure == "iou" else np.minimum(a[:, None], a[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        m = I.astype(np.float64) / den.astype(np.float64)
    m = np.where(I == 0, 0.0, np.where((I < 0) | (den < 1), -1.0, m))
    if cat is not None:
        m = np.where(cat[:, None] != cat[None, :], 0.0, m)
    return m


def rank(scores: np.ndarray) -> np.ndarray:
    """Score descending, equal scores in member order, NaN behind every number."""
    return np.argsort(-scores.astype(np.float32), kind="mergesort")


def nms_oracle(sc: dict, inter: np.ndarray, *, measure="iou", method="greedy", thr=0.5, sigma=2.0, class_aware=False, scores=None) -> dict:
    Q, member, goff, poff = len(sc["area"]), sc["member"], sc["group_offsets"], sc["pair_offsets"]
    G = len(goff) - 1
    scores = sc["scores"] if scores is None else scores
    out = dict(order=np.full(Q, -1, np.int32), keep=np.zeros(Q, np.uint8), by=np.full(Q, -1, np.int32), decay=np.zeros(Q, np.float32),
               n_keep=np.zeros(G, np.int32))
    for g in range(G):
        rows = member[goff[g]:goff[g + 1]]
        D = len(rows)
        area = sc["area"][rows]
        m = measure_matrix(inter[poff[g]:poff[g + 1]], area, sc["category"][rows] if class_aware else None, measure)
        order = rank(scores[rows])
        out["order"][goff[g]:goff[g + 1]] = rows[order]
        if method == "greedy":
            gone = np.zeros(D, bool)
            for r, i in enumerate(order):
                if gone[i] or area[i] < 1:
                    continue
                out["keep"][rows[i]] = 1
                out["decay"][rows[i]] = 1.0
                for j in order[r + 1:]:                               # the textbook loop
                    if not gone[j] and m[i, j] > thr:
                        gone[j] = True
                        out["by"][rows[j]] = rows[i]
        else:
            s = np.maximum(m[np.ix_(order, order)], 0.0)
            up = np.triu(np.ones((D, D), bool), 1)                    # [i, j]: i ranked above j
            c = np.where(up, s, 0.0).max(axis=0) if D else np.zeros(0)
            if method == "linear":
                with np.errstate(divide="ignore", invalid="ignore"):
                    term = np.where((1.0 - c)[:, None] == 0.0, 1.0, (1.0 - s) / (1.0 - c)[:, None])
            else:
                term = np.exp(-sigma * (s * s - (c * c)[:, None]))
            decay = np.where(up, term, np.inf).min(axis=0) if D else np.zeros(0)
            decay = np.where(np.isinf(decay), 1.0, decay)
            out["decay"][rows[order]] = decay.astype(np.float32)
            out["keep"][rows] = (area >= 1).astype(np.uint8)
        out["n_keep"][g] = int(out["keep"][rows].sum())
    return out


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
def rect(h, w, y0, y1, x0, x1) -> np.ndarray:
    p = np.zeros((h, w), bool)
    p[y0:y1 + 1, x0:x1 + 1] = True
    return p


def hand_made() -> list:
    """(image, plane, score, category) of the hand-made groups; DESIGN.md §30 names each."""
    nan = float("nan")
    out = [(0, np.ones((1, 1), bool), 0.5, 1)]                                                     # D = 1: an empty pair block
    out += [(1, np.ones((1, 32), bool), 0.9, 1), (1, rect(1, 32, 0, 0, 16, 31), 0.8, 1)]          # D = 2, one full word
    # D = 3 on (5, 33): boxes that meet only in column 32 (planes 0, 1) and only in column 31 (planes 1, 2)
    out += [(2, rect(5, 33, 0, 4, 32, 32), 0.9, 1), (2, rect(5, 33, 1, 3, 31, 32), 0.8, 1), (2, rect(5, 33, 0, 4, 0, 31), 0.7, 1)]
    # (7, 31): the exact tie -- areas 1 and 2, inter 1, IoU 1 / 2 -- and two boxes that meet only in row 3
    out += [(3, rect(7, 31, 3, 3, 5, 5), 0.9, 1), (3, rect(7, 31, 3, 3, 5, 6), 0.8, 1),
            (3, rect(7, 31, 0, 3, 20, 30), 0.7, 1), (3, rect(7, 31, 3, 6, 20, 30), 0.6, 1)]
    # (3, 70): the chain A, B, C -- IoU(A, B) = IoU(B, C) = 0.6, IoU(A, C) = 1 / 3: A suppresses B, C survives because B is gone
    out += [(4, rect(3, 70, 0, 2, 0, 39), 0.9, 1), (4, rect(3, 70, 0, 2, 10, 49), 0.8, 1), (4, rect(3, 70, 0, 2, 20, 59), 0.7, 1)]
    big, far = rect(40, 65, 0, 29, 0, 49), rect(40, 65, 32, 39, 40, 64)
    blob = np.random.default_rng(5).random((40, 65)) < 0.3
    out += [(5, big, 0.9, 1), (5, big, 0.9, 1),                       # identical, equal scores: member order; c = 1 in linear mode
            (5, big, 0.8, 2),                                         # identical, another category
            (5, rect(40, 65, 5, 9, 5, 9), 0.7, 1),                    # nested in big: IoU 25 / 1500, min measure 1
            (5, np.zeros((40, 65), bool), 0.95, 1),                   # empty, ranked first
            (5, far, nan, 1), (5, far, nan, 1),                       # NaN scores: behind every number, member order
            (5, blob, 0.5, 1)]
    return out


def random_group(image: int, D: int, h: int, w: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(D):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        y1, x1 = int(rng.integers(y0, min(h, y0 + max(2, h // 2)))), int(rng.integers(x0, min(w, x0 + max(2, w // 2))))
        p = rect(h, w, y0, y1, x0, x1) & (rng.random((h, w)) < 0.9)
        out.append((image, p, float(np.float32(rng.integers(0, 64)) / np.float32(64)), int(rng.integers(0, 3))))   # many equal scores
    return out


_SCENE = {}


def scene(big: bool = True) -> dict:
    """The ragged call: the hand-made groups, D = 65 and 257 on (16, 40) planes, and (big) one group of D = 1024 on (8, 33) planes, the
    instances of all groups interleaved by a fixed permutation, every pad bit dirty.  Computed once; callers do not change it."""
    if big in _SCENE:
        return _SCENE[big]
    items = hand_made() + random_group(6, 65, 16, 40, 65) + random_group(7, 257, 16, 40, 257)
    if big:
        items += random_group(8, 1024, 8, 33, 1024)
    perm = np.random.default_rng(11).permutation(len(items))
    items = [items[k] for k in perm]
    planes = [it[1] for it in items]
    sizes = [p.shape for p in planes]
    dims, off = tables(sizes)
    st = [stats(p) for p in planes]
    keys, member, goff, poff = groups_of([it[0] for it in items])
    sc = dict(planes=planes, sizes=sizes, dims=dims, offsets=off, image=[it[0] for it in items],
              bits=np.concatenate([pack_rows(p, dirty=True, seed=k) for k, p in enumerate(planes)]),
              area=np.asarray([s[0] for s in st], np.int32), box=np.asarray([s[1] for s in st], np.int32).reshape(-1, 4),
              scores=np.asarray([it[2] for it in items], np.float32), category=np.asarray([it[3] for it in items], np.int32),
              keys=keys, member=member, group_offsets=goff, pair_offsets=poff, where={int(p): k for k, p in enumerate(perm)})
    sc["inter"] = inter_oracle(sc)
    _SCENE[big] = sc
    return sc


def row_of(sc: dict, k: int) -> int:
    """The row, in the scene's interleaved order, of item k of hand_made()."""
    return sc["where"][k]


# ---- runners --------------------------------------------------------------------------------------------------------------------------------
def run_inter(hip, sc: dict, dev="cpu", **over) -> dict:
    """cvlm_mask_nms_inter (or its host twin for dev = "cpu") on the scene's tables, `over` replacing any of them; inter lies between
    two guard bands and everything is pre-filled with garbage -> inter, status and whether the bands are whole."""
    t = {k: torch.from_numpy(np.ascontiguousarray(over.get(k, sc[k]))).to(dev) for k in
         ("bits", "offsets", "dims", "area", "box", "group_offsets", "member", "pair_offsets")}
    N = int(over.get("N", sc["pair_offsets"][-1]))
    whole = torch.full((N + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    status = torch.full((1,), FILL, dtype=torch.int32, device=dev)
    hip.mask_nms_inter(t["bits"], t["offsets"], t["dims"], t["area"], t["box"], t["group_offsets"], t["member"], t["pair_offsets"],
                       whole[GUARD:GUARD + N], status, host=dev == "cpu")
    w = whole.cpu().numpy()
    return dict(inter=w[GUARD:GUARD + N].copy(), status=int(status.cpu()), bands=bool((w[:GUARD] == FILL).all() and (w[GUARD + N:] == FILL).all()))


def run_nms(hip, sc: dict, inter: np.ndarray, dev="cpu", *, measure="iou", method="greedy", thr=0.5, sigma=2.0, class_aware=False, **over) -> dict:
    """cvlm_mask_nms (or its host twin) with every output pre-filled with garbage -> the outputs as numpy arrays and the status."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {k: up(over.get(k, sc[k])) for k in ("group_offsets", "member", "pair_offsets", "area", "scores", "category")}
    Q, G = len(sc["area"]), len(t["group_offsets"]) - 1
    order, by, n_keep, status = (torch.full((n,), FILL, dtype=torch.int32, device=dev) for n in (Q, Q, G, 1))
    keep = torch.full((Q,), 0xA5, dtype=torch.uint8, device=dev)
    decay = torch.full((Q,), float("nan"), dtype=torch.float32, device=dev)
    hip.mask_nms(t["group_offsets"], t["member"], t["pair_offsets"], up(inter), t["area"], t["scores"], t["category"] if class_aware else None,
                 MEASURES[measure], METHODS[method], thr, sigma, order, keep, by, decay, n_keep, status, host=dev == "cpu")
    return dict(order=order.cpu().numpy(), keep=keep.cpu().numpy(), by=by.cpu().numpy(), decay=decay.cpu().numpy(), n_keep=n_keep.cpu().numpy(),
                status=int(status.cpu()))


EXACT = ("order", "keep", "by", "n_keep")


def same(got: dict, want: dict, method: str) -> None:
    """The integers equal; the decay bit-equal for greedy and linear, within one float32 ulp (relative 2^-23) for gaussian."""
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), k
    if method == "gaussian":
        err = np.abs(got["decay"].astype(np.float64) - want["decay"].astype(np.float64))
        assert bool((err <= 2.0 ** -23 * np.abs(want["decay"].astype(np.float64))).all()), float(err.max())
    else:
        assert np.array_equal(got["decay"].view(np.uint32), want["decay"].view(np.uint32))
