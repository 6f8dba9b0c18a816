"""Simplified contour rings as defined, in plain Python ints: Ramer-Douglas-Peucker on a closed ring as a recursive
split, written from the definition without a look at csrc/simplify_logic.h.  `simplify_ring` gives the kept indices of one ring, the
depth of its recursion and whether a chord with coincident ends was met; `expected` the tables the entries write for a list of planes;
`within` the Hausdorff bound in integers.  `run` calls cvlm_contour_simplify_mark and cvlm_contour_simplify_emit, or the host entry,
on the rings of `contour_oracle.rings_of` inside guard bands; `check` holds the result against `expected`."""
import sys

import numpy as np

import contour_oracle as CO

BAND = CO.BAND
FILL = CO.FILL
MAX_T = 65535

sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------
def d2(a, b) -> int:
    return (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def key(pi, pj, pv):
    """-> (num, L): the squared distance of pv to the SEGMENT pi pj is num / L."""
    if pi == pj:
        return d2(pv, pi), 1
    cx, cy, vx, vy = pj[0] - pi[0], pj[1] - pi[1], pv[0] - pi[0], pv[1] - pi[1]
    L = cx * cx + cy * cy
    t = vx * cx + vy * cy
    if t <= 0:
        return d2(pv, pi) * L, L
    if t >= L:
        return d2(pv, pj) * L, L
    return (cx * vy - cy * vx) ** 2, L


def simplify_ring(ring, T: int):
    """ring: (n, 2) ints, v_0 first -> (the kept indices in order, [] for a dropped ring; the depth of the recursion; whether a chord
    whose two ends coincide was split or tested)."""
    pts = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    n = len(pts)
    closed = pts + [pts[0]]                                           # index n: the closing appearance of v_0
    far = max(range(n), key=lambda v: (d2(pts[v], pts[0]), -v))
    kept = {0, far}
    info = {"depth": 0, "coincident": False}

    def split(i, j, depth):
        info["depth"] = max(info["depth"], depth)
        if j - i < 2:
            return
        if closed[i] == closed[j]:
            info["coincident"] = True
        best, at, L = -1, None, 1
        for v in range(i + 1, j):
            num, L = key(closed[i], closed[j], closed[v])
            if num > best:
                best, at = num, v
        if 16 * best > T * T * L:
            kept.add(at)
            split(i, at, depth + 1)
            split(at, j, depth + 1)

    if far != 0:
        split(0, far, 1)
        split(far, n, 1)
    else:
        split(0, n, 1)
    out = sorted(kept)
    return (out if len(out) >= 3 else []), info["depth"], info["coincident"]


def within(ring, kept, T: int) -> bool:
    """Every vertex of the ring lies within T / 4 of the segment between the kept vertices that bracket it: 16 num <= T^2 L, in ints."""
    pts = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    n = len(pts)
    closed = pts + [pts[0]]
    ends = list(kept) + [n]
    for i, j in zip(ends[:-1], ends[1:]):
        for v in range(i + 1, j):
            num, L = key(closed[i], closed[j], closed[v])
            if 16 * num > T * T * L:
                return False
    return True


def simplify_plane(rings, T: int):
    """The rings of one plane (contour_oracle.rings_of) -> dict(keep: uint8 per input vertex, xy int16 (m, 2), ring_start uint8 (m,) with
    1 outer / 2 hole, n_rings (outer, holes), dropped, depth, coincident)."""
    keep, xy, start, counts, dropped, depth, coincident = [], [], [], [0, 0], 0, 0, False
    for ring in rings:
        kept, d, c = simplify_ring(ring, T)
        depth, coincident = max(depth, d), coincident or c
        flags = np.zeros(len(ring), dtype=np.uint8)
        flags[kept] = 1
        keep.append(flags)
        if not kept:
            dropped += 1
            continue
        hole = CO.signed_area(ring) < 0
        counts[hole] += 1
        xy.append(np.asarray(ring)[kept])
        s = np.zeros(len(kept), dtype=np.uint8)
        s[0] = 2 if hole else 1
        start.append(s)
    cat = lambda parts, shape, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype=dtype)
    return dict(keep=cat(keep, (0,), np.uint8), xy=cat(xy, (0, 2), np.int16), ring_start=cat(start, (0,), np.uint8), n_rings=tuple(counts),
                dropped=dropped, depth=depth, coincident=coincident)


def expected(planes_rings, Ts) -> list:
    return [simplify_plane(rings, int(T)) for rings, T in zip(planes_rings, Ts)]


def rings_of_planes(planes, connectivity) -> list:
    return [CO.rings_of(p, connectivity) for p in planes]


# ---- the entries on lists of planes ------------------------------------------------------------------------------------------------------------
def run(planes_rings, Ts, dev="cpu", *, host=False, shift=0, outs=None, rounds=1, vertex_offsets=None, spoil_start=(), short=None):
    """Mark and emit on the rings of P planes: the device entries on `dev`, or with host=True cvlm_debug_contour_simplify_host.  Every
    output and the workspace lie between BAND sentinels.  shift: bytes by which the base of xy is moved off its allocation (a multiple
    of 4).  outs: the tensors of an earlier call, to be used again.  rounds: the mark runs as this many calls on consecutive groups of
    planes, each through a workspace of exactly its own need.  vertex_offsets: a doctored table.  spoil_start: planes whose first
    ring_start is cleared.  short: a plane whose output slice is made one entry short.  -> dict(keep / xy / ring_start: per plane,
    n_kept, n_rings, out_offsets, status: (mark, emit), outs)."""
    import torch
    from camouflaged_vlm_amd import hip
    P = len(planes_rings)
    flats = [CO.flat(r) for r in planes_rings]
    lengths = np.asarray([f[0].shape[0] for f in flats], dtype=np.int64)
    good_vo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(good_vo[-1])
    xy_in = np.concatenate([f[0] for f in flats]).astype(np.int16).reshape(total, 2)
    start_in = np.concatenate([f[1] for f in flats]).astype(np.uint8)
    for p in spoil_start:
        start_in[good_vo[p]] = 0
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    holder = torch.zeros(4 * total + 32, dtype=torch.uint8, device=dev)
    xy = holder[shift:shift + 4 * total].view(torch.int16).reshape(total, 2)
    xy.copy_(dv(xy_in))
    start = dv(start_in)
    vo = good_vo if vertex_offsets is None else np.asarray(vertex_offsets, dtype=np.int64)
    vo_t, T_t = dv(vo), dv(np.asarray(Ts, dtype=np.int32))
    if outs is None:
        outs = dict(keep=torch.full((total + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    n_kept=torch.full((P + 2 * BAND,), -7, dtype=torch.int32, device=dev),
                    rings=torch.full((P + 2 * BAND, 2), -7, dtype=torch.int32, device=dev),
                    xy=torch.full((total + 2 * BAND, 2), 0x5a5a, dtype=torch.int16, device=dev),
                    start=torch.full((total + 2 * BAND,), FILL, dtype=torch.uint8, device=dev), ws=None)
    assert outs["keep"].shape[0] == total + 2 * BAND and outs["n_kept"].shape[0] == P + 2 * BAND
    keep, n_kept, rings = outs["keep"][BAND:BAND + total], outs["n_kept"][BAND:BAND + P], outs["rings"][BAND:BAND + P]
    status = []
    if host:
        st = torch.full((1,), 77, dtype=torch.int32, device=dev)
        hip.contour_simplify_sequential(xy, start, vo_t, T_t, keep, n_kept, rings, st)
        status.append(int(st.item()))
    else:
        cuts = [round(P * r / rounds) for r in range(rounds + 1)]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            rv = max(int(vo[b] - vo[a]), int(good_vo[b] - good_vo[a]))        # a doctored table does not shrink the window of the others
            need = hip.contour_simplify_workspace_bytes(b - a, rv)
            if outs["ws"] is None or outs["ws"].numel() < need + 2 * BAND:
                outs["ws"] = torch.full((need + 2 * BAND,), FILL, dtype=torch.uint8, device=dev)
            ws = outs["ws"]
            ws[BAND + need:BAND + need + BAND] = FILL                  # a used workspace may be longer: the band lies behind this call's need
            st = torch.full((1,), 77, dtype=torch.int32, device=dev)
            hip.contour_simplify_mark(xy, start, vo_t[a:b + 1], T_t[a:b], rv, keep, n_kept[a:b], rings[a:b], st, ws[BAND:BAND + need])
            status.append(int(st.item()))
            w = ws.cpu().numpy()
            assert (w[:BAND] == FILL).all() and (w[BAND + need:BAND + need + BAND] == FILL).all(), "workspace: a guard band was written"
    counted = n_kept.cpu().numpy().astype(np.int64)
    lengths_out = counted.copy()
    if short is not None:
        lengths_out[short] -= 1
    oo = np.concatenate([[0], np.cumsum(lengths_out)]).astype(np.int64)
    total_out = int(oo[-1])
    assert total_out <= total
    xy_out, start_out = outs["xy"][BAND:BAND + total_out], outs["start"][BAND:BAND + total_out]
    outs["xy"][BAND + total_out:] = 0x5a5a                            # used outputs: the band lies behind this call's total
    outs["start"][BAND + total_out:] = FILL
    st = torch.full((1,), 77, dtype=torch.int32, device=dev)
    if host:
        again = {k: t.clone() for k, t in (("keep", keep), ("n_kept", n_kept), ("rings", rings))}       # a slice outside the table is left alone
        hip.contour_simplify_sequential(xy, start, vo_t, T_t, again["keep"], again["n_kept"], again["rings"], st, dv(oo), xy_out, start_out)
        assert torch.equal(again["keep"], keep) and torch.equal(again["n_kept"], n_kept) and torch.equal(again["rings"], rings)
    else:
        hip.contour_simplify_emit(xy, start, vo_t, keep, dv(oo), xy_out, start_out, st)
    emit_status = int(st.item())
    k, n, r = outs["keep"].cpu().numpy(), outs["n_kept"].cpu().numpy(), outs["rings"].cpu().numpy()
    x, s = outs["xy"].cpu().numpy(), outs["start"].cpu().numpy()
    assert (k[:BAND] == FILL).all() and (k[BAND + total:] == FILL).all(), "keep: a guard band was written"
    assert (n[:BAND] == -7).all() and (n[BAND + P:] == -7).all(), "n_kept: a guard band was written"
    assert (r[:BAND] == -7).all() and (r[BAND + P:] == -7).all(), "n_rings_out: a guard band was written"
    assert (x[:BAND] == 0x5a5a).all() and (x[BAND + total_out:] == 0x5a5a).all(), "xy_out: a guard band was written"
    assert (s[:BAND] == FILL).all() and (s[BAND + total_out:] == FILL).all(), "ring_start_out: a guard band was written"
    assert np.array_equal(xy.cpu().numpy(), xy_in) and np.array_equal(start.cpu().numpy(), start_in), "the input rings were written"
    inside = lambda p: 0 <= vo[p] <= vo[p + 1] <= total
    return dict(keep=[k[BAND + vo[p]:BAND + vo[p + 1]].copy() if inside(p) else None for p in range(P)],
                xy=[x[BAND + oo[p]:BAND + oo[p + 1]].copy() for p in range(P)],
                ring_start=[s[BAND + oo[p]:BAND + oo[p + 1]].copy() for p in range(P)],
                n_kept=counted, n_rings=r[BAND:BAND + P].copy(), out_offsets=oo, status=(max(status), emit_status), outs=outs)


def check(res, planes_rings, Ts, refused=(), short=()):
    """The outputs of `run` against the definition, every mark, vertex, flag and count.  refused: planes with no mark, no vertex and no
    ring; short: planes whose marks and counts are right but whose output slice, one short, holds zeros."""
    for p, (rings, T) in enumerate(zip(planes_rings, Ts)):
        if p in refused:
            assert res["n_kept"][p] == 0 and tuple(res["n_rings"][p]) == (0, 0) and res["xy"][p].shape[0] == 0, p
            assert res["keep"][p] is None or not res["keep"][p].any(), p
            continue
        want = simplify_plane(rings, int(T))
        assert np.array_equal(res["keep"][p], want["keep"]), (p, T)
        assert res["n_kept"][p] == want["xy"].shape[0] and tuple(res["n_rings"][p]) == want["n_rings"], (p, T)
        if p in short:
            assert not res["xy"][p].any() and not res["ring_start"][p].any(), p
            continue
        assert np.array_equal(res["xy"][p], want["xy"]), (p, T)
        assert np.array_equal(res["ring_start"][p], want["ring_start"]), (p, T)


def same(res, other):
    """Two results of `run`, table for table."""
    assert np.array_equal(res["n_kept"], other["n_kept"]) and np.array_equal(res["n_rings"], other["n_rings"])
    for name in ("keep", "xy", "ring_start"):
        for a, b in zip(res[name], other[name]):
            assert (a is None and b is None) or np.array_equal(a, b), name
    assert res["status"] == other["status"]


# ---- planes ------------------------------------------------------------------------------------------------------------------------------------
def disc(radius: int = 20) -> np.ndarray:
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return yy * yy + xx * xx <= radius * radius


def staircase(n: int = 24) -> np.ndarray:
    """A one-pixel-wide diagonal band under connectivity 4: pixels (k, k) and (k, k + 1) -- one ring that hugs a diagonal line."""
    m = np.zeros((n, n + 1), dtype=bool)
    for k in range(n):
        m[k, k] = m[k, k + 1] = True
    return m


def many_rings(h: int = 33, w: int = 65) -> np.ndarray:
    """Single pixels on every second row and column, and a few larger blocks: hundreds of rings, most of them dropped at T >= 4."""
    m = np.zeros((h, w), dtype=bool)
    m[0::2, 0::2] = True
    m[10:17, 20:41] = True
    m[12:15, 24:30] = False
    return m


# ---- the cases the host entry and the device entries are both held to, their rings computed once ----------------------------------------------
TOLERANCES = (0, 2, 4, 12)
_cache = {}


def cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def width_rings(w: int, connectivity: int) -> list:
    """The rings of contour_oracle's contents at width w and the three heights: the planes of one width in one call."""
    return cached(("width", w, connectivity),
                  lambda: rings_of_planes([m for h in CO.HEIGHTS for _, m in CO.contents(h, w, 100 * h + w)], connectivity))


def big_rings(connectivity: int) -> list:
    """(name, rings): the 300 x 300 chain, the 257-wide comb, 65 x 129 random at 0.5, the many-rings plane."""
    return cached(("big", connectivity),
                  lambda: [(n, CO.rings_of(m, connectivity)) for n, m in CO.big_cases() + [("many rings", many_rings())]])


def ragged_rings(connectivity: int = 8) -> list:
    return cached(("ragged", connectivity), lambda: rings_of_planes(CO.ragged_planes(), connectivity))
