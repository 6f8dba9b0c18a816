"""Crack contours as defined, in plain Python: a sequential walk over the unit edges of a plane, written without a look
at csrc/contour_logic.h.  `rings_of` gives the canonical rings of a bool plane; `flat` the tables the entries write; `signed_area`,
`components` and `framed_holes` what the consequences of the definition are held against.  `run` calls cvlm_mask_contour_count and
cvlm_mask_contour_emit, or the host entry, on a list of planes inside guard bands; `check` holds the result against `rings_of`."""
import numpy as np

GUARD = 16                    # sentinel bytes before the first and behind the last plane inside bits (offsets stay multiples of 4)
BAND = 64                     # sentinel elements around every output and bytes around the workspace
FILL = 0xA5
MAX_VERTS = 1 << 22


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------
def edges_of(mask: np.ndarray):
    """Every side of a set pixel whose neighbour across it is clear, as (start point, end point, pixel); points are (i, j) = (y, x) of
    the lattice, the foreground on the edge's right."""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    get = lambda y, x: 0 <= y < h and 0 <= x < w and bool(m[y, x])
    out = []
    for y in range(h):
        for x in range(w):
            if not m[y, x]:
                continue
            if not get(y - 1, x):
                out.append(((y, x), (y, x + 1), (y, x)))              # top side, heading east
            if not get(y, x + 1):
                out.append(((y, x + 1), (y + 1, x + 1), (y, x)))      # right side, heading south
            if not get(y + 1, x):
                out.append(((y + 1, x + 1), (y + 1, x), (y, x)))      # bottom side, heading west
            if not get(y, x - 1):
                out.append(((y + 1, x), (y, x), (y, x)))              # left side, heading north
    return out


def rings_of(mask: np.ndarray, connectivity: int = 8) -> list:
    """The canonical rings of a plane: a list of int arrays (n, 2) of (x, y), each starting at its vertex with the smallest (y, x),
    the list ordered by those starts."""
    assert connectivity in (4, 8)
    edges = edges_of(mask)
    leaving = {}
    for k, (s, _, _) in enumerate(edges):
        leaving.setdefault(s, []).append(k)
    seen = [False] * len(edges)
    rings = []
    for first in range(len(edges)):
        if seen[first]:
            continue
        points, k = [], first
        while not seen[k]:
            seen[k] = True
            s, t, pixel = edges[k]
            points.append(s)
            outs = leaving[t]
            assert len(outs) in (1, 2)
            if len(outs) == 1:
                k = outs[0]
            else:                                                     # a diagonal pair: 8 goes on with the other pixel, 4 with its own
                own = [o for o in outs if edges[o][2] == pixel]
                other = [o for o in outs if edges[o][2] != pixel]
                assert len(own) == 1 and len(other) == 1
                k = other[0] if connectivity == 8 else own[0]
        assert k == first, "the edges do not close into a ring"
        n = len(points)
        verts = []
        for a in range(n):                                            # a vertex: the edge that arrives and the edge that leaves differ in direction
            p, q, r = points[a - 1], points[a], points[(a + 1) % n]
            if (q[0] - p[0], q[1] - p[1]) != (r[0] - q[0], r[1] - q[1]):
                verts.append(q)
        assert len(verts) >= 4 and len(verts) % 2 == 0
        low = min(verts)
        assert verts.count(low) == 1, "a ring visits its smallest point twice"
        a = verts.index(low)
        verts = verts[a:] + verts[:a]
        rings.append(verts)
    rings.sort(key=lambda v: v[0])
    starts = [v[0] for v in rings]
    assert len(set(starts)) == len(starts), "two rings start at one point"
    return [np.asarray([(j, i) for i, j in v], dtype=np.int64) for v in rings]


def signed_area(ring) -> float:
    """1/2 sum(x_k y_k+1 - x_k+1 y_k): positive for an outer ring in image coordinates (y down, foreground on the right)."""
    r = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
    x, y = r[:, 0], r[:, 1]
    return 0.5 * float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def flat(rings):
    """-> (xy int16 (n, 2), ring_start uint8 (n,), (outer rings, holes)) as the entries write them."""
    if not rings:
        return np.zeros((0, 2), dtype=np.int16), np.zeros(0, dtype=np.uint8), (0, 0)
    xy = np.concatenate(rings).astype(np.int16)
    start = np.zeros(xy.shape[0], dtype=np.uint8)
    start[np.cumsum([0] + [len(r) for r in rings[:-1]])] = 1
    areas = [signed_area(r) for r in rings]
    return xy, start, (sum(a > 0 for a in areas), sum(a < 0 for a in areas))


def split(xy, ring_start) -> list:
    """The inverse of `flat`: the rings of one plane."""
    xy = np.asarray(xy).reshape(-1, 2)
    cuts = np.flatnonzero(np.asarray(ring_start))
    return [xy[a:b].astype(np.int64) for a, b in zip(cuts, list(cuts[1:]) + [xy.shape[0]])]


def components(mask: np.ndarray, connectivity: int) -> int:
    """Connected components of the set pixels by flood fill (no scipy needed)."""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    seen = np.zeros_like(m)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    n = 0
    for y0, x0 in zip(*np.nonzero(m)):
        if seen[y0, x0]:
            continue
        n += 1
        stack = [(y0, x0)]
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and m[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
    return n


def framed_holes(mask: np.ndarray, connectivity: int) -> int:
    """Background components that do not reach the outside, under the COMPLEMENTARY connectivity (4 for 8, 8 for 4): the components of
    the complement inside one clear frame, less the one that holds the frame."""
    m = np.asarray(mask, dtype=bool)
    framed = np.ones((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
    framed[1:-1, 1:-1] = ~m
    return components(framed, 12 - connectivity) - 1


# ---- the entries on lists of planes ------------------------------------------------------------------------------------------------------------
def tables(sizes, guard: int = GUARD):
    """-> dims int32 (P, 2), byte offsets int64 (P + 1) starting at `guard`, the byte length, the largest word count."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    offsets = guard + np.concatenate([[0], np.cumsum(4 * words)]).astype(np.int64)
    return dims, offsets, int(offsets[-1]) + guard, int(words.max())


def pack(plane: np.ndarray, dirty_pads: bool = False) -> np.ndarray:
    """bool (h, w) -> uint8 (h, 4 * ceil(w / 32)) in numpy.packbits' order; pad bits 0, or 1 with dirty_pads."""
    h, w = plane.shape
    full = np.full((h, 32 * ((w + 31) // 32)), 1 if dirty_pads else 0, dtype=np.uint8)
    full[:, :w] = plane
    return np.packbits(full, axis=1)


def run(planes, connectivity, dev="cpu", *, host=False, shift=0, outs=None, offsets=None, dims=None, short=None, dirty_pads=False, rounds=1):
    """Count and emit on `planes` (bool arrays): the device entries on `dev`, or with host=True cvlm_debug_mask_contour_host.  bits is a
    sentinel-filled tensor with GUARD bytes around the planes; every output and the workspace lie between BAND sentinels.  shift: bytes
    by which the base of bits is moved off its allocation.  outs: the tensors of an earlier call, to be used again (they must be large
    enough).  offsets / dims: doctored tables.  short: a plane whose slice of the vertex table is made one entry short.  rounds: the
    emit runs as this many calls on consecutive groups of planes, each through a workspace of exactly its own need.  -> dict(n_vertices: the count pass's, vertex_offsets, xy / ring_start: per plane, n_rings,
    status: (count, emit), outs)."""
    import torch
    from camouflaged_vlm_amd import hip
    sizes = [p.shape for p in planes]
    P = len(planes)
    good_dims, good_off, nbytes, max_words = tables(sizes)
    src = np.full(nbytes, FILL, dtype=np.uint8)
    for p, plane in enumerate(planes):
        src[good_off[p]:good_off[p + 1]] = pack(plane, dirty_pads).reshape(-1)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    holder = torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)
    bits = holder[shift:shift + nbytes]
    bits.copy_(dv(src))
    use_off = dv(good_off if offsets is None else np.asarray(offsets, dtype=np.int64))
    use_dims = dv(good_dims if dims is None else np.asarray(dims, dtype=np.int32).reshape(P, 2))
    n_vert = torch.full((P + 2 * BAND,), -7, dtype=torch.int32, device=dev)
    st_count = torch.full((1,), 77, dtype=torch.int32, device=dev)
    if host:
        hip.mask_contour_host(bits, use_off, use_dims, connectivity, n_vert[BAND:BAND + P], st_count)
    else:
        hip.mask_contour_count(bits, use_off, use_dims, connectivity, max_words, n_vert[BAND:BAND + P], st_count)
    nv = n_vert.cpu().numpy()
    assert (nv[:BAND] == -7).all() and (nv[BAND + P:] == -7).all(), "n_vertices: a guard band was written"
    counted = nv[BAND:BAND + P].astype(np.int64)
    lengths = counted.copy()
    if short is not None:
        lengths[short] -= 1
    vo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(vo[-1])
    if outs is None:
        outs = dict(xy=torch.full((total + 2 * BAND, 2), 0x5a5a, dtype=torch.int16, device=dev),
                    start=torch.full((total + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    rings=torch.full((P + 2 * BAND, 2), -7, dtype=torch.int32, device=dev), ws=None)
    xy_all, start_all, rings_all = outs["xy"], outs["start"], outs["rings"]
    cap = xy_all.shape[0] - 2 * BAND                                  # used outputs may be longer than this call needs
    assert cap >= total and rings_all.shape[0] == P + 2 * BAND
    xy, start, rings = xy_all[BAND:BAND + total], start_all[BAND:BAND + total], rings_all[BAND:BAND + P]
    vo_t = dv(vo)
    status = []
    if host:
        st = torch.full((1,), 77, dtype=torch.int32, device=dev)
        again = torch.empty(P, dtype=torch.int32, device=dev)
        hip.mask_contour_host(bits, use_off, use_dims, connectivity, again, st, vo_t, xy, start, rings)
        status.append(int(st.item()))
    else:
        cuts = [round(P * r / rounds) for r in range(rounds + 1)]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            rv = max(int(vo[b] - vo[a]), 0)
            need = hip.mask_contour_workspace_bytes(b - a, rv, max_words)
            if outs["ws"] is None or outs["ws"].numel() < need + 2 * BAND:
                outs["ws"] = torch.full((need + 2 * BAND,), FILL, dtype=torch.uint8, device=dev)
            ws = outs["ws"]
            ws[BAND + need:BAND + need + BAND] = FILL                  # a used workspace may be longer: the band lies behind this call's need
            st = torch.full((1,), 77, dtype=torch.int32, device=dev)
            hip.mask_contour_emit(bits, use_off[a:b + 1], use_dims[a:b], connectivity, max_words, vo_t[a:b + 1], rv, xy, start, rings[a:b],
                                  st, ws[BAND:BAND + need])
            status.append(int(st.item()))
            w = ws.cpu().numpy()
            assert (w[:BAND] == FILL).all() and (w[BAND + need:BAND + need + BAND] == FILL).all(), "workspace: a guard band was written"
    x, s, r = xy_all.cpu().numpy(), start_all.cpu().numpy(), rings_all.cpu().numpy()
    assert (x[:BAND] == 0x5a5a).all() and (s[:BAND] == FILL).all(), "xy / ring_start: the band in front was written"
    if cap == total:
        assert (x[BAND + total:] == 0x5a5a).all() and (s[BAND + total:] == FILL).all(), "xy / ring_start: the band behind was written"
    assert (r[:BAND] == -7).all() and (r[BAND + P:] == -7).all(), "n_rings: a guard band was written"
    assert (bits.cpu().numpy() == src[:bits.numel()]).all(), "bits were written"
    per_xy = [x[BAND + vo[p]:BAND + vo[p + 1]].copy() for p in range(P)]
    per_start = [s[BAND + vo[p]:BAND + vo[p + 1]].copy() for p in range(P)]
    return dict(n_vertices=counted, vertex_offsets=vo, xy=per_xy, ring_start=per_start, n_rings=r[BAND:BAND + P].copy(),
                status=(int(st_count.item()), max(status) if status else 0), outs=outs)


def check(res, planes, connectivity, refused=(), short=()):
    """The outputs of `run` against `rings_of`, every vertex, flag and count.  refused: planes with 0 vertices, 0 rings and an empty
    slice; short: planes whose count is right but whose slice, one short, holds zeros."""
    for p, plane in enumerate(planes):
        if p in refused:
            assert res["n_vertices"][p] == 0 and tuple(res["n_rings"][p]) == (0, 0) and res["xy"][p].shape[0] == 0, p
            continue
        xy, start, counts = flat(rings_of(plane, connectivity))
        assert res["n_vertices"][p] == xy.shape[0], (p, plane.shape, res["n_vertices"][p], xy.shape[0])
        if p in short:
            assert not res["xy"][p].any() and not res["ring_start"][p].any() and tuple(res["n_rings"][p]) == (0, 0), p
            continue
        assert np.array_equal(res["xy"][p], xy), (p, plane.shape, connectivity)
        assert np.array_equal(res["ring_start"][p], start), (p, plane.shape, connectivity)
        assert tuple(res["n_rings"][p]) == counts, (p, plane.shape, connectivity, tuple(res["n_rings"][p]), counts)


def same(res, other):
    """Two results of `run`, table for table."""
    assert np.array_equal(res["n_vertices"], other["n_vertices"])
    assert np.array_equal(res["n_rings"], other["n_rings"])
    for a, b in zip(res["xy"], other["xy"]):
        assert np.array_equal(a, b)
    for a, b in zip(res["ring_start"], other["ring_start"]):
        assert np.array_equal(a, b)
    assert res["status"] == other["status"]


# ---- planes ------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 31, 32, 33, 63, 64, 65)
HEIGHTS = (1, 2, 33)
RAGGED = [(1, 1), (70, 33), (5, 65), (33, 31), (1, 32), (97, 131), (2, 64)]          # DESIGN.md §19's seven


def contents(h: int, w: int, seed: int) -> list:
    """(name, plane) for one size: what the issue lists, each where the size has room for it."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((h, w), dtype=bool)
    out = [("empty", z()), ("full", ~z())]
    for name, (y, x) in (("nw", (0, 0)), ("ne", (0, w - 1)), ("sw", (h - 1, 0)), ("se", (h - 1, w - 1)), ("mid", (h // 2, w // 2))):
        m = z()
        m[y, x] = True
        out.append(("pixel " + name, m))
    for name, (y, x) in (("mid", (h // 2, w // 2)), ("corner", (h - 1, w - 1))):
        m = ~z()
        m[y, x] = False
        out.append(("clear " + name, m))
    if h >= 2 and w >= 2:
        y, x = h // 2 - (h // 2 == h - 1), w // 2 - (w // 2 == w - 1)
        m = z()
        m[y, x] = m[y + 1, x + 1] = True
        out.append(("main diagonal pair", m))
        m = z()
        m[y, x + 1] = m[y + 1, x] = True
        out.append(("anti diagonal pair", m))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", (yy + xx) % 2 == 0))
    out.append(("checkerboard 1", (yy + xx) % 2 == 1))
    if h >= 3 and w >= 3:
        m = ~z()
        m[1:-1, 1:-1] = False
        out.append(("ring", m))
    if h >= 7 and w >= 7:
        m = ~z()
        m[1:-1, 1:-1] = False
        m[2:-2, 2:-2] = True
        m[3:-3, 3:-3] = False
        out.append(("hole in island in hole", m))
    for name, sl in (("top", (slice(0, max(1, h // 3)), slice(None))), ("bottom", (slice(h - max(1, h // 3), h), slice(None))),
                     ("left", (slice(None), slice(0, max(1, w // 3)))), ("right", (slice(None), slice(w - max(1, w // 3), w)))):
        m = z()
        m[sl] = True
        out.append(("rectangle " + name, m))
    for d in (0.02, 0.5, 0.98):
        out.append((f"random {d}", rng.random((h, w)) < d))
    return out


def chain(n: int = 300) -> np.ndarray:
    """A diagonal chain of single pixels: one ring of 4 n vertices under 8, n rings of 4 under 4."""
    return np.eye(n, dtype=bool)


def comb(w: int = 257, h: int = 40) -> np.ndarray:
    """A spine along row 1 with 128 teeth, one in every second column, down to the last row, and a merlon above every second column of
    the spine: ONE ring of more than 1024 vertices whose vertical segments span the plane."""
    m = np.zeros((h, w), dtype=bool)
    m[0, 0::2] = True
    m[1, :] = True
    m[2:, 0:w - 1:2] = True
    return m


def big_cases() -> list:
    rng = np.random.default_rng(2626)
    return [("chain", chain()), ("comb", comb()), ("random 65 x 129", rng.random((65, 129)) < 0.5)]


def ragged_planes(seed: int = 26) -> list:
    rng = np.random.default_rng(seed)
    return [rng.random(s) < 0.6 for s in RAGGED]
