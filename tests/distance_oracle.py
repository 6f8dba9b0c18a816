"""Distance maps of sized planes and directed surface totals, from their definitions, in plain numpy and plain loops.
`brute` is D2(y, x) = min over the set pixels of (y - y')^2 + (x - x')^2 by looking at every set pixel, for planes up to 40 x 65;
`edt` takes scipy's distance_transform_edt(~X, return_indices=True) and recomputes D2 from the indices in integers, for larger planes;
`with_reach` is the reach rule; `surface` the default surface of a mask; `totals` the directed totals of one pair as a loop over the
set pixels of A with math.fsum for sum_d; `metrics` the Hausdorff distance, ASSD, NSD and the boundary F-measure with their empty
cases.  `run_distance` / `run_totals` call the device entries or their host twins on lists of planes inside guard bands."""
import math

import numpy as np

import boundary_oracle as BO

FAR = 0x7fffffff
MAX_REACH = 23170
BRUTE_MAX = 40 * 65           # pixels up to which `d2_of` looks at every set pixel
PBAND = 64                    # sentinel entries before the first and behind the last plane of out_d2, and around every totals table
BAND = 64                     # sentinel bytes around the workspaces
FILL = BO.FILL
SENT = -7                     # the sentinel of the int32 / int64 tables
SENT_F = -7.5                 # and of sum_d


# ---- the definitions --------------------------------------------------------------------------------------------------------------------------
def brute(x: np.ndarray) -> np.ndarray:
    """int64 (h, w): the minimum over every set pixel; FAR on an empty plane."""
    x = np.asarray(x, dtype=bool)
    h, w = x.shape
    out = np.full((h, w), FAR, dtype=np.int64)
    ys, xs = np.nonzero(x)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    for a in range(0, ys.size, 256):                                  # 256 set pixels at a time: (256, h, w) integers
        d = (yy[None] - ys[a:a + 256, None, None]) ** 2 + (xx[None] - xs[a:a + 256, None, None]) ** 2
        out = np.minimum(out, d.min(axis=0))
    return out


def edt(x: np.ndarray) -> np.ndarray:
    """int64 (h, w) from scipy's nearest set pixel of every pixel: D2 recomputed from the indices in integers."""
    from scipy import ndimage
    x = np.asarray(x, dtype=bool)
    h, w = x.shape
    if not x.any():
        return np.full((h, w), FAR, dtype=np.int64)
    iy, ix = ndimage.distance_transform_edt(~x, return_indices=True, return_distances=False)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    return (yy - iy.astype(np.int64)) ** 2 + (xx - ix.astype(np.int64)) ** 2


def with_reach(d2: np.ndarray, reach: int) -> np.ndarray:
    """reach 0: unlimited; R >= 1: D2 if D2 <= R^2 else FAR."""
    return d2 if reach == 0 else np.where(d2 <= int(reach) ** 2, d2, FAR)


def d2_of(x: np.ndarray, reach: int = 0) -> np.ndarray:
    x = np.asarray(x, dtype=bool)
    return with_reach(brute(x) if x.size <= BRUTE_MAX else edt(x), reach)


def surface(x: np.ndarray) -> np.ndarray:
    """The default surface of a mask: a set pixel with a clear or outside pixel among its eight neighbours."""
    x = np.asarray(x, dtype=bool)
    h, w = x.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = x
    inner = np.ones((h, w), dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            inner &= pad[dy:dy + h, dx:dx + w]
    return x & ~inner


def surface_tolerance(h, w, ratio=0.008):
    return int(np.ceil(ratio * np.sqrt(h ** 2 + w ** 2))) if ratio < 1 else int(np.ceil(ratio))


def totals(a: np.ndarray, d2_b: np.ndarray, radii) -> dict:
    """The directed totals of the set pixels of `a` against the map `d2_b`, as a plain loop."""
    n = far = 0
    within = [0] * len(radii)
    max_d2, sum_d2, roots = -1, 0, []
    for y, x in zip(*np.nonzero(np.asarray(a, dtype=bool))):
        n += 1
        d2 = int(d2_b[y, x])
        if d2 == FAR:
            far += 1
            continue
        for k, r in enumerate(radii):
            within[k] += d2 <= int(r) ** 2
        max_d2 = max(max_d2, d2)
        sum_d2 += d2
        roots.append(math.sqrt(d2))
    return dict(n=n, far=far, within=within, max_d2=max_d2, sum_d2=sum_d2, sum_d=math.fsum(roots))


REFUSED = dict(n=-1, far=-1, max_d2=-1, sum_d2=-1, sum_d=0.0)       # and within = -1 everywhere


def metrics(ab: dict, ba: dict) -> dict:
    """AB: prediction against truth, BA: the reverse.  Floats; nsd / precision / recall / f are lists over the radii."""
    na, nb = ab["n"], ba["n"]
    T = len(ab["within"])
    any_far = ab["far"] != 0 or ba["far"] != 0
    if na == 0 and nb == 0:
        hd = assd = 0.0
    elif na == 0 or nb == 0 or any_far:
        hd = assd = math.inf
    else:
        hd = math.sqrt(max(ab["max_d2"], ba["max_d2"]))
        assd = (ab["sum_d"] + ba["sum_d"]) / (na + nb)
    nsd, prec, rec, f = [], [], [], []
    for k in range(T):
        if na == 0 and nb == 0:
            nsd.append(1.0)
        elif na == 0 or nb == 0:
            nsd.append(0.0)
        else:
            nsd.append((ab["within"][k] + ba["within"][k]) / (na + nb))
        if na == 0 and nb == 0:
            p, r = 1.0, 1.0
        elif na == 0:
            p, r = 1.0, 0.0
        elif nb == 0:
            p, r = 0.0, 1.0
        else:
            p, r = ab["within"][k] / na, ba["within"][k] / nb
        prec.append(p)
        rec.append(r)
        f.append(0.0 if p + r == 0 else 2 * p * r / (p + r))
    return dict(hausdorff=hd, assd=assd, nsd=nsd, precision=prec, recall=rec, f=f)


# ---- cvlm_mask_distance_sized on lists of planes ---------------------------------------------------------------------------------------------
def pix_tables(sizes, band: int = PBAND):
    """-> pixel offsets int64 (P + 1) starting at `band`, n_pix (band behind the last plane too)."""
    px = np.asarray([h * w for h, w in sizes], dtype=np.int64)
    off = band + np.concatenate([[0], np.cumsum(px)]).astype(np.int64)
    return off, int(off[-1]) + band


def ws_need(n_pix: int) -> int:
    return (2 * n_pix + 15) // 16 * 16


def run_distance(fn, planes, reaches, dev="cpu", shift=0, outs=None, offsets=None, dims=None, pix_offsets=None, dirty_pads=False):
    """One call of hip.mask_distance_sized / its host twin on `planes` (bool arrays) at `reaches`.  bits as in boundary_oracle.run (GUARD
    sentinel bytes, `shift` bytes off the allocation, dirty_pads); out_d2 has PBAND sentinel entries before the first and behind the
    last plane, the workspace BAND sentinel bytes around it.  outs: the tensors of an earlier call, used again.  offsets / dims /
    pix_offsets: doctored tables (the refusal tests).  -> dict(maps: each plane's int32 (h, w), status, outs); every band is checked."""
    import torch
    sizes = [p.shape for p in planes]
    good_dims, good_off, nbytes, max_words = BO.tables(sizes)
    good_pix, n_pix = pix_tables(sizes)
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
    need = ws_need(n_pix)
    if outs is None:
        outs = dict(d2=torch.full((n_pix,), SENT, dtype=torch.int32, device=dev),
                    ws=torch.full((need + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    status=torch.full((1,), 77, dtype=torch.int32, device=dev))
    use_off = good_off if offsets is None else np.asarray(offsets, dtype=np.int64)
    use_dims = good_dims if dims is None else np.asarray(dims, dtype=np.int32).reshape(P, 2)
    use_pix = good_pix if pix_offsets is None else np.asarray(pix_offsets, dtype=np.int64)
    fn(bits, dv(use_off), dv(use_dims), dv(np.asarray(reaches, dtype=np.int32)), max_words, dv(use_pix), outs["ws"][BAND:BAND + need],
       outs["d2"], outs["status"])
    d2 = outs["d2"].cpu().numpy()
    ws = outs["ws"].cpu().numpy()
    assert (d2[:PBAND] == SENT).all() and (d2[n_pix - PBAND:] == SENT).all(), "out_d2: a guard band was written"
    assert (ws[:BAND] == FILL).all() and (ws[BAND + need:] == FILL).all(), "workspace: a guard band was written"
    maps = [d2[good_pix[p]:good_pix[p + 1]].reshape(h, w).copy() for p, (h, w) in enumerate(sizes)]
    return dict(maps=maps, status=int(outs["status"].cpu().numpy()[0]), outs=outs)


def check_distance(res, planes, reaches, want=None, refused=(), untouched=()):
    """The maps of `run_distance` against the oracle, every entry; a refused plane is FAR everywhere, or -- `untouched` -- the sentinel
    it held.  want: the unlimited maps where the caller has them already."""
    for p, (plane, R) in enumerate(zip(planes, reaches)):
        if p in refused or p in untouched:
            assert (res["maps"][p] == (SENT if p in untouched else FAR)).all(), p
            continue
        ref = with_reach(d2_of(plane) if want is None else want[p], int(R))
        bad = res["maps"][p] != ref
        assert not bad.any(), (p, plane.shape, int(R), int(bad.sum()), np.argwhere(bad)[:3].tolist())


# ---- cvlm_mask_surface_totals on lists of pairs ----------------------------------------------------------------------------------------------
def run_totals(fn, a_planes, b_maps, pairs, radii, dev="cpu", outs=None, a_offsets=None, a_dims=None, b_pix_offsets=None, b_dims=None):
    """One call of hip.mask_surface_totals / its host twin: the set pixels of a_planes (bool arrays) against b_maps (int (h, w) arrays,
    e.g. d2_of's).  Every table lies between PBAND sentinel entries, the workspace between BAND sentinel bytes.  -> dict of numpy
    tables, status, outs; every band is checked."""
    import torch
    import importlib
    hip = importlib.import_module("camouflaged_vlm_amd.hip")
    a_sizes = [p.shape for p in a_planes]
    good_dims, good_off, nbytes, max_words = BO.tables(a_sizes)
    src = np.full(nbytes, FILL, dtype=np.uint8)
    for p, plane in enumerate(a_planes):
        src[good_off[p]:good_off[p + 1]] = BO.pack(plane).reshape(-1)
    b_sizes = [m.shape for m in b_maps]
    good_pix, n_pix = pix_tables(b_sizes)
    flat = np.full(n_pix, SENT, dtype=np.int32)
    for p, m in enumerate(b_maps):
        flat[good_pix[p]:good_pix[p + 1]] = np.asarray(m, dtype=np.int32).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    N = pairs.shape[0]
    radii = np.asarray(radii, dtype=np.int32).reshape(N, -1)
    T = radii.shape[1]
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    need = hip.mask_surface_workspace_bytes(N)
    if outs is None:
        table = lambda n, dtype, fill: torch.full((n + 2 * PBAND,), fill, dtype=dtype, device=dev)
        outs = dict(n=table(N, torch.int32, SENT), far=table(N, torch.int32, SENT), within=table(N * T, torch.int32, SENT),
                    max_d2=table(N, torch.int32, SENT), sum_d2=table(N, torch.int64, SENT), sum_d=table(N, torch.float64, SENT_F),
                    ws=torch.full((need + 2 * BAND,), FILL, dtype=torch.uint8, device=dev),
                    status=torch.full((1,), 77, dtype=torch.int32, device=dev))
    mid = lambda name, n: outs[name][PBAND:PBAND + n]
    use = lambda good, given, dtype: good if given is None else np.asarray(given, dtype=dtype)
    fn(dv(src), dv(use(good_off, a_offsets, np.int64)), dv(use(good_dims, a_dims, np.int32).reshape(-1, 2)), dv(flat),
       dv(use(good_pix, b_pix_offsets, np.int64)), dv(use(np.asarray(b_sizes, dtype=np.int32), b_dims, np.int32).reshape(-1, 2)), dv(pairs),
       dv(radii), max_words, outs["ws"][BAND:BAND + need], mid("n", N), mid("far", N), mid("within", N * T).view(N, T), mid("max_d2", N),
       mid("sum_d2", N), mid("sum_d", N), outs["status"])
    res = {}
    for name, n, fill in (("n", N, SENT), ("far", N, SENT), ("within", N * T, SENT), ("max_d2", N, SENT), ("sum_d2", N, SENT),
                          ("sum_d", N, SENT_F)):
        arr = outs[name].cpu().numpy()
        assert (arr[:PBAND] == fill).all() and (arr[PBAND + n:] == fill).all(), f"{name}: a guard band was written"
        res[name] = arr[PBAND:PBAND + n].copy()
    res["within"] = res["within"].reshape(N, T)
    ws = outs["ws"].cpu().numpy()
    assert (ws[:BAND] == FILL).all() and (ws[BAND + need:] == FILL).all(), "workspace: a guard band was written"
    res.update(status=int(outs["status"].cpu().numpy()[0]), outs=outs)
    return res


def sum_d_bound(t: dict) -> float:
    """|sum_d - fsum| allowed: n * 2^-52 * fsum -- each square root and each of at most n - 1 additions contributes at most 2^-53
    relative."""
    return t["n"] * 2.0 ** -52 * t["sum_d"]


def check_totals(res, a_planes, b_maps, pairs, radii, refused=()):
    """The tables of `run_totals` against `totals`: every integer exactly, sum_d within `sum_d_bound`."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    radii = np.asarray(radii).reshape(pairs.shape[0], -1)
    for i, (ia, ib) in enumerate(pairs):
        if i in refused:
            assert res["n"][i] == res["far"][i] == res["max_d2"][i] == res["sum_d2"][i] == -1 and (res["within"][i] == -1).all(), i
            assert res["sum_d"][i] == 0.0, i
            continue
        want = totals(a_planes[ia], b_maps[ib], radii[i])
        got = dict(n=int(res["n"][i]), far=int(res["far"][i]), within=res["within"][i].tolist(), max_d2=int(res["max_d2"][i]),
                   sum_d2=int(res["sum_d2"][i]))
        assert got == {k: want[k] for k in got}, (i, got, want)
        assert abs(float(res["sum_d"][i]) - want["sum_d"]) <= sum_d_bound(want), (i, float(res["sum_d"][i]), want["sum_d"])


# ---- planes -------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 129)
HEIGHTS = (1, 2, 33, 130)
RAGGED = BO.RAGGED                                                    # DESIGN.md §19's seven


def reaches_of(h: int, w: int):
    """0, 1, 2, 7 and one above the diagonal."""
    return (0, 1, 2, 7, int(math.ceil(math.sqrt(h * h + w * w))) + 1)


def contents(h: int, w: int, seed: int):
    """(name, plane) of every pattern the issue lists, at one size."""
    rng = np.random.default_rng(seed)
    zero = lambda: np.zeros((h, w), dtype=bool)
    out = [("empty", zero()), ("full", np.ones((h, w), dtype=bool))]
    for name, (y, x) in (("top left", (0, 0)), ("top right", (0, w - 1)), ("bottom left", (h - 1, 0)), ("bottom right", (h - 1, w - 1)),
                         ("middle", (h // 2, w // 2))):
        m = zero()
        m[y, x] = True
        out.append((f"one pixel, {name}", m))
    m = np.ones((h, w), dtype=bool)
    m[h // 2, w // 3] = False
    out.append(("one clear pixel", m))
    m = zero()
    m[:, w // 2] = True
    out.append(("a set column", m))
    m = zero()
    m[h // 3, :] = True
    out.append(("a set row", m))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", (yy + xx) % 2 == 0))
    for density in (0.02, 0.5, 0.98):
        out.append((f"random {density}", rng.random((h, w)) < density))
    return out


def gpu_list():
    """Every (size, pattern, reach) of the shapes-and-reaches matrix as three parallel lists: planes, reaches, and the index of each
    plane's pattern in `unique` -- the unlimited map of a pattern is computed once and cut at every reach."""
    planes, reaches, which, unique = [], [], [], []
    for i, h in enumerate(HEIGHTS):
        for j, w in enumerate(WIDTHS):
            for _, plane in contents(h, w, 100 * i + j):
                unique.append(plane)
                for R in reaches_of(h, w):
                    planes.append(plane)
                    reaches.append(R)
                    which.append(len(unique) - 1)
    return planes, reaches, which, unique


def stress_planes():
    """(name, plane): the three planes that stress the passes."""
    corner = np.zeros((300, 300), dtype=bool)
    corner[0, 0] = True
    wide = np.zeros((2, 16384), dtype=bool)
    wide[0, 0] = True
    stripes = np.zeros((67, 150), dtype=bool)
    stripes[::2] = True
    stripes[21:40] = False                                            # a thick run of empty rows in the middle as well
    return [("300 x 300, one corner pixel", corner), ("2 x 16384, one pixel at x = 0", wide), ("rows alternately empty and full", stripes)]
