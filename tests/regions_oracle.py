"""Oracle of the instance entries (cvlm_mask_regions_sized, cvlm_region_alpha).  Regions: components_oracle.regions --
scipy.ndimage.label on the unpacked (h, w) plane, rows sorted by (-area, seed) -- plus what is new here: the min_area filter, the M
slots with their filler rows, and each slot as a packed plane of the source's size.  Alpha: rowops_oracle.bilinear on the plane as 0 / 1
gives the gate in fp64; it is multiplied by alpha[src].  Also the hand-made planes both test files run (`planes`) and one call of the
entry or its host twin on garbage-filled outputs (`run`)."""
from __future__ import annotations

import numpy as np
import torch

import components_oracle as CO
import rowops_oracle as RO

FILLER = CO.FILLER
WS_PER_WORD = 448


def tables(sizes):
    """-> dims int32 (P, 2), byte offsets int64 (P + 1), the largest word count: planes back to back, rows of ceil(w / 32) words."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    offsets = np.zeros(len(words) + 1, dtype=np.int64)
    np.cumsum(4 * words, out=offsets[1:])
    return dims, offsets, int(words.max())


def pack_rows(plane: np.ndarray, dirty: bool = False) -> np.ndarray:
    """bool (h, w) -> uint8 (h * 4 * ceil(w / 32),): every row packed on its own; dirty: every pad bit set instead of clear."""
    h, w = plane.shape
    wide = np.full((h, 32 * ((w + 31) // 32)), dirty, dtype=bool)
    wide[:, :w] = plane
    return np.packbits(wide, axis=1).reshape(-1)


def unpack_rows(flat: np.ndarray, h: int, w: int):
    """uint8 (h * 4 ws,) -> (bool (h, w), True if a pad bit is set)."""
    bits = np.unpackbits(flat.reshape(h, -1), axis=1).astype(bool)
    return bits[:, :w], bool(bits[:, w:].any())


def planes() -> list:
    """(name, bool plane) of every shape and content at which the sized labelling can go wrong; built once, never changed."""
    if _CACHE.get("planes") is None:
        out = []
        for name, stack in CO.operator_cases().items():
            out += [(f"{name}[{i}]", np.ascontiguousarray(p)) for i, p in enumerate(stack)]
        rnd = CO.operator_cases()["random"]
        out += [("random[2] cropped to 90", np.ascontiguousarray(rnd[2][:, :90])), ("random[1] cropped to 33", np.ascontiguousarray(rnd[1][:, :33]))]
        rng = np.random.default_rng(29)
        for h, w in ((1, 1), (1, 32), (5, 33), (7, 31), (40, 65)):
            out += [(f"random {h}x{w}", rng.random((h, w)) < 0.55), (f"full {h}x{w}", np.ones((h, w), bool))]
        a = np.zeros((4, 64), bool)
        a[1, 63] = a[2, 0] = True                                     # a row end: two regions under both connectivities
        out.append(("row end 4x64", a))
        a = np.zeros((3, 70), bool)
        a[0, 31] = a[1, 32] = a[2, 33] = True                         # a diagonal across a word seam: one region under 8, three under 4
        out.append(("diagonal seam 3x70", a))
        a = np.zeros((9, 45), bool)
        a[0:2, 0:5] = a[4, 20:22] = a[5:8, 30:43] = True              # three regions of 10, 2 and 39 pixels: min_area = 4 drops the middle one
        out.append(("three 9x45", a))
        out += [("empty 5x33", np.zeros((5, 33), bool)), ("full 5x33", np.ones((5, 33), bool))]
        out.append(("random 300x500", np.random.default_rng(593).random((300, 500)) < 0.593))
        _CACHE["planes"] = out
    return _CACHE["planes"]


_CACHE: dict = {}


def labelled(i: int, connectivity: int):
    """components_oracle.regions of plane i of `planes`, computed once."""
    key = ("lab", i, connectivity)
    if key not in _CACHE:
        _CACHE[key] = CO.regions(planes()[i][1], connectivity)
    return _CACHE[key]


def split(plane: np.ndarray, lab: np.ndarray, rows: np.ndarray, M: int, min_area: int):
    """-> (n_regions, table int32 (M, 6), the M planes bool (M, h, w)) of one plane from its labels and sorted rows."""
    keep = rows[rows[:, 0] >= max(min_area, 1)]
    table = np.tile(np.array(FILLER, np.int32), (M, 1))
    out = np.zeros((M,) + plane.shape, bool)
    for m, row in enumerate(keep[:M]):
        table[m] = row
        out[m] = lab == lab.ravel()[row[5]]
    return len(keep), table, out


def expected(connectivity: int, M: int, min_area: int, which=None) -> dict:
    """What one ragged call on `planes` (or the planes `which` of it) must give: n_regions (P,), table (P, M, 6), out_bits flat."""
    idx = list(range(len(planes()))) if which is None else list(which)
    n, tabs, bits = [], [], []
    for i in idx:
        lab, rows = labelled(i, connectivity)
        c, t, o = split(planes()[i][1], lab, rows, M, min_area)
        n.append(c)
        tabs.append(t)
        bits += [pack_rows(s) for s in o]
    return dict(n_regions=np.asarray(n, np.int32), table=np.stack(tabs), out_bits=np.concatenate(bits))


def run(fn, plane_list, connectivity: int, M: int, min_area: int, dev="cpu", ws_bytes=None, dirty: bool = False) -> dict:
    """One call of hip.mask_regions_sized (ws_bytes given: a workspace of exactly that many bytes) or its host twin on bool planes;
    every output is filled with garbage first.  -> numpy n_regions, table, out_bits, status."""
    dims, offsets, max_words = tables([p.shape for p in plane_list])
    bits = torch.from_numpy(np.concatenate([pack_rows(p, dirty) for p in plane_list])).to(dev)
    P = len(plane_list)
    n_regions = torch.full((P,), -77, dtype=torch.int32, device=dev)
    table = torch.full((P, M, 6), -77, dtype=torch.int32, device=dev)
    out_bits = torch.full((M * bits.numel(),), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    args = (bits, torch.from_numpy(offsets).to(dev), torch.from_numpy(dims).to(dev), max_words, connectivity, min_area)
    if ws_bytes is None:
        fn(*args, n_regions, table, out_bits, status)
    else:
        fn(*args, torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=dev), n_regions, table, out_bits, status)
    return dict(n_regions=n_regions.cpu().numpy(), table=table.cpu().numpy(), out_bits=out_bits.cpu().numpy(), status=int(status.item()))


def same(got: dict, want: dict) -> None:
    assert got["status"] == 0
    assert np.array_equal(got["n_regions"], want["n_regions"]), (got["n_regions"], want["n_regions"])
    bad = np.nonzero((got["table"] != want["table"]).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad[:4], got["table"][bad[0]], want["table"][bad[0]])
    assert got["out_bits"].shape == want["out_bits"].shape
    assert np.array_equal(got["out_bits"], want["out_bits"]), np.nonzero(got["out_bits"] != want["out_bits"])[0][:8]


# ---- cvlm_region_alpha ----------------------------------------------------------------------------------------------------------------
def gate(plane: np.ndarray, R: int) -> torch.Tensor:
    """bool (h, w) -> fp64 (R, R): the plane as 0 / 1 through rowops_oracle.bilinear."""
    return RO.bilinear(torch.from_numpy(plane.astype(np.float32))[None], R, R)[0]


def region_alpha(plane_list, alpha: torch.Tensor, src) -> torch.Tensor:
    """alpha f32 (N, R, R) -> fp64 (Q, R, R): alpha[src[q]] * gate_q."""
    R = int(alpha.shape[-1])
    return torch.stack([alpha[int(s)].double() * gate(p, R) for p, s in zip(plane_list, src)])


def run_alpha(fn, plane_list, alpha: torch.Tensor, src, dev="cpu"):
    """One call of hip.region_alpha or its host twin, out pre-filled with NaN -> (out f32 (Q, R, R) on the host, status)."""
    dims, offsets, _ = tables([p.shape for p in plane_list])
    bits = torch.from_numpy(np.concatenate([pack_rows(p) for p in plane_list])).to(dev)
    Q, R = len(plane_list), int(alpha.shape[-1])
    out = torch.full((Q, R, R), float("nan"), dtype=torch.float32, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    fn(bits, torch.from_numpy(offsets).to(dev), torch.from_numpy(dims).to(dev), alpha.contiguous().to(dev),
       torch.as_tensor(np.asarray(src, np.int32)).to(dev), out, status)
    return out.cpu(), int(status.item())
