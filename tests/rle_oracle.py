"""Oracle of the run-length encoding of packed masks (include/cvlm.h: cvlm_mask_rle_count / cvlm_mask_rle_emit): the
definition itself in numpy -- unpackbits, transpose, flatnonzero of the differences -- and, for the oracle's own check, a plain pixel
loop.  pycocotools is not a dependency of this project: the definition is the reference.  Importable without a GPU."""
import numpy as np


def plane_counts(plane: np.ndarray) -> np.ndarray:
    """bool (H, W) -> int64 run counts: column-major, alternating, starting with the 0s."""
    f = np.ascontiguousarray(plane.astype(np.int8).T).reshape(-1)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0).astype(np.int64)


def plane_counts_loop(plane: np.ndarray) -> list:
    """The same by a pixel loop: walk the columns, close a run whenever the pixel changes."""
    H, W = plane.shape
    counts, value, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            v = int(plane[y, x])
            if v != value:
                counts.append(run)
                value, run = v, 0
            run += 1
    counts.append(run)
    return counts


def unpack(bits: np.ndarray, H: int, W: int) -> np.ndarray:
    """uint8 (P, H * W / 8) in numpy.packbits' order -> bool (P, H, W)."""
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), axis=-1).reshape(-1, H, W).astype(bool)


def pack(planes: np.ndarray) -> np.ndarray:
    """bool (P, H, W) -> uint8 (P, H * W / 8)."""
    P = planes.shape[0]
    return np.packbits(planes.reshape(P, -1), axis=-1)


def encode(bits: np.ndarray, H: int, W: int) -> list:
    """uint8 (P, H * W / 8) -> the list of each plane's counts."""
    return [plane_counts(p) for p in unpack(bits, H, W)]


def cases(H: int, W: int, seed: int = 0) -> dict:
    """The operator cases on planes of H x W (W % 32 == 0): name -> bool (H, W)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    z = lambda: np.zeros((H, W), dtype=bool)
    out = {"empty": z(), "full": ~z()}
    for name, (y, x) in (("first_pixel", (0, 0)), ("last_pixel", (H - 1, W - 1))):
        out[name] = z()
        out[name][y, x] = True
    out["column"] = z()
    out["column"][:, W // 2 + 1] = True
    out["row"] = z()
    out["row"][H // 2] = True
    out["checker"] = (np.add.outer(np.arange(H), np.arange(W)) & 1).astype(bool)
    out["stripes"] = np.broadcast_to((np.arange(H) & 1).astype(bool)[:, None], (H, W)).copy()   # period 2 down a column: most runs
    out["stripes_columns"] = np.broadcast_to((np.arange(W) & 1).astype(bool)[None, :], (H, W)).copy()   # every column one run
    if W >= 64:                                                       # row 0 across the word seam, both ways
        out["seam_below"] = z()
        out["seam_below"][H - 1, 31] = True
        out["seam_above"] = z()
        out["seam_above"][0, 32] = True
    for d in (0.01, 0.5, 0.99):
        out[f"random_{d}"] = rng.random((H, W)) < d
    return out
