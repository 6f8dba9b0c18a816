"""scipy oracle of connected components of packed masks (cvlm_mask_components): planes unpacked by
compact_oracle.unpack, labelled by scipy.ndimage.label under generate_binary_structure(2, 1) (4-connectivity) or (2, 2) (8), areas
by bincount, boxes by find_objects, seed = the first raster index of each label, rows sorted by (-area, seed), the kept plane from
the area lookup.  Also the hand-made planes both test files run (`operator_cases`)."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

import compact_oracle as XO

FILLER = (0, -1, -1, -1, -1, -1)


def regions(plane: np.ndarray, connectivity: int):
    """plane bool [H, W] -> (labels int32 [H, W] from 1, rows int64 [n, 6] = (area, x0, y0, x1, y1, seed) sorted by (-area, seed))."""
    H, W = plane.shape
    lab, n = ndimage.label(plane, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    if n == 0:
        return lab, np.zeros((0, 6), np.int64)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    seed = np.full(n + 1, H * W, np.int64)
    np.minimum.at(seed, flat[idx], idx)
    rows = np.empty((n, 6), np.int64)
    for k, (sy, sx) in enumerate(ndimage.find_objects(lab)):
        rows[k] = (area[k], sx.start, sy.start, sx.stop - 1, sy.stop - 1, seed[k + 1])
    order = np.lexsort((rows[:, 5], -rows[:, 0]))
    return lab, rows[order]


def components(bits: np.ndarray, H: int, W: int, connectivity: int = 8, M: int = 1, min_area: int = 0) -> dict:
    """bits uint8 [P, H * W / 8] -> dict of n_comp int32 [P], comps int32 [P, M, 6] and, with min_area >= 1, n_kept [P], kept_bits
    uint8 like bits, kept_area [P], kept_box [P, 4] -- what cvlm_mask_components writes."""
    P = bits.shape[0]
    planes = XO.unpack(bits, H, W)
    out = dict(n_comp=np.zeros(P, np.int32), comps=np.tile(np.array(FILLER, np.int32), (P, M, 1)))
    kept = np.zeros_like(planes)
    n_kept = np.zeros(P, np.int32)
    for p in range(P):
        lab, rows = regions(planes[p], connectivity)
        out["n_comp"][p] = len(rows)
        m = min(M, len(rows))
        out["comps"][p, :m] = rows[:m]
        if min_area >= 1 and len(rows):
            big = np.concatenate([[False], np.bincount(lab.ravel(), minlength=len(rows) + 1)[1:] >= min_area])
            kept[p] = big[lab]
            n_kept[p] = int(big.sum())
    if min_area >= 1:
        out["n_kept"] = n_kept
        out["kept_bits"] = np.packbits(kept.reshape(P, H * W), axis=-1)
        out["kept_area"], out["kept_box"] = XO.stats(kept)
    return out


def pack(planes: np.ndarray) -> np.ndarray:
    """bool [P, H, W] -> uint8 [P, H * W / 8] in numpy.packbits' order."""
    P, H, W = planes.shape
    return np.packbits(planes.reshape(P, H * W), axis=-1)


def operator_cases():
    """name -> bool planes [P, H, W]: the smallest shapes at which the word-seeded labelling can go wrong."""
    c = {}
    z = lambda P, H, W: np.zeros((P, H, W), bool)
    # (1, 1, 32): one word
    a = z(4, 1, 32)
    a[1] = True
    a[2, 0, 13] = True
    a[3, 0, ::2] = True
    c["one_word"] = a                                                 # empty, full, one pixel, alternating bits
    # (2, 2, 64): seams
    a = z(2, 2, 64)
    a[0, 0, 31] = a[0, 0, 32] = True                                  # word seam: one region
    a[0, 0, 63] = a[0, 1, 0] = True                                   # row end: must not join
    a[0, 1, 63] = a[1, 0, 0] = True                                   # plane end: must not join
    c["seams"] = a
    # (1, 2, 32) and the diagonal across a word seam at W = 64
    a = z(2, 2, 32)
    a[0, 0, 5] = a[0, 1, 6] = True
    a[1, 0, 6] = a[1, 1, 5] = True
    c["diagonal"] = a
    a = z(2, 2, 64)
    a[0, 0, 31] = a[0, 1, 32] = True
    a[1, 0, 32] = a[1, 1, 31] = True
    c["diagonal_seam"] = a
    # (1, 32, 32)
    a = z(2, 32, 32)
    a[0] = (np.add.outer(np.arange(32), np.arange(32)) & 1) == 0      # checkerboard: 512 regions at 4, one at 8
    a[1, :, 3] = a[1, :, 28] = a[1, 31, 3:29] = True                  # a "U": the arms meet only in the last row
    c["board_and_u"] = a
    # (1, 64, 64)
    a = z(3, 64, 64)
    a[0, ::2, :] = True                                               # serpentine: full rows joined alternately at the right and left end
    a[0, 1::4, 63] = a[0, 3::4, 0] = True
    a[1, 3:8, 4:9] = a[1, 40:45, 50:55] = True                        # two equal squares: the tie goes to the lower seed
    a[2, 2:4, 2:30] = a[2, 10:30, 40:44] = a[2, 60, 60] = True        # three regions: filler rows with M = 5
    c["serpentine_squares_three"] = a
    # (3, 64, 96): random planes, the last at the site-percolation threshold of the square lattice
    rng = np.random.default_rng(14)
    c["random"] = np.stack([rng.random((64, 96)) < d for d in (0.3, 0.5, 0.593)])
    return c
