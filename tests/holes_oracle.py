"""scipy oracle of the holes of packed masks (cvlm_mask_holes).  A hole of a plane is a connected region of its CLEAR
pixels that contains no pixel of the plane's border; clear pixels are connected at the DUAL of the foreground connectivity.  So: the
complement labelled by scipy.ndimage.label under generate_binary_structure(2, 1) for connectivity 8 and (2, 2) for connectivity 4,
the labels seen on the border discarded, areas by bincount, boxes by find_objects, seed = the first raster index of each label, rows
sorted by (-area, seed), the filled plane from the area lookup.  Also the hand-made planes both test files run (`operator_cases`)."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

import compact_oracle as XO
from components_oracle import FILLER, pack  # noqa: F401  (re-exported: the test files pack through the oracle)


def hole_regions(plane: np.ndarray, connectivity: int):
    """plane bool [H, W] -> (labels int32 [H, W] of the CLEAR pixels from 1, is_hole bool [n + 1] by label, rows int64 [holes, 6] =
    (area, x0, y0, x1, y1, seed) sorted by (-area, seed))."""
    H, W = plane.shape
    lab, n = ndimage.label(~plane, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 8 else 2))
    is_hole = np.ones(n + 1, bool)
    is_hole[0] = False
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        is_hole[edge] = False
    if not is_hole.any():
        return lab, is_hole, np.zeros((0, 6), np.int64)
    flat = lab.ravel()
    area = np.bincount(flat, minlength=n + 1)
    idx = np.nonzero(flat)[0]
    seed = np.full(n + 1, H * W, np.int64)
    np.minimum.at(seed, flat[idx], idx)
    rows = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        if is_hole[k]:
            sy, sx = sl
            rows.append((area[k], sx.start, sy.start, sx.stop - 1, sy.stop - 1, seed[k]))
    rows = np.array(rows, np.int64)
    return lab, is_hole, rows[np.lexsort((rows[:, 5], -rows[:, 0]))]


def holes(bits: np.ndarray, H: int, W: int, connectivity: int = 8, M: int = 1, fill_below: int = 0) -> dict:
    """bits uint8 [P, H * W / 8] -> dict of n_holes int32 [P], holes int32 [P, M, 6] and, with fill_below >= 1, n_filled [P],
    filled_bits uint8 like bits, filled_area [P] -- what cvlm_mask_holes writes."""
    P = bits.shape[0]
    planes = XO.unpack(bits, H, W)
    out = dict(n_holes=np.zeros(P, np.int32), holes=np.tile(np.array(FILLER, np.int32), (P, M, 1)))
    filled = planes.copy()
    n_filled = np.zeros(P, np.int32)
    for p in range(P):
        lab, is_hole, rows = hole_regions(planes[p], connectivity)
        out["n_holes"][p] = len(rows)
        m = min(M, len(rows))
        out["holes"][p, :m] = rows[:m]
        if fill_below >= 1:
            small = is_hole & (np.bincount(lab.ravel(), minlength=len(is_hole)) < fill_below)
            filled[p] |= small[lab]
            n_filled[p] = int(small.sum())
    if fill_below >= 1:
        out["n_filled"] = n_filled
        out["filled_bits"] = np.packbits(filled.reshape(P, H * W), axis=-1)
        out["filled_area"] = XO.stats(filled)[0]
    return out


def ring(a: np.ndarray, y0: int, x0: int, h: int, w: int) -> None:
    """Set the one-pixel outline of the h x w rectangle at (y0, x0) of plane a."""
    a[y0, x0:x0 + w] = a[y0 + h - 1, x0:x0 + w] = True
    a[y0:y0 + h, x0] = a[y0:y0 + h, x0 + w - 1] = True


def operator_cases():
    """name -> bool planes [P, H, W]: the smallest shapes at which hole finding on words can go wrong."""
    c = {}
    z = lambda P, H, W: np.zeros((P, H, W), bool)
    # (1, 32): one word, one row -- y = 0 is the border: never a hole
    a = z(3, 1, 32)
    a[1] = True
    a[2] = True
    a[2, 0, 13] = False
    c["one_word"] = a                                                 # empty, full, one interior clear bit
    # (8, 32): rings
    a = z(7, 8, 32)
    ring(a[0], 2, 10, 4, 5)                                           # a 4 x 5 ring around a 2 x 3 interior: one hole of 6
    ring(a[1], 2, 10, 4, 5)
    a[1, 2, 10] = False                                               # a corner removed: the hole leaks at connectivity 4 only
    ring(a[2], 0, 10, 4, 5)                                           # a ring lying against the border, the border its fourth side:
    a[2, 0, 11:14] = False                                            # the interior reaches y = 0
    ring(a[3], 2, 27, 4, 5)
    a[3, 3:5, 31] = False                                             # ... and x = W - 1
    a[4] = (np.add.outer(np.arange(8), np.arange(32)) & 1) == 0       # checkerboard: 90 one-pixel holes at 8, none at 4
    ring(a[5], 0, 0, 8, 32)                                           # a frame on the border: one hole of 180
    ring(a[6], 4, 0, 4, 5)                                            # a closed ring that touches the border keeps its hole
    c["rings"] = a
    a = np.ones((2, 8, 32), bool)
    a[0, 3, 17] = False                                               # everything set but one interior pixel
    a[1, 7, 17] = False                                               # ... but one border pixel: no hole
    c["pinhole"] = a
    # (8, 64): a hole across a word seam; (8, 96): a hole spanning a whole word
    a = z(1, 8, 64)
    ring(a[0], 1, 28, 5, 9)
    c["seam"] = a
    a = z(1, 8, 96)
    ring(a[0], 1, 20, 6, 60)
    c["whole_word"] = a
    # (32, 32): a background "U" whose arms meet only in the last row of the hole; nested rings (hole, island, hole)
    a = z(2, 32, 32)
    a[0, 1:31, 1:31] = True
    a[0, 2:29, 3] = a[0, 2:29, 28] = a[0, 28, 3:29] = False
    ring(a[1], 2, 2, 28, 28)
    ring(a[1], 8, 8, 12, 12)
    a[1, 12:16, 12:16] = True
    c["u_and_nested"] = a
    # (64, 64): two equal holes (the tie goes to the lower seed); three holes (filler rows with M = 5)
    a = np.ones((2, 64, 64), bool)
    a[0, 3:8, 4:9] = a[0, 40:45, 50:55] = False
    a[1, 2:4, 2:30] = a[1, 10:30, 40:44] = a[1, 60, 60] = False
    c["squares_three"] = a
    # (2, 64): the first plane ends and the second starts with clear pixels -- and so do rows: the regions must not join
    a = np.ones((2, 4, 64), bool)
    a[0, 3, 60:] = a[1, 0, :4] = False
    a[0, 1, 60:] = a[0, 2, :4] = False
    a[0, 1, 10:20] = False                                            # and one real hole, so that the planes are not trivially equal
    c["plane_ends"] = a
    # (3, 64, 96): random planes
    rng = np.random.default_rng(7)
    c["random"] = np.stack([rng.random((64, 96)) < d for d in (0.5, 0.7, 0.9)])
    return c
