"""Oracle of the morphology of packed masks (cvlm_mask_morph).  The band is computed by the reference's own lines
(models/sam_maskdecoder_edge.py:441-445: two max_pool2d with stride 1 and padding k // 2 on the unpacked plane, band = dilated - eroded
> 0, at kernel 2 r + 1), dilation and erosion by scipy.ndimage with the (2 r + 1)^2 structure and the border values of the definition:
outside the plane is clear to dilation (border_value=0) and set to erosion (border_value=1).  `plain` is the double loop over the
clipped window that tests/test_morph_cpu.py holds both against.  Also the hand-made planes both test files run (`operator_cases`)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

import compact_oracle as XO
from components_oracle import pack  # noqa: F401  (re-exported: the test files pack through the oracle)

RADII = (1, 2, 3, 7, 16)


def reference_band(planes: np.ndarray, r: int) -> np.ndarray:
    """bool [P, H, W] -> bool [P, H, W]: the reference's edge target at edge_ks = 2 r + 1."""
    mask = torch.from_numpy(planes.astype(np.float32))[:, None]
    edge_ks = 2 * r + 1
    eroded = -F.max_pool2d(-mask, edge_ks, stride=1, padding=edge_ks // 2)
    dilated = F.max_pool2d(mask, edge_ks, stride=1, padding=edge_ks // 2)
    return ((dilated - eroded) > 0)[:, 0].numpy()


def dilate_erode(planes: np.ndarray, r: int):
    """bool [P, H, W] -> (dil, ero) bool [P, H, W] by scipy.ndimage, plane by plane."""
    st = np.ones((2 * r + 1, 2 * r + 1), bool)
    dil = np.stack([ndimage.binary_dilation(p, structure=st, border_value=0) for p in planes])
    ero = np.stack([ndimage.binary_erosion(p, structure=st, border_value=1) for p in planes])
    return dil, ero


def plain(plane: np.ndarray, r: int):
    """bool [H, W] -> (dil, ero, band): the definition itself, any / all over the window clipped to the plane."""
    H, W = plane.shape
    dil, ero = np.zeros_like(plane), np.zeros_like(plane)
    for y in range(H):
        for x in range(W):
            win = plane[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            dil[y, x], ero[y, x] = win.any(), win.all()
    return dil, ero, dil & ~ero


def morph_planes(planes: np.ndarray, r: int) -> dict:
    """bool [P, H, W] -> what cvlm_mask_morph writes with all three pairs asked for."""
    P, H, W = planes.shape
    dil, ero = dilate_erode(planes, r)
    band = reference_band(planes, r)
    out = {}
    for name, a in (("dil", dil), ("ero", ero), ("band", band)):
        out[name + "_bits"] = np.packbits(a.reshape(P, H * W), axis=-1)
        out[name + "_area"] = a.reshape(P, -1).sum(1).astype(np.int32)
    return out


def morph(bits: np.ndarray, H: int, W: int, r: int) -> dict:
    """bits uint8 [P, H * W / 8] -> dict of dil_bits, dil_area, ero_bits, ero_area, band_bits, band_area."""
    return morph_planes(XO.unpack(bits, H, W), r)


def operator_cases():
    """name -> (bool planes [P, H, W], radii): the smallest shapes at which morphology on words can go wrong."""
    c = {}
    z = lambda P, H, W: np.zeros((P, H, W), bool)
    # (1, 32): one word, one row -- empty, full, one pixel, alternating bits
    a = z(4, 1, 32)
    a[1] = True
    a[2, 0, 13] = True
    a[3, 0, ::2] = True
    c["one_word"] = (a, RADII)
    # H < 2 r + 1 at every radius but the smallest
    rng = np.random.default_rng(16)
    c["one_row_two_words"] = (rng.random((2, 1, 64)) < np.array([0.1, 0.9]).reshape(2, 1, 1), RADII)
    c["three_rows"] = (rng.random((2, 3, 32)) < np.array([0.1, 0.9]).reshape(2, 1, 1), RADII)
    # the word seam, both directions
    a = z(2, 8, 64)
    a[0, 4, 31] = True
    a[1, 4, 32] = True
    c["seam"] = (a, RADII)
    # r = 16 from the middle word: both neighbour words reached, no further
    a = z(2, 5, 160)
    a[0, 2, 64 + 15] = True
    a[1, 2, 64] = a[1, 2, 95] = True
    c["three_words"] = (a[:, :, 32:128].copy(), (16,))                # 5 x 96
    c["five_words"] = (a, (16,))                                      # 5 x 160: words 0 and 4 stay clear
    # x = 0 and x = W - 1 on different rows: the row end must not wrap
    a = z(2, 40, 64)
    a[0, 10, 63] = a[0, 30, 0] = True
    a[1] = ~a[0]
    c["row_ends"] = (a, RADII)
    # planes must not leak: last row set, next plane empty; and the reverse
    a = z(4, 8, 64)
    a[0, 7] = True
    a[3, 0] = True
    c["plane_ends"] = (a, RADII)
    # a pixel in a corner ((r + 1)^2) and one in the interior ((2 r + 1)^2)
    a = z(5, 40, 64)
    a[0, 0, 0] = a[1, 0, 63] = a[2, 39, 0] = a[3, 39, 63] = True
    a[4, 18, 30] = True
    c["corner_interior"] = (a, RADII)
    for r in RADII:
        a = z(2, 4 * r + 4, 96)                                       # room for the whole dilation
        a[0, r + 1:3 * r + 2, 20:20 + 2 * r + 1] = True              # a (2 r + 1)^2 square: erodes to one pixel
        a[1, r + 1:3 * r + 1, 20:20 + 2 * r] = True                  # 2 r x 2 r: erodes to nothing, band = dilation
        c[f"squares_r{r}"] = (a, (r,))
    a = np.ones((4, 40, 64), bool)                                    # full; less one interior pixel; less one border pixel; ...
    a[1, 18, 30] = False
    a[2, 0, 33] = False
    a[3] = False
    a[3, 0] = a[3, -1] = a[3, :, 0] = a[3, :, -1] = True             # ... and a one-pixel frame on the border
    c["full_pinhole_frame"] = (a, RADII)
    a = z(1, 96, 160)
    a[0, 30:70, 50:120] = True                                        # a solid 40 x 70 blob: non-degenerate at r = 16
    c["blob"] = (a, (16,))
    rng = np.random.default_rng(70)
    c["random"] = (np.stack([rng.random((70, 160)) < d for d in (0.02, 0.5, 0.98)]), RADII)
    return c
