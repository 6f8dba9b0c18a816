"""numpy oracle of packed masks, areas, boxes and overlaps (cvlm_mask_pack / cvlm_mask_overlap): the binarisation
`m > 0` and numpy.packbits' default bit order of every digest in tests/golden/, counts and boxes by the plainest numpy there is,
intersections by a boolean matrix product."""
from __future__ import annotations

import numpy as np


def stats(b: np.ndarray):
    """b bool [..., H, W] -> (area int32 [...], box int32 [..., 4] = inclusive (x0, y0, x1, y1), -1 for an empty plane)."""
    lead, (H, W) = b.shape[:-2], b.shape[-2:]
    flat = b.reshape(-1, H, W)
    area = flat.sum((1, 2)).astype(np.int32)
    box = np.full((flat.shape[0], 4), -1, np.int32)
    for p, m in enumerate(flat):
        ys, xs = np.nonzero(m)
        if ys.size:
            box[p] = (xs.min(), ys.min(), xs.max(), ys.max())
    return area.reshape(lead), box.reshape(lead + (4,))


def pack(m: np.ndarray):
    """m f32 [..., H, W] logits -> (bits uint8 [..., H * W / 8] = packbits(m > 0), area, box)."""
    b = np.asarray(m) > 0
    H, W = b.shape[-2:]
    return (np.packbits(b.reshape(b.shape[:-2] + (H * W,)), axis=-1),) + stats(b)


def unpack(bits: np.ndarray, H: int, W: int) -> np.ndarray:
    """bits uint8 [..., H * W / 8] -> bool [..., H, W]."""
    return np.unpackbits(bits, axis=-1)[..., :H * W].astype(bool).reshape(bits.shape[:-1] + (H, W))


def inter(bits: np.ndarray) -> np.ndarray:
    """bits uint8 [n, K, bytes] -> int32 [n, K, K], inter[i, a, b] = |plane a AND plane b| of image i."""
    out = np.empty(bits.shape[:2] + bits.shape[1:2], np.int32)
    for i, planes in enumerate(bits):                                  # image by image: the unpacked planes are 64 x the input
        u = np.unpackbits(planes, axis=-1).astype(np.float64)          # counts below 2^53: the product is exact
        out[i] = np.rint(u @ u.T)
    return out
