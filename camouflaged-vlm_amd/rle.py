"""COCO run-length encoding on the host: the compressed string form of a plane's run counts and the way back to the
plane.  Pure numpy, no device: `Cascade.mask_rle` produces the counts (cvlm_mask_rle_count / cvlm_mask_rle_emit), this module turns
them into what a consumer of COCO annotations takes.

The counts of a plane of H x W pixels are the lengths of the alternating runs of 0s and 1s of its pixels in column-major order,
starting with the 0s (the first count is 0 where pixel (0, 0) is set); they sum to H * W.  The compressed form writes, for i > 2, the
difference to counts[i - 2] in place of counts[i], each value in 5-bit groups, low group first: bit 0x20 of a group says that more
follow, bit 0x10 of the last group is the value's sign, and every group is a character offset by 48."""
from typing import Sequence, Union

import numpy as np


def counts_to_string(counts: Union[Sequence[int], np.ndarray]) -> bytes:
    """Run counts -> COCO's compressed string."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    out = bytearray()
    for i, x in enumerate(c):
        if i > 2:
            x -= c[i - 2]
        more = True
        while more:
            group = x & 0x1F
            x >>= 5                                                  # Python's shift keeps the sign, as the format expects
            more = x != -1 if group & 0x10 else x != 0
            out.append((group | 0x20 if more else group) + 48)
    return bytes(out)


def string_to_counts(s: Union[bytes, str]) -> np.ndarray:
    """COCO's compressed string -> run counts, int64 (n,).  ValueError for a string that ends inside a value or holds a character
    outside the format's 64."""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError("string_to_counts: the string ends inside a value")
            group = data[p] - 48
            if not 0 <= group < 64:
                raise ValueError(f"string_to_counts: character {data[p]!r} at {p} is outside the format")
            x |= (group & 0x1F) << (5 * k)
            more = bool(group & 0x20)
            p += 1
            k += 1
            if not more and group & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, dtype=np.int64)


def decode(counts: Union[Sequence[int], np.ndarray], H: int, W: int) -> np.ndarray:
    """Run counts of an H x W plane -> bool (H, W).  ValueError for a negative count or counts that do not sum to H * W."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size == 0 or bool((c < 0).any()) or int(c.sum()) != H * W:
        raise ValueError(f"decode: {c.size} counts summing to {int(c.sum())} do not describe a plane of {H} x {W}")
    values = (np.arange(c.size) & 1).astype(bool)
    return np.repeat(values, c).reshape(W, H).T.copy()
