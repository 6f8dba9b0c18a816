"""The cases of the edge tests of the two ends of the path -- preprocessing (csrc/preprocess.hip, N1) and the evaluation tail
(the metric kernels of csrc/evaltail.hip, N2) -- and the rule by which their C entry points choose a kernel, restated.

Both files pick a kernel from shapes and pointer alignment inside the entry point; there is no planner to ask.  `resample_path`,
`tensor_path` and `wfm_paths` restate those predicates from the call's arguments (pointers as integers), every case below names the
path it is aimed at, tests/test_ends_cases_cpu.py checks case against rule and the table against the list of paths without a GPU,
and the GPU tests (tests/test_preprocess_edges_gpu.py, tests/test_evaltail_edges_gpu.py) check the rule once more on the pointers they
really pass.  The inputs of a case are built here, from the case alone, so the CPU test sees what the GPU test runs.

Also here, shared with tests/test_evaltail.py: the numpy counters of cvlm_mask_joint_hist / cod_counts, and the weighted F-measure of
oracle/metrics_oracle.py taken apart into the pieces the kernels leave in their workspace (d2, Et, the three sums)."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from oracle import metrics_oracle as M

SENTINEL = 0xA5

# ---- the dispatch rules, restated ---------------------------------------------------------------------------------------------------
RESAMPLE_PATHS = ("row3", "row1", "generic_h", "col4", "generic_v")
TENSOR_PATHS = ("x4_word", "x4_byte", "generic")
ROW_LDS_LIMIT = 60 * 1024


def row_lds_bytes(W: int, C: int, n_out: int) -> int:
    """`smem` of cvlm_resample_u8 (csrc/preprocess.hip): source row and output row, each padded for any offset modulo 16"""
    return (((W * C) + 31) & ~15) + 16 + (((n_out * C) + 31) & ~15) + 16


def resample_path(N: int, H: int, W: int, C: int, n_out: int, axis: int, src_ptr: int, dst_ptr: int) -> str:
    """cvlm_resample_u8 (csrc/preprocess.hip, the three `if`s after the argument check): the row kernel for a horizontal pass of 1 or 3
    channels whose two rows fit 60 KB of LDS, the four-byte kernel for a vertical pass over rows of a multiple of 4 bytes between
    4-byte aligned pointers, the generic kernel for everything else."""
    if axis == 1 and C in (1, 3) and N * H < (1 << 30) and row_lds_bytes(W, C, n_out) <= ROW_LDS_LIMIT:
        return "row3" if C == 3 else "row1"
    if axis == 0 and (W * C) % 4 == 0 and (src_ptr | dst_ptr) % 4 == 0:
        return "col4"
    return "generic_h" if axis == 1 else "generic_v"


def tensor_path(N: int, H: int, W: int, C: int, top: int, left: int, ch: int, cw: int, src_ptr: int, dst_ptr: int):
    """cvlm_u8_to_tensor (csrc/preprocess.hip): the four-pixel kernel for C == 3, cw % 4 == 0 and a 16-byte aligned destination, the
    generic kernel otherwise.  Inside u8_to_tensor3x4_kernel a thread loads three words when its twelve source bytes start on a 4-byte
    boundary and twelve bytes otherwise; 12 * x4 keeps the residue, so the branch is one per source row.
    -> (path, rows on the word branch, rows on the byte branch); a case is named "x4_byte" when any row takes the byte branch."""
    if not (C == 3 and cw % 4 == 0 and dst_ptr % 16 == 0):
        return "generic", 0, 0
    res = [(src_ptr + ((n * H + top + y) * W + left) * 3) % 4 for n in range(N) for y in range(ch)]
    word = sum(r == 0 for r in res)
    return ("x4_byte" if word < len(res) else "x4_word"), word, len(res) - word


WFM_SEG, WFM_MAXSEG = 64, 64                 # csrc/evaltail.hip
WFM_MAX_W, WFM_MAX_H = 8192, 16384           # the refusals of cvlm_mask_wfm / cvlm_prob_wfm


def wfm_paths(h: int, w: int):
    """wfm_launch (csrc/evaltail.hip): the segmented column pass up to 64 segments of 64 rows, one thread per column above; the row pass
    keeps four ints per column in dynamic LDS and raises the kernel's limit above 64 KB (hipFuncSetAttribute).  The entries refuse
    w > 8192 and h > 16384.  -> (column pass, row pass) or None for a refused size."""
    if h <= 0 or w <= 0 or w > WFM_MAX_W or h > WFM_MAX_H:
        return None
    return ("segmented" if h <= WFM_SEG * WFM_MAXSEG else "tall"), ("lds_le_64k" if 4 * w * 4 <= 64 * 1024 else "lds_gt_64k")


# ---- resample cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Resample:
    path: str
    N: int
    H: int
    W: int
    C: int
    n_out: int
    axis: int
    src_off: int = 0            # bytes past a 16-byte boundary
    dst_off: int = 0
    pattern: str = "random"     # random | blocks (0 / 255 in 3-pixel blocks: bicubic overshoot at both ends)
    filters: Tuple[str, ...] = ("bilinear", "bicubic", "nearest")

    @property
    def id(self) -> str:
        s = f"{self.path}-n{self.N}-{self.H}x{self.W}x{self.C}-ax{self.axis}-to{self.n_out}"
        if self.src_off or self.dst_off:
            s += f"-s{self.src_off}d{self.dst_off}"
        return s + ("" if self.pattern == "random" else "-" + self.pattern)

    @property
    def n_in(self) -> int:
        return self.W if self.axis == 1 else self.H

    @property
    def out_shape(self):
        return (self.N, self.n_out, self.W, self.C) if self.axis == 0 else (self.N, self.H, self.n_out, self.C)


_EDGE_SIZES = (1, 2, 5, 16, 17, 341)


def _resample_cases():
    out = []
    for C in (3, 1):
        p = "row3" if C == 3 else "row1"
        out += [Resample(p, 1, 2, W, C, n, 1) for W in _EDGE_SIZES for n in _EDGE_SIZES]
        # 18 rows of an odd pitch on both sides: source and destination rows start at every offset modulo 16
        out.append(Resample(p, 3, 6, 341, C, 17, 1))
        out.append(Resample(p, 3, 6, 17, C, 341, 1))
        out += [Resample(p, 2, 3, 37, C, 21, 1, src_off=o, dst_off=(o * 5) % 16) for o in (1, 7, 15)]
    # either side of the 60 KB of LDS: 60096 bytes stay on the row kernel, 61536 fall to the generic one
    out.append(Resample("row3", 1, 2, 20000, 3, 7, 1))
    out.append(Resample("generic_h", 1, 2, 20480, 3, 7, 1))
    out.append(Resample("row1", 1, 2, 61000, 1, 7, 1, filters=("bilinear", "nearest")))
    out.append(Resample("generic_h", 1, 2, 61400, 1, 7, 1, filters=("bilinear", "nearest")))
    for C in (2, 4):
        out += [Resample("generic_h", 2, 3, 9, C, 5, 1), Resample("generic_h", 2, 3, 9, C, 13, 1), Resample("generic_h", 2, 2, 1, C, 4, 1)]
    for H in (1, 2, 3, 61):
        for n in (1, 7, 128):
            out.append(Resample("col4", 3, H, 4, 3, n, 0))
            out.append(Resample("generic_v", 3, H, 4, 3, n, 0, src_off=2))
            out.append(Resample("generic_v", 3, H, 4, 3, n, 0, dst_off=2))
    out += [Resample("col4", 2, 9, 33, 4, 20, 0), Resample("col4", 2, 61, 100, 1, 7, 0)]
    out += [Resample("generic_v", 2, 9, 33, 3, 4, 0), Resample("generic_v", 2, 9, 33, 3, 20, 0), Resample("generic_v", 2, 5, 7, 2, 3, 0)]
    # saturation: 0 / 255 blocks of three pixels through bicubic enlargement and reduction, on every path
    sat = ("bicubic",)
    out += [Resample("row3", 1, 40, 40, 3, 61, 1, pattern="blocks", filters=sat), Resample("row3", 1, 40, 40, 3, 29, 1, pattern="blocks", filters=sat),
            Resample("row1", 1, 40, 40, 1, 97, 1, pattern="blocks", filters=sat), Resample("generic_h", 1, 40, 40, 2, 61, 1, pattern="blocks", filters=sat),
            Resample("col4", 1, 40, 40, 3, 97, 0, pattern="blocks", filters=sat), Resample("col4", 1, 40, 40, 3, 29, 0, pattern="blocks", filters=sat),
            Resample("generic_v", 1, 40, 41, 3, 97, 0, pattern="blocks", filters=sat)]
    return tuple(out)


RESAMPLE_CASES = _resample_cases()


def _seed(*key) -> int:
    import zlib
    return zlib.crc32(repr(key).encode())


def resample_input(c: Resample) -> np.ndarray:
    """uint8 [N][H][W][C] of a case"""
    if c.pattern == "blocks":
        yy, xx = np.mgrid[0:c.H, 0:c.W]
        board = (((yy // 3) + (xx // 3)) % 2 * 255).astype(np.uint8)
        return np.broadcast_to(board[None, :, :, None], (c.N, c.H, c.W, c.C)).copy()
    return np.random.default_rng(_seed("resample", c.id)).integers(0, 256, (c.N, c.H, c.W, c.C), dtype=np.uint8)


def resample_tables(c: Resample, filt: str):
    from camouflaged_vlm_amd.preprocess import _coeffs
    return _coeffs(c.n_in, c.n_out, filt)


def resample_unclamped(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray, axis: int) -> np.ndarray:
    """the accumulator of preprocess_oracle._pass after the shift and before the clamp (one image, HWC)"""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for o in range(bounds.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        out[o] = ((src[lo:lo + n] * kk[o, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))).sum(axis=0) + (1 << 21)) >> 22
    return np.moveaxis(out, 0, axis)


def resample_reference(c: Resample, filt: str) -> np.ndarray:
    from oracle import preprocess_oracle as P
    b, k = resample_tables(c, filt)
    src = resample_input(c)
    return np.stack([P._pass(src[n], b, k, c.axis) for n in range(c.N)])


# (H, W) -> (out_h, out_w) of the whole resizes, every channel count, all three filters
RESIZE_CASES = (((1, 1), (4, 4)), ((5, 7), (11, 13)), ((3, 400), (3, 7)), ((683, 1024), (336, 503)))
RESIZE_CHANNELS = (1, 2, 3, 4)


# ---- ToTensor + Normalize + crop cases ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ToTensor:
    path: str
    N: int
    H: int
    W: int
    C: int
    top: int
    left: int
    ch: int
    cw: int
    src_off: int = 0            # bytes past a 16-byte boundary
    dst_off: int = 0            # bytes past a 16-byte boundary (a multiple of 4)
    both_branches: bool = False  # rows of the word branch and of the byte branch in one launch

    @property
    def id(self) -> str:
        s = f"{self.path}-n{self.N}-{self.H}x{self.W}x{self.C}-crop{self.top},{self.left},{self.ch}x{self.cw}"
        return s + (f"-s{self.src_off}d{self.dst_off}" if self.src_off or self.dst_off else "")


TENSOR_CASES = (
    ToTensor("x4_word", 2, 6, 16, 3, 1, 4, 4, 8),                           # W % 4 == 0, left % 4 == 0, top > 0
    ToTensor("x4_word", 1, 5, 12, 3, 2, 8, 3, 4),                           # the crop ends in the last row and column
    ToTensor("x4_word", 3, 4, 8, 3, 0, 0, 4, 8),                            # no crop, N = 3
    ToTensor("x4_byte", 2, 9, 503, 3, 0, 83, 9, 336, both_branches=True),   # the 683 x 1024 image at 336 x 503: pitch 1509 = 1 mod 4
    ToTensor("x4_byte", 2, 7, 503, 3, 2, 167, 5, 336, both_branches=True),  # top > 0, ends in the last row and column
    ToTensor("x4_byte", 1, 4, 16, 3, 0, 4, 4, 8, src_off=1),                # every row on the byte branch
    ToTensor("x4_byte", 1, 4, 16, 3, 1, 3, 3, 12),                          # left odd alone
    ToTensor("generic", 2, 5, 11, 3, 1, 2, 4, 7),                           # cw % 4 != 0
    ToTensor("generic", 2, 5, 11, 3, 1, 4, 4, 7),                           # ... ending in the last row and column
    ToTensor("generic", 2, 6, 10, 1, 2, 1, 4, 8),                           # C = 1
    ToTensor("generic", 2, 6, 10, 4, 1, 2, 5, 8),                           # C = 4
    ToTensor("generic", 2, 6, 16, 3, 1, 4, 4, 8, dst_off=4),                # C = 3, cw % 4 == 0, destination 4 bytes off
    ToTensor("generic", 1, 3, 5, 3, 0, 0, 3, 5, src_off=3, dst_off=8),      # no crop
    ToTensor("generic", 1, 1, 1, 2, 0, 0, 1, 1),                            # one pixel
)


def tensor_input(c: ToTensor):
    rng = np.random.default_rng(_seed("tensor", c.id))
    img = rng.integers(0, 256, (c.N, c.H, c.W, c.C), dtype=np.uint8)
    mean = rng.uniform(0.3, 0.6, c.C).astype(np.float32)
    std = rng.uniform(0.2, 0.3, c.C).astype(np.float32)
    return img, mean, std


def tensor_reference(c: ToTensor) -> np.ndarray:
    from oracle import preprocess_oracle as P
    img, mean, std = tensor_input(c)
    return np.stack([P.to_tensor_normalize(img[n, c.top:c.top + c.ch, c.left:c.left + c.cw], mean, std) for n in range(c.N)])


# GpuPreprocess(inp_size, clip_size) and the images of the clip_input / sam_input test: the resized side is 83 (odd: byte-branch rows in the
# crop), left = 14 (landscape) or top = 14 (portrait)
PIPELINE_SIZES = (64, 56)
PIPELINE_IMAGES = ((683, 1024), (1024, 683))


# ---- weighted F-measure cases -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Wfm:
    h: int
    w: int
    col: str                    # segmented | tall
    row: str                    # lds_le_64k | lds_gt_64k
    gt: str = "sparse"          # sparse | first_row | last_row | alt_cols | corner | empty | full | one_px
    N: int = 1

    @property
    def id(self) -> str:
        return f"{self.h}x{self.w}-{self.gt}" + (f"-n{self.N}" if self.N > 1 else "")


WFM_CASES = (
    Wfm(65, 64, "segmented", "lds_le_64k"),                     # a last segment of one row
    Wfm(64, 65, "segmented", "lds_le_64k"),                     # a second column group of one column
    Wfm(1024, 3, "segmented", "lds_le_64k"),                    # exactly 16 segments: one per thread row
    Wfm(1025, 3, "segmented", "lds_le_64k"),                    # 17: thread row 0 owns two
    Wfm(4096, 65, "segmented", "lds_le_64k"),                   # 64 segments: the last size on the segmented pass
    Wfm(4097, 8, "tall", "lds_le_64k"),                         # the first on the tall pass
    Wfm(4100, 70, "tall", "lds_le_64k", N=2),
    Wfm(3, 4096, "segmented", "lds_le_64k"),                    # 64 KB of LDS exactly
    Wfm(3, 4097, "segmented", "lds_gt_64k"),                    # 16 bytes more
    Wfm(8, 8192, "segmented", "lds_gt_64k"),                    # the widest row: 128 KB
    Wfm(1, 1, "segmented", "lds_le_64k", "full"),               # smaller than the Gaussian
    Wfm(1, 1, "segmented", "lds_le_64k", "empty"),
    Wfm(7, 7, "segmented", "lds_le_64k"),
    Wfm(3, 200, "segmented", "lds_le_64k"),
    Wfm(4096, 5, "segmented", "lds_le_64k", "first_row"),       # the carries cross every segment
    Wfm(4096, 5, "segmented", "lds_le_64k", "last_row"),
    Wfm(4100, 5, "tall", "lds_le_64k", "first_row"),
    Wfm(4100, 5, "tall", "lds_le_64k", "last_row"),
    Wfm(4097, 6, "tall", "lds_le_64k", "pairs"),                # the tall pass's tie rule: pairs of foreground rows an even gap apart
    Wfm(700, 9, "segmented", "lds_le_64k", "pairs"),
    Wfm(700, 9, "segmented", "lds_le_64k", "far_apart"),        # two foreground rows 600 apart: carries across empty segments, both ways
    Wfm(130, 131, "segmented", "lds_le_64k", "alt_cols"),       # columns without foreground beside columns with some
    Wfm(65, 70, "segmented", "lds_le_64k", "corner"),
    Wfm(65, 70, "segmented", "lds_le_64k", "empty"),
    Wfm(65, 70, "segmented", "lds_le_64k", "full"),
)
WFM_REFUSED = ((3, 8193), (16385, 2))


def wfm_input(c: Wfm):
    """-> pre uint8 (N,h,w), prob f32 (N,h,w), gt uint8 (N,h,w); foreground levels are 255 and 129, background 0 and 128 (the threshold
    is > 128)"""
    rng = np.random.default_rng(_seed("wfm", c.id))
    shape = (c.N, c.h, c.w)
    fg = np.zeros(shape, bool)
    if c.gt == "sparse":
        for n in range(c.N):
            fg[n] = rng.random((c.h, c.w)) < (0.03 if c.h * c.w > 64 else 0.2) * (1 + n)
            if not fg[n].any():
                fg[n, c.h // 2, c.w // 2] = True
    elif c.gt == "first_row":
        fg[:, 0, ::2] = True
    elif c.gt == "last_row":
        fg[:, -1, ::2] = True
    elif c.gt == "pairs":                                         # rows y and y + 2k in one column: the row between them is a tie
        for x in range(c.w):
            y = 3 + x
            while y + 40 < c.h:
                gap = 2 * int(rng.integers(1, 20))
                fg[:, y, x] = fg[:, y + gap, x] = True
                y += gap + 2 * int(rng.integers(1, 60)) + 1
    elif c.gt == "far_apart":
        fg[:, 37, ::2] = True
        fg[:, 637, 1::3] = True
    elif c.gt == "alt_cols":
        fg[:, :, ::2] = rng.random((c.N, c.h, (c.w + 1) // 2)) < 0.02
        fg[:, :, 64:68] = False                                   # and a run of empty columns across the column-group edge
    elif c.gt == "corner":
        fg[:, -1, -1] = True
    elif c.gt == "full":
        fg[:] = True
    elif c.gt != "empty":
        raise ValueError(c.gt)
    gt = np.where(fg, np.where(rng.random(shape) < 0.5, 255, 129), np.where(rng.random(shape) < 0.5, 0, 128)).astype(np.uint8)
    pre = rng.integers(0, 256, shape, dtype=np.uint8)
    prob = rng.random(shape, dtype=np.float32)
    return pre, prob, gt


def wfm_parts(pred: np.ndarray, gt: np.ndarray):
    """`metrics_oracle.wfm` (WeightedFmeasure.cal_wfm) on a prepared prediction `pred` (float64, one image) and a bool ground truth, taken
    apart: -> (sums f64 [3] = (sum Ew over gt, sum Ew over ~gt, |gt|), d2 int64 (h,w), Et f64 (h,w)) -- what cvlm_mask_wfm / cvlm_prob_wfm
    return and leave in their workspace.  The nearest foreground pixel is scipy's own (`return_indices`), ties included; d2 comes from
    those indices as integers.  None for an empty ground truth (the reference returns 0 before it transforms anything)."""
    from scipy.ndimage import convolve, distance_transform_edt as bwdist
    if not gt.any():
        return None
    dst, idx = bwdist(gt == 0, return_indices=True)
    yy, xx = np.mgrid[0:gt.shape[0], 0:gt.shape[1]]
    d2 = (idx[0].astype(np.int64) - yy) ** 2 + (idx[1].astype(np.int64) - xx) ** 2
    e = np.abs(pred - gt)
    et = np.copy(e)
    et[gt == 0] = et[idx[0][gt == 0], idx[1][gt == 0]]
    ea = convolve(et, weights=M.gauss2d((7, 7), sigma=5), mode="constant", cval=0)
    ew = np.where(gt & (ea < e), ea, e) * np.where(gt == 0, 2 - np.exp(np.log(0.5) / 5 * dst), 1.0)
    return np.asarray([ew[gt].sum(), ew[~gt].sum(), gt.sum()], dtype=np.float64), d2, et


def wfm_value(sums, beta: float = 1.0) -> float:
    """the last lines of cal_wfm from the three sums, as metrics_oracle.wfm writes them"""
    s_fg, s_bg, n1 = (float(v) for v in sums)
    if n1 == 0:
        return 0.0
    tpw = n1 - s_fg
    r = 1 - s_fg / n1
    p = tpw / (tpw + s_bg + np.spacing(1))
    return float((1 + beta) * r * p / (r + beta * p + np.spacing(1)))


def prob_prepared(p: np.ndarray) -> np.ndarray:
    """utils.calc_cod's prepared prediction of one float32 map, in numpy's float32 operations (p * 255, / 255, min-max)"""
    pred = (p * np.float32(255)) / 255
    mn, mx = pred.min(), pred.max()
    return (pred - mn) / (mx - mn) if mx != mn else pred


def edt_kernel_rule(fg: np.ndarray):
    """The nearest foreground pixel by the rule csrc/evaltail.hip states for its two passes: inside each column the nearest foreground
    row, ties to the smaller row; then along the row the column minimising dx^2 + dy^2, ties to the smaller column.  -> (d2, iy, ix)
    int64, or None without foreground.  Brute force over candidate columns: for the sizes of WFM_CASES only."""
    h, w = fg.shape
    if not fg.any():
        return None
    big = 1 << 29
    rows = np.arange(h, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(fg, rows, -1), axis=0)
    below = np.minimum.accumulate(np.where(fg, rows, big)[::-1], axis=0)[::-1]
    near = np.where((below < big) & ((above < 0) | (below - rows < rows - above)), below, above)       # (h, w); -1: an empty column
    cols = np.nonzero(fg.any(axis=0))[0].astype(np.int64)
    dy2 = (near[:, cols] - rows) ** 2                                                                  # (h, cand)
    d2 = np.empty((h, w), np.int64)
    ix = np.empty((h, w), np.int64)
    xs = np.arange(w, dtype=np.int64)
    for y in range(h):
        for x0 in range(0, w, 1024):
            d = (xs[x0:x0 + 1024, None] - cols[None, :]) ** 2 + dy2[y][None, :]
            j = d.argmin(axis=1)                                                                       # the first minimum: the smaller column
            d2[y, x0:x0 + 1024] = d[np.arange(len(j)), j]
            ix[y, x0:x0 + 1024] = cols[j]
    iy = near[np.arange(h)[:, None], ix]
    return d2, iy, ix


# ---- joint histogram / centroid cases -------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Hist:
    N: int
    h: int
    w: int
    off: int = 0                # bytes past a 16-byte boundary, both inputs
    pre: str = "random"         # random | flat
    gt: str = "blob"            # blob | last_px | last_row | last_col | empty
    vec: bool = False           # the 16-byte path: h * w % 16 == 0 and both image pointers 16-byte aligned

    @property
    def id(self) -> str:
        return f"n{self.N}-{self.h}x{self.w}-off{self.off}-{self.pre}-{self.gt}"


HIST_CASES = (
    Hist(1, 16, 32, vec=True),
    Hist(1, 16, 32, off=1),                  # h * w % 16 == 0, a view one byte into a larger buffer
    Hist(1, 16, 32, off=8),
    Hist(3, 4, 12, vec=True),                # N = 3, every image on the vector path
    Hist(3, 16, 5, vec=True),                # w < 16: a run of 16 pixels crosses rows
    Hist(3, 7, 9),                           # h * w % 16 != 0: images 1 and 2 start off a boundary as well
    Hist(2, 40, 5),                          # w < 16, the scalar path
    Hist(2, 3, 4),                           # h * w < 16
    Hist(2, 1, 1),
    Hist(1, 33, 48, pre="flat", vec=True),   # 99 runs: a flat prediction on a partial second wave
    Hist(1, 33, 47, pre="flat"),
    Hist(1, 21, 31, gt="last_px"),           # centroid on the last row and column
    Hist(1, 16, 32, gt="last_row", vec=True),
    Hist(1, 21, 31, gt="last_col"),
    Hist(1, 9, 23, gt="empty"),
)


def hist_input(c: Hist):
    rng = np.random.default_rng(_seed("hist", c.id))
    shape = (c.N, c.h, c.w)
    pre = np.full(shape, 200, np.uint8) if c.pre == "flat" else rng.integers(0, 256, shape, dtype=np.uint8)
    gt = rng.integers(0, 129, shape, dtype=np.uint8)                       # background levels up to 128
    if c.gt == "blob":
        for n in range(c.N):
            y0, x0 = int(rng.integers(0, c.h)), int(rng.integers(0, c.w))
            gt[n, y0:y0 + max(1, c.h // 2), x0:x0 + max(1, c.w // 3)] = rng.integers(129, 256)
    elif c.gt == "last_px":
        gt[:, -1, -1] = 255
    elif c.gt == "last_row":
        gt[:, -1, :] = 129
    elif c.gt == "last_col":
        gt[:, :, -1] = 255
    return pre, gt


def hist_vec(c: Hist, pre_ptr: int, gt_ptr: int):
    """gt_centroid_kernel / joint_hist_kernel (csrc/evaltail.hip, `vec`): per image, 16-byte loads iff h * w % 16 == 0 and the image's
    pointers are 16-byte aligned -> one bool per image"""
    hw = c.h * c.w
    return [hw % 16 == 0 and (pre_ptr + n * hw) % 16 == 0 and (gt_ptr + n * hw) % 16 == 0 for n in range(c.N)]


def counts_numpy(pre, gt):
    """what cvlm_mask_joint_hist returns, built with numpy"""
    h, w = gt.shape
    g = gt > 128
    ys, xs = np.nonzero(g)
    stats = np.asarray([g.sum(), xs.sum(), ys.sum()], dtype=np.int64)
    cx, cy = M.centroid(g)
    yy, xx = np.mgrid[0:h, 0:w]
    quad = (yy >= cy) * 2 + (xx >= cx)
    hist = np.zeros((4, 2, 256), dtype=np.int64)
    np.add.at(hist, (quad.ravel(), g.ravel().astype(np.int64), pre.ravel().astype(np.int64)), 1)
    return stats, hist


def cod_counts_numpy(p, g):
    """what cod_counts returns for one image (without the weighted-F sums), built with numpy in the reference's float32 operations"""
    h, w = g.shape
    gt = g > 128
    pred = (p * np.float32(255)) / 255
    mn, mx = pred.min(), pred.max()
    pn = (pred - mn) / (mx - mn) if mx != mn else pred
    q = (pn * 255).astype(np.uint8)
    stats, hist = counts_numpy(q, g)
    cx, cy = M.centroid(gt)
    yy, xx = np.mgrid[0:h, 0:w]
    quad = (yy >= cy) * 2 + (xx >= cx)
    mom = np.zeros((4, 2, 2), dtype=np.float64)
    for k in range(4):
        for c in range(2):
            v = pn[(quad == k) & (gt == bool(c))].astype(np.float64)
            mom[k, c] = (v.sum(), (v * v).sum())
    return stats, hist, mom, pn, gt


# ---- mask -> uint8, exact -----------------------------------------------------------------------------------------------------------------
# logits from {-40, 0, +40}: sigmoid = below 1e-17 / exactly 0.5 / exactly 1 in float32 whatever the last bit of exp, and every later step
# is the oracle's fp32 products and sums
MASK_SOURCES = ((1, 1), (1, 5), (2, 3), (64, 64))
MASK_TARGETS = ((1, 1), (5, 1), (1, 7), (97, 131), None)       # None: the source's own size
MASK_N = 3


def mask_logits(src) -> np.ndarray:
    rng = np.random.default_rng(_seed("mask", src))
    return rng.choice(np.asarray([-40.0, 0.0, 40.0], np.float32), size=(MASK_N,) + tuple(src))


# ---- calc_cod cases -----------------------------------------------------------------------------------------------------------------------
COD_CASES = ("constant", "two_values", "8x8", "5x300", "n3_ranges")


def cod_input(name: str):
    """-> prob f32 (N,1,h,w), gt f32 {0, 1} (N,1,h,w)"""
    rng = np.random.default_rng(_seed("cod", name))
    if name == "constant":                                       # max == min: the un-normalised branch
        prob = np.full((1, 1, 40, 52), 0.3, np.float32)
    elif name == "two_values":
        prob = np.where(rng.random((1, 1, 40, 52)) < 0.4, np.float32(0.2), np.float32(0.7)).astype(np.float32)
    elif name == "8x8":                                          # 64 pixels on 64 workgroups of 256 threads: most hold (+inf, -inf)
        prob = rng.random((1, 1, 8, 8), dtype=np.float32)
    elif name == "5x300":
        prob = rng.random((1, 1, 5, 300), dtype=np.float32)
    elif name == "n3_ranges":                                    # one image's range must not reach another's
        prob = rng.random((3, 1, 33, 47), dtype=np.float32)
        prob[0] = 0.1 + 0.3 * prob[0]
        prob[1] = 0.5 + 0.4 * prob[1]
        prob[2, 0, 0, 0], prob[2, 0, -1, -1] = 0.0, 1.0
    else:
        raise ValueError(name)
    n, _, h, w = prob.shape
    gt = np.zeros((n, 1, h, w), np.float32)
    for k in range(n):
        gt[k, 0, h // 4 + k:h - h // 4, w // 4 + 2 * k:w - w // 4] = 1
    return prob, gt
