"""The cases of the split-1 GEMM tests: every launch form of the cascade in precision `fast` (engine.py: Precision(1, 1, 1), every
cvlm_gemm with split = 1) on each of the four instantiations csrc/gemm_plan.h keeps for split 1 only,

    CVLM_GEMM_VARIANT=1   gemm_nt_kernel<1, 2, 2, 2, 32>           128 x 128 tiles, two-slot loop, one staging slab per wave (NBUF == 1)
    CVLM_GEMM_VARIANT=2   gemm_nt_kernel<1, 4, 2, 3, 32>           256 x 128 tiles, three-slot ring
    CVLM_GEMM_VARIANT=5   gemm_nt_kernel<1, 2, 4, 3, 32, 0, 8>     256 x 256 tiles, three-slot ring, eight waves of 128 x 64
    conv3x3 = (H, W, C)   gemm_nt_kernel<1, 4, 1, 2, 32, .., true> 256 x 64 tiles, implicit 3x3 convolution

at shapes on the tile and ring edges.  tests/test_gemm_split1_cpu.py plans every case (no GPU) and checks that it reaches the kernel it
names; tests/test_gemm_split1_gpu.py runs them against fp64.  `launch` builds the operands and the keyword arguments of hip.gemm of a
case on any device, so both files look at the same launch; tests/gemm_split3_cases.py builds the split-3 launches with it too (both
planes real, images, a workspace, guard rows)."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Tuple

import torch

KERNELS = {
    "1": "gemm_nt_kernel<1, 2, 2, 2, 32, 0, 4, false, -1, false, false, false, false, false>",
    "2": "gemm_nt_kernel<1, 4, 2, 3, 32, 0, 4, false, -1, false, false, false, false, false>",
    "5": "gemm_nt_kernel<1, 2, 4, 3, 32, 0, 8, false, -1, false, false, false, false, false>",
    "conv": "gemm_nt_kernel<1, 4, 1, 2, 32, 0, 4, false, -1, true, false, false, false, false>",
}
PLAIN_KERNELS = ("1", "2", "5")

# (M, N, K): R = 3 slots in the ring of variants 2 and 5, nk = K / 32 K-tiles
SHAPES = (
    (70, 36, 32),        # one ragged tile; N % 8 == 4: direct-store epilogue; nk = 1 < R - 1
    (257, 129, 64),      # one row and one column past a tile edge; odd N: scalar tail stores; nk = 2
    (300, 264, 96),      # ragged both ways; N % 8 == 0: LDS-staged epilogue; nk = 3 = R
    (520, 392, 160),     # 3 x 2 tiles of 256^2, 5 x 4 of 128^2; nk = 5 > R: the ring wraps
    (300, 264, 1280),    # long K through the ring: 40 K-tiles
)
STAGED_SHAPES = tuple(s for s in SHAPES if s[1] % 8 == 0)             # the fold and h2-residual forms need 8-column row pieces
BATCHED_SHAPE = (3, 96, 80, 64)                                       # (batch, M, N, K)
PIXEL_SHUFFLE_SHAPES = ((2, 6, 5, 64, 16), (2, 12, 11, 32, 8))        # (Bn, H, W, Cin, Cout); the second: M = 264, a ragged second row tile
HEAD_MAJOR_SHAPES = ((256, 80), (200, 80), (50, 20))                  # (S, hd) at Bn = 2, heads = 2, K = 64
CONV_SHAPES = ((2, 20, 24, 32, 64), (3, 9, 7, 64, 32), (1, 16, 16, 128, 40))   # (Bn, H, W, C, N)
PARITY_SHAPE = (520, 392, 160)                                        # the three plain kernels against each other

ALPHA, OUT_SCALE, XS = 0.5, 0.25, 0.25
ACT_ABS_POST = 4
# leading dimensions of the plain form, as offsets from N: (ldo, ldr, ldoh)
LAYOUTS = {
    "tight": (0, 0, 0),
    "padded": (4, 4, 8),         # N % 8 == 0: still the LDS-staged path, with padding columns
    "odd": (1, None, 0),         # ldo = N + 1 and an odd ldr: vec_f32 / vec_res false
    "h2_direct": (0, 0, 4),      # ldoh = N + 4: the h2 store (and with it the launch) on the direct path
}


@dataclass(frozen=True)
class Case:
    kernel: str                  # CVLM_GEMM_VARIANT that forces it, or "conv"
    form: str                    # product | plain | batched | pixel_shuffle | head_major | ln_fold | h2_residual | conv
    shape: Tuple[int, ...]
    act: int = 0
    layout: str = "tight"
    nolo: int = 0

    @property
    def id(self) -> str:
        s = f"k{self.kernel}-{self.form}-" + "x".join(str(v) for v in self.shape)
        if self.form in ("plain", "ln_fold"):
            s += f"-act{self.act}"
        if self.form == "plain":
            s += "-" + self.layout
        if self.form == "head_major":
            s += f"-nolo{self.nolo}"
        return s


def _cases():
    out = []
    for k in PLAIN_KERNELS:
        for i, shape in enumerate(SHAPES):
            out.append(Case(k, "product", shape))
            out += [Case(k, "plain", shape, act=act) for act in (0, 1, 2, 3)]
            # the three other layouts once per shape, the activation rotating with them
            out += [Case(k, "plain", shape, act=(i + j) % 4, layout=lay) for j, lay in enumerate(("padded", "odd", "h2_direct"))]
        out.append(Case(k, "batched", BATCHED_SHAPE, act=ACT_ABS_POST))
        out += [Case(k, "pixel_shuffle", s) for s in PIXEL_SHUFFLE_SHAPES]
        out += [Case(k, "head_major", s, nolo=nolo) for s in HEAD_MAJOR_SHAPES for nolo in (0, 2, 5)]
        out += [Case(k, "ln_fold", s, act=act) for s in STAGED_SHAPES for act in (0, 1, 2)]
        out += [Case(k, "h2_residual", s) for s in STAGED_SHAPES]
    out += [Case("conv", "conv", s) for s in CONV_SHAPES]
    return tuple(out)


CASES = _cases()
# one case per kernel that runs a second time with the true lo planes of A and W: the same bits
TRUE_LO_CASES = tuple(Case(k, "plain", (300, 264, 96), act=1) for k in PLAIN_KERNELS) + (Case("conv", "conv", CONV_SHAPES[0]),)
assert all(c in CASES for c in TRUE_LO_CASES)


def of(form: str, kernel: str = None):
    return [c for c in CASES if c.form == form and (kernel is None or c.kernel == kernel)]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def operand(hip, x, device, true_lo=False):
    """H2.pack(x) with the lo plane replaced by NaN: a split-1 launch must not read it."""
    t = hip.H2.pack(x).t
    if not true_lo:
        t[1] = float("nan")
    return hip.H2(t.to(device))


def launch(case, hip, device, true_lo=False, *, split=1, guard=0, w_il=False, a_il=False, out_il=False, workspace=None) -> SimpleNamespace:
    """The operands, prefilled outputs and hip.gemm keyword arguments of a case: A, W (h2; split 1: lo planes NaN unless true_lo; split 3:
    both planes real), M, N, K, kw, and `host`, the f32 tensors they were packed from plus whatever else the reference needs.  Outputs
    are prefilled with NaN (7.0: the half planes of the head-major cases).

    guard: rows allocated and prefilled behind row M of every output and of the row-statistics pieces; `guards` lists them (they must
    still hold the prefill after the launch).  w_il / a_il: the weight's interleaved image is passed / the activation travels as its
    128-byte-row image (`A` is an H2IL, `planar_A` the planes).  out_il: the h2 output (and the in-place h2 residual) is an image
    `out_img` of `out_cols` columns; `out_h2` is None then.  workspace: passed on."""
    f = case.form
    nan = float("nan")
    host = SimpleNamespace()
    kw = dict(split=split)
    if f in ("product", "plain", "ln_fold", "h2_residual"):
        M, N, K = case.shape
        a, w = rnd(M, K, seed=101), rnd(N, K, seed=102, scale=K ** -0.5)
    elif f == "batched":
        Bz, M, N, K = case.shape
        a, w = rnd(M, K, seed=103), rnd(Bz * N, K, seed=104, scale=K ** -0.5)
    elif f == "pixel_shuffle":
        Bn, H, Wd, Cin, Cout = case.shape
        M, N, K = Bn * H * Wd, 4 * Cout, Cin
        a, w = rnd(M, K, seed=105), rnd(N, K, seed=106, scale=K ** -0.5)       # weight rows (dy, dx, co)
    elif f == "head_major":
        S, hd = case.shape[:2]                                                 # (S, hd) or (S, hd, K, Bn, heads)
        K, Bn, Hh = tuple(case.shape[2:]) + (64, 2, 2)[len(case.shape) - 2:]
        M, N = Bn * S, 3 * Hh * hd
        a, w = rnd(M, K, seed=107), rnd(N, K, seed=108, scale=K ** -0.5)
    elif f == "conv":
        Bn, H, Wd, Cc, N = case.shape
        M, K = Bn * H * Wd, 9 * Cc
        a, w = rnd(M, Cc, seed=109), rnd(N, K, seed=110, scale=K ** -0.5)      # NHWC image; weight columns (ky, kx, c)
    else:
        raise ValueError(f)
    host.a, host.w = a, w
    true_lo = true_lo or split == 3
    A, W = operand(hip, a, device, true_lo), operand(hip, w, device, true_lo)
    planar_A = A
    if w_il or a_il:
        kw.update(w_il=hip.interleave_planes(W))
    if a_il:
        A = hip.H2IL.from_planes(A)
    if workspace is not None:
        kw.update(workspace=workspace)
    guards = []

    def rows_of(full, rows, axis=0):
        """the first `rows` rows of `full` (a view with the same base address: what the launch is given); the rest are guard rows"""
        if full.shape[axis] > rows:
            guards.append(full.narrow(axis, rows, full.shape[axis] - rows))
        return full.narrow(axis, 0, rows)

    def new_f32(rows, cols):
        return rows_of(torch.full((rows + guard, cols), nan, device=device), rows)

    def new_h2(cols, fill=nan):
        return hip.H2(rows_of(torch.full((2, M + guard, cols), fill, dtype=torch.float16, device=device), M, axis=1))

    out_cols = N + 64 - N % 32                                                 # image width: a multiple of 32, wider than N
    out_f32 = out_h2 = out_img = None
    if f == "product":
        out_f32 = new_f32(M, N)
        kw.update(out_f32=out_f32)
    elif f == "plain":
        dldo, dldr, dldoh = LAYOUTS[case.layout]
        ldo, ldoh = N + dldo, N + dldoh
        ldr = N + dldr if dldr is not None else N + 1 + N % 2
        host.bias, host.res = rnd(N, seed=111), rnd(M, ldr, seed=112)
        out_f32 = new_f32(M, ldo)
        if out_il:
            out_img = hip.H2IL(rows_of(torch.full((M + guard, 2 * out_cols), nan, dtype=torch.float16, device=device), M))
            kw.update(out_h2=out_img)
        else:
            out_h2 = new_h2(ldoh)
            kw.update(out_h2=out_h2, ldoh=ldoh)
        kw.update(bias=host.bias.to(device), residual=host.res.to(device), ldr=ldr, out_f32=out_f32, ldo=ldo,
                  act=case.act, alpha=ALPHA, out_scale=OUT_SCALE)
    elif f == "batched":
        host.res = rnd(Bz, M, N, seed=113)
        out_f32 = new_f32(Bz * M, N).view(Bz, M, N)
        kw.update(residual=host.res.to(device), out_f32=out_f32, act=ACT_ABS_POST, alpha=-1.0, batch=Bz, stride_a=0, stride_w=N * K,
                  stride_r=M * N, stride_o=M * N)
    elif f == "pixel_shuffle":
        host.bias = rnd(Cout, seed=114)
        out_f32 = new_f32(Bn * 2 * H * 2 * Wd, Cout).view(Bn, 2 * H, 2 * Wd, Cout)
        kw.update(bias=host.bias.repeat(4).to(device), out_f32=out_f32, pixel_shuffle=(H, Wd, 2 * Cout))
    elif f == "head_major":
        host.bias = rnd(N, seed=115)
        out_h2 = new_h2(N, 7.0)
        kw.update(bias=host.bias.to(device), out_h2=out_h2, head_major=(S, Hh, hd), head_major_nolo=case.nolo)
    elif f == "ln_fold":
        host.bias, host.colsum = rnd(N, seed=116), rnd(N, seed=117)
        host.stats = torch.stack([0.5 + rnd(M, seed=118).abs(), 0.3 * rnd(M, seed=119)], 1).contiguous()   # (rstd, mu * rstd)
        if out_il:
            out_img = hip.H2IL(rows_of(torch.full((M + guard, 2 * out_cols), nan, dtype=torch.float16, device=device), M))
        else:
            out_h2 = new_h2(N)
        kw.update(bias=host.bias.to(device), out_h2=out_img if out_il else out_h2, act=case.act, alpha=ALPHA, out_scale=OUT_SCALE,
                  ln_fold=(host.stats.to(device), host.colsum.to(device)))
    elif f == "h2_residual":
        host.bias = rnd(N, seed=120)
        x_old = rnd(M, N, seed=121)
        x_old[:, 3] *= 1e3                                                     # massive channels, like real ViT residual streams
        x_old[:, N // 2] *= 300.0
        host.x_old = hip.H2.pack(x_old * XS)                                   # both planes real: this form reads the residual's lo plane
        pieces = hip.stats_pieces(N)
        stats = new_f32(pieces * M, 2).view(pieces, M, 2)
        if out_il:                                                             # in place: the output image is the residual image
            pl = torch.full((2, M + guard, out_cols), nan, dtype=torch.float16, device=device)
            pl[:, :M, :N] = host.x_old.t.to(device)
            out_img = hip.H2IL(rows_of(hip.interleave_planes(hip.H2(pl)), M))
            kw.update(out_h2=out_img, residual_h2=(out_img, 1.0 / XS))
        else:
            out_h2 = new_h2(N)
            out_h2.t.copy_(host.x_old.t)                                       # in place: the output is the residual
            kw.update(out_h2=out_h2, residual_h2=(out_h2, 1.0 / XS))
        kw.update(bias=host.bias.to(device), out_scale=XS, row_stats=stats, alpha=ALPHA)
    elif f == "conv":
        host.bias, host.res = rnd(N, seed=122), rnd(M, N, seed=123)
        out_f32 = new_f32(M, N)
        kw.update(bias=host.bias.to(device), residual=host.res.to(device), out_f32=out_f32, conv3x3=(H, Wd, Cc))
    return SimpleNamespace(case=case, A=A, planar_A=planar_A, W=W, M=M, N=N, K=K, kw=kw, host=host, out_f32=out_f32, out_h2=out_h2,
                           out_img=out_img, out_cols=out_cols, guards=guards)
