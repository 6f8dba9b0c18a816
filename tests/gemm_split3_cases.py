"""The cases of the split-3 GEMM tests: every gemm_nt_kernel instantiation csrc/gemm_plan.h keeps for precision `exact` (split = 3; the
mx kernels are tests/test_gemm_mx_gpu.py's), each named by the environment that forces it, in every launch form gemm_validate and the
planner admit on it, at shapes on its tile and ring edges.  tests/test_gemm_split3_cpu.py plans every case (no GPU) and checks that it
reaches the kernel it names; tests/test_gemm_split3_gpu.py runs them against fp64.  Operands, outputs and keyword arguments come from
gemm_split1_cases.launch (split = 3: both planes real; guard rows behind every output).

    key      instantiation <3, WM, WN, NSTAGE, 32, 0, MT, PERSIST, EPI, CONV, SK>    tile       ring  environment (CVLM_GEMM_*)
    r2       <2, 2, 2>                                                                 128 x 128  2     VARIANT=1 RING=2 W8=0
    r3       <2, 2, 13>                                                                128 x 128  3     VARIANT=1 RING=3 W8=0
    r4       <2, 2, 14>                                                                128 x 128  4     VARIANT=1 RING=4 W8=0
    r5       <2, 2, 15>                                                                128 x 128  5     VARIANT=1 RING=5 W8=0
    w64      <4, 2, 14, MT 1>   eight waves of 16 x 64                                 64 x 128   4     VARIANT=1 RING=4 W8=2
    w128     <4, 2, 14, MT 2>   eight waves of 32 x 64                                 128 x 128  4     VARIANT=1 RING=4 W8=3
    sk_r2    <2, 2, 2, SK>      K-parts of every tile, slabs in the workspace          128 x 128  2     VARIANT=1 RING=2 W8=0 SK=parts
    sk_r3    <2, 2, 13, SK>                                                            128 x 128  3     VARIANT=1 RING=3 W8=0 SK=parts
    sk_r4    <2, 2, 14, SK>                                                            128 x 128  4     VARIANT=1 RING=4 W8=0 SK=parts
    sk_w8    <4, 2, 14, MT 2, SK>                                                      128 x 128  4     VARIANT=1 RING=4 W8=1 SK=parts
    k2       <4, 2, 3>                                                                 256 x 128  3     VARIANT=2
    g256     <2, 4, 5, MT 8>    every epilogue form: what the staged path cannot store 256 x 256  5     VARIANT=7
    e0/1/2   <2, 4, 5, MT 8, false, EPI>   one workgroup per tile                      256 x 256  5     VARIANT=7 PERSIST=0 TAIL=0
             ... with a workspace and TAIL=1: the last round's tiles as chained K-parts
    p0/1/2   <2, 4, 5, MT 8, true, EPI>    one workgroup per CU, more tiles than CUs   256 x 256  5     VARIANT=7 PERSIST=1 TAIL=0
    t192     <2, 4, 5, MT 6, false, 2>     h2-residual form, M > 4096                  192 x 256  5     VARIANT=0 T192=1, no workspace
    conv     <4, 1, 2, CONV>    implicit 3 x 3 convolution                             256 x 64   2     conv3x3 = (H, W, C)
    X-w      the WIL twin of X: w_il given;  X-wa: the WIL + AIL twin: w_il and a_il given.  An activation image is refused under
             VARIANT=1, so the -wa twins of w64 / w128 / sk_w8 run under VARIANT=0, where the small-grid model picks the 128^2 family
             for their shapes (and SK=parts forces the K-parts).

What the planner admits (asserted by the CPU test through the plan of every case): a batched launch is not `one3`, so of the 128^2
family only r2 runs it; SK needs one problem; the staged forms (N % 8 == 0, aligned leading dimensions, head-major with 8 | hd and
S >= 128) under VARIANT=7 go to e0 / e1 / e2 (p0 / p1 / p2 with more tiles than CUs), so g256 sees only N % 8 != 0, odd leading
dimensions, pixel shuffle, batches and the head-major stores the staged path refuses, and never the fold or the h2 residual; t192 needs
0.0685 K + 14 us to beat two rounds of 256 x 128 tiles, i.e. K >= 512: its K-tile count is never near the ring depth."""
import dataclasses
from dataclasses import dataclass
from typing import Tuple

import gemm_split1_cases as S1


def _b(v):
    return "true" if v else "false"


def kernel_name(wm, wn, nstage, mt=4, persist=False, epi=-1, conv=False, sk=False, wil=False, ail=False):
    return (f"gemm_nt_kernel<3, {wm}, {wn}, {nstage}, 32, 0, {mt}, {_b(persist)}, {epi}, {_b(conv)}, {_b(sk)}, {_b(wil)}, {_b(ail)}, "
            "false>")


@dataclass(frozen=True)
class Kernel:
    key: str
    args: Tuple                  # (wm, wn, nstage, mt, persist, epi, conv, sk)
    env: Tuple[Tuple[str, str], ...]
    tile: Tuple[int, int]
    ring: int
    kind: str                    # generic | g256 | sk | epi0 | epi1 | epi2 | t192 | conv
    il: str = ""                 # "": planar operands; "w": weight image; "wa": weight and activation image
    base: str = ""               # the planar kernel an image twin is compared with

    @property
    def name(self):
        wm, wn, nstage, mt, persist, epi, conv, sk = self.args
        return kernel_name(wm, wn, nstage, mt, persist, epi, conv, sk, self.il != "", self.il == "wa")

    @property
    def tiling(self):
        return f"{self.tile[0]}x{self.tile[1]}"

    @property
    def persist(self):
        return self.args[4]


def _env(**kw):
    return tuple(sorted(("CVLM_GEMM_" + k, str(v)) for k, v in kw.items()))


_PLANAR = (
    Kernel("r2", (2, 2, 2, 4, False, -1, False, False), _env(VARIANT=1, RING=2, W8=0), (128, 128), 2, "generic"),
    Kernel("r3", (2, 2, 13, 4, False, -1, False, False), _env(VARIANT=1, RING=3, W8=0), (128, 128), 3, "generic"),
    Kernel("r4", (2, 2, 14, 4, False, -1, False, False), _env(VARIANT=1, RING=4, W8=0), (128, 128), 4, "generic"),
    Kernel("r5", (2, 2, 15, 4, False, -1, False, False), _env(VARIANT=1, RING=5, W8=0), (128, 128), 5, "generic"),
    Kernel("w64", (4, 2, 14, 1, False, -1, False, False), _env(VARIANT=1, RING=4, W8=2), (64, 128), 4, "generic"),
    Kernel("w128", (4, 2, 14, 2, False, -1, False, False), _env(VARIANT=1, RING=4, W8=3), (128, 128), 4, "generic"),
    Kernel("sk_r2", (2, 2, 2, 4, False, -1, False, True), _env(VARIANT=1, RING=2, W8=0), (128, 128), 2, "sk"),
    Kernel("sk_r3", (2, 2, 13, 4, False, -1, False, True), _env(VARIANT=1, RING=3, W8=0), (128, 128), 3, "sk"),
    Kernel("sk_r4", (2, 2, 14, 4, False, -1, False, True), _env(VARIANT=1, RING=4, W8=0), (128, 128), 4, "sk"),
    Kernel("sk_w8", (4, 2, 14, 2, False, -1, False, True), _env(VARIANT=1, RING=4, W8=1), (128, 128), 4, "sk"),
    Kernel("k2", (4, 2, 3, 4, False, -1, False, False), _env(VARIANT=2), (256, 128), 3, "generic"),
    Kernel("g256", (2, 4, 5, 8, False, -1, False, False), _env(VARIANT=7), (256, 256), 5, "g256"),
    Kernel("e0", (2, 4, 5, 8, False, 0, False, False), _env(VARIANT=7, PERSIST=0, TAIL=0), (256, 256), 5, "epi0"),
    Kernel("e1", (2, 4, 5, 8, False, 1, False, False), _env(VARIANT=7, PERSIST=0, TAIL=0), (256, 256), 5, "epi1"),
    Kernel("e2", (2, 4, 5, 8, False, 2, False, False), _env(VARIANT=7, PERSIST=0, TAIL=0), (256, 256), 5, "epi2"),
    Kernel("p0", (2, 4, 5, 8, True, 0, False, False), _env(VARIANT=7, PERSIST=1, TAIL=0), (256, 256), 5, "epi0"),
    Kernel("p1", (2, 4, 5, 8, True, 1, False, False), _env(VARIANT=7, PERSIST=1, TAIL=0), (256, 256), 5, "epi1"),
    Kernel("p2", (2, 4, 5, 8, True, 2, False, False), _env(VARIANT=7, PERSIST=1, TAIL=0), (256, 256), 5, "epi2"),
    Kernel("t192", (2, 4, 5, 6, False, 2, False, False), _env(VARIANT=0, T192=1), (192, 256), 5, "t192"),
    Kernel("conv", (4, 1, 2, 4, False, -1, True, False), (), (256, 64), 2, "conv"),
)
# the planar kernels gemm_plan.h lists under CVLM_X_IL: a weight-image twin and a weight-and-activation-image twin each
IL_BASES = ("e0", "e1", "e2", "p0", "p1", "p2", "t192", "k2", "w64", "w128", "sk_w8")


def _twins():
    out = []
    for k in _PLANAR:
        if k.key in IL_BASES:
            for il in ("w", "wa"):
                env = dict(k.env)
                if il == "wa" and env.get("CVLM_GEMM_VARIANT") == "1":
                    env["CVLM_GEMM_VARIANT"] = "0"                   # an activation image is refused under VARIANT=1
                out.append(dataclasses.replace(k, key=f"{k.key}-{il}", env=tuple(sorted(env.items())), il=il, base=k.key))
    return tuple(out)


KERNELS = {k.key: k for k in _PLANAR + _twins()}
TILINGS = ("128x128", "64x128", "256x128", "256x256", "192x256")

TALL = -1                        # M (or the batch of a head-major case) of a persistent case: from the CU count, see resolve()


def tall_rows(cus):
    """rows of a tall thin problem with more 256^2 tiles than CUs at N = 264, ragged both ways"""
    return (cus // 2 + 2) * 256 + 1


@dataclass(frozen=True)
class Case:
    kernel: str                  # key of KERNELS
    form: str                    # product | plain | batched | pixel_shuffle | head_major | ln_fold | h2_residual | conv
    shape: Tuple[int, ...]
    act: int = 0
    layout: str = "tight"
    nolo: int = 0
    outs: str = "both"           # plain form: "both" f32 and h2 outputs, "h2" / "f32" only that one
    parts: int = 1               # SK kernels: forced K-parts (CVLM_GEMM_SK); tail cases: the chained K-parts the planner must choose
    tail: bool = False           # 256^2 EPI kernel with a workspace and CVLM_GEMM_TAIL=1
    out_il: bool = False         # h2 output (and in-place h2 residual) as an image

    @property
    def id(self) -> str:
        s = f"{self.kernel}-{self.form}-" + "x".join("tall" if v == TALL else str(v) for v in self.shape)
        if self.form in ("plain", "ln_fold"):
            s += f"-act{self.act}"
        if self.form == "plain":
            s += "-" + self.layout + ("" if self.outs == "both" else "-" + self.outs)
        if self.form == "head_major":
            s += f"-nolo{self.nolo}"
        if self.parts > 1:
            s += f"-{'tail' if self.tail else 'sk'}{self.parts}"
        if self.out_il:
            s += "-outil"
        return s

    @property
    def k(self) -> Kernel:
        return KERNELS[self.kernel]

    @property
    def needs_ws(self) -> bool:
        return self.tail or self.k.kind == "sk"

    @property
    def env(self) -> dict:
        e = dict(self.k.env)
        if self.k.kind == "sk":
            e["CVLM_GEMM_SK"] = str(self.parts)
        if self.tail:
            e["CVLM_GEMM_TAIL"] = "1"
        return e

    def resolve(self, cus: int) -> "Case":
        """the case with the rows of its tall problem filled in for a device of `cus` compute units"""
        if TALL not in self.shape:
            return self
        fill = cus // 2 + 2 if self.form == "head_major" else tall_rows(cus)
        return dataclasses.replace(self, shape=tuple(fill if v == TALL else v for v in self.shape))


def shapes(k: Kernel):
    """(M, N, K) on the edges of kernel k: tile = (WM * MT * 16) x (WN * 64), ring of R slots, nk = K / 32 K-tiles"""
    (tm, tn), r = k.tile, k.ring
    return (
        (min(70, tm - 10), 36, 32),                     # one ragged tile; N % 8 == 4: direct-store epilogue; nk = 1
        (tm + 1, tn + 1, 32 * max(1, r - 1)),           # one row and one column past a tile edge; odd N: scalar tail stores; nk = R - 1
        (tm + 44, tn + 8, 32 * r),                      # ragged both ways; N % 64 == 8: LDS-staged, the last piece has 8 columns; nk = R
        (2 * tm + 8, tn + 136, 32 * (r + 1)),           # 3 x 3 tiles; nk = R + 1: the ring wraps
        (300, 264, 1280),                               # long K through the ring: 40 K-tiles
    )


# 256^2 kernels, ring of 5.  g256 sees only what the staged path cannot store: N % 8 != 0 here
G256_SHAPES = ((70, 36, 32), (257, 257, 128), (300, 268, 160), (520, 396, 192), (300, 268, 1280))
# (S, hd, K, Bn, heads) with hd % 8 == 4 and N = 3 * heads * hd no multiple of 8: the direct store, and the plain launch it is compared
# with stays on g256 too (at N % 8 == 0 that one is staged and goes to e0)
G256_HEAD_MAJOR = ((50, 20, 64, 2, 1), (100, 20, 64, 2, 3), (300, 44, 64, 2, 1))
EPI_SHAPES = ((70, 40, 32), (257, 264, 128), (300, 264, 160), (520, 520, 192), (300, 264, 1280))    # N % 8 == 0; nk = 1, R - 1, R, R + 1, 40
EPI_HEAD_MAJOR = ((256, 80), (200, 80), (128, 8, 160, 3, 11))      # hd % 8 == 0 and S >= 128: the staged store; the last: N = 264, nk = R
TALL_K = (32, 160, 192)                                             # persistent kernels: nk = 1, R, R + 1
TALL_HEAD_MAJOR = (257, 88, 160, TALL, 1)                           # M = (cus / 2 + 2) * 257, N = 264
TAIL_SHAPES = {2: (257, 264, 1024), 3: (257, 264, 2048), 4: (257, 264, 8192)}     # parts -> shape: 4 tail tiles, ragged both ways
T192_SHAPES = ((4104, 2056, 512), (4225, 2056, 512), (4104, 2056, 2048))          # last 192-row tile: 72 rows, 1 row; long K
# split-K: (parts, shape) with K / 32 >= 4 * parts; K-tiles per part 4, 5, 5 and an uneven 19 = 5 + 5 + 5 + 4
SK_SHAPES = ((2, (70, 36, 256)), (4, (129, 129, 640)), (8, (300, 264, 1280)), (4, (300, 264, 608)))
IL_SHAPES = {"256x256": ((257, 264, 128), (520, 520, 192)), "256x128": ((257, 136, 64), (520, 264, 128)),
             "128x128": ((129, 136, 96), (264, 264, 160)), "64x128": ((65, 136, 96), (136, 264, 160))}
IL_HEAD_MAJOR = (256, 80)                                           # an image launch stores head-major only at S >= 256
PARITY_SHAPE = (520, 392, 160)                                      # every non-persistent kernel that takes the plain form
FORMS_GENERIC = ("product", "plain", "batched", "pixel_shuffle", "head_major", "ln_fold", "h2_residual")


def _generic(key, shp, batched=True, head_major=S1.HEAD_MAJOR_SHAPES, staged=True, parts=1):
    out = []
    for i, shape in enumerate(shp):
        out.append(Case(key, "product", shape, parts=parts))
        out += [Case(key, "plain", shape, act=act, parts=parts) for act in (0, 1, 2, 3)]
        out += [Case(key, "plain", shape, act=(i + j) % 4, layout=lay, parts=parts) for j, lay in enumerate(("padded", "odd", "h2_direct"))]
        if staged and shape[1] % 8 == 0:
            out += [Case(key, "ln_fold", shape, act=act, parts=parts) for act in (0, 1, 2)]
            out.append(Case(key, "h2_residual", shape, parts=parts))
    if batched:
        out.append(Case(key, "batched", S1.BATCHED_SHAPE))
    out += [Case(key, "pixel_shuffle", s, parts=parts) for s in S1.PIXEL_SHUFFLE_SHAPES]
    out += [Case(key, "head_major", s, nolo=nolo, parts=parts) for s in head_major for nolo in (0, 2, 5)]
    return out


def _il_cases(k: Kernel):
    """the forms the il_any block of gemm_validate allows, on the image twin k of a planar kernel"""
    wa, out = k.il == "wa", []
    kind = k.kind
    if kind == "t192":
        return [Case(k.key, "h2_residual", T192_SHAPES[0]), Case(k.key, "h2_residual", T192_SHAPES[1], out_il=wa)]
    if k.persist:
        tall = (TALL, 264, 160)
        if kind == "epi0":
            return [Case(k.key, "plain", tall, act=1), Case(k.key, "plain", tall, act=2, layout="padded", out_il=wa),
                    Case(k.key, "head_major", TALL_HEAD_MAJOR, nolo=2)]
        if kind == "epi1":
            return [Case(k.key, "ln_fold", tall, act=1, out_il=wa)]
        return [Case(k.key, "h2_residual", tall, out_il=wa)]
    if kind == "sk":
        for i, parts in enumerate((2, 4, 8)):                       # four K-tiles per part, and the uneven split
            shape = (300, 264, 128 * parts)
            out.append(Case(k.key, "plain", shape, act=1 + i, parts=parts, out_il=wa and i == 1))
            out.append(Case(k.key, "ln_fold", shape, act=i, parts=parts, out_il=wa and i == 2))
            out.append(Case(k.key, "h2_residual", shape, parts=parts, out_il=wa and i == 0))
        out.append(Case(k.key, "plain", SK_SHAPES[3][1], act=0, layout="padded", parts=4, out_il=wa))
        return out
    for i, shape in enumerate(IL_SHAPES[k.tiling]):
        if kind in ("generic", "epi0"):
            out.append(Case(k.key, "plain", shape, act=1))
            out.append(Case(k.key, "plain", shape, act=2 + i, layout="padded", out_il=wa))
            out.append(Case(k.key, "plain", shape, act=0, outs="h2", out_il=wa))
        if kind in ("generic", "epi1"):
            out.append(Case(k.key, "ln_fold", shape, act=i + 1, out_il=wa))
        if kind in ("generic", "epi2"):
            out.append(Case(k.key, "h2_residual", shape, out_il=wa))
    if kind in ("generic", "epi0"):
        out.append(Case(k.key, "head_major", IL_HEAD_MAJOR, nolo=2))
    if kind in ("epi0", "epi1", "epi2"):                            # chained K-parts of the last round on the image twins too
        form, act = {"epi0": ("plain", 0), "epi1": ("ln_fold", 1), "epi2": ("h2_residual", 0)}[kind]
        out.append(Case(k.key, form, TAIL_SHAPES[2], act=act, parts=2, tail=True, out_il=wa))
    return out


def _cases():
    out = []
    for k in _PLANAR:
        key = k.key
        if k.kind == "generic":
            out += _generic(key, shapes(k), batched=key in ("r2", "k2"))
        elif k.kind == "g256":
            out += _generic(key, G256_SHAPES, head_major=G256_HEAD_MAJOR, staged=False)
        elif k.kind == "sk":
            for parts, shape in SK_SHAPES:
                out += [c for c in _generic(key, (shape,), batched=False, head_major=(), parts=parts) if c.form != "pixel_shuffle"]
            out += [Case(key, "pixel_shuffle", S1.PIXEL_SHUFFLE_SHAPES[1] [:3] + (256, 8), parts=2)]     # M = 264, K = 256
            out += [Case(key, "head_major", (200, 80, 256), nolo=nolo, parts=2) for nolo in (0, 2, 5)]
            out += [Case(key, "head_major", (50, 20, 512), nolo=2, parts=4)]
        elif k.kind in ("epi0", "epi1", "epi2") and not k.persist:
            for i, shape in enumerate(EPI_SHAPES):
                if k.kind == "epi0":
                    out.append(Case(key, "product", shape))
                    out += [Case(key, "plain", shape, act=act) for act in (0, 1, 2, 3)]
                    out.append(Case(key, "plain", shape, act=i % 4, layout="padded"))
                    out.append(Case(key, "plain", shape, act=(i + 1) % 4, outs="h2"))
                    out.append(Case(key, "plain", shape, act=(i + 2) % 4, outs="f32"))
                elif k.kind == "epi1":
                    out += [Case(key, "ln_fold", shape, act=act) for act in (0, 1, 2)]
                else:
                    out.append(Case(key, "h2_residual", shape))
            if k.kind == "epi0":
                out += [Case(key, "head_major", s, nolo=nolo) for s in EPI_HEAD_MAJOR for nolo in (0, 2, 5)]
            form, act = {"epi0": ("plain", 0), "epi1": ("ln_fold", 1), "epi2": ("h2_residual", 0)}[k.kind]
            out += [Case(key, form, shape, act=act, parts=parts, tail=True) for parts, shape in TAIL_SHAPES.items()]
        elif k.persist:
            for i, kk in enumerate(TALL_K):
                shape = (TALL, 264, kk)
                if k.kind == "epi0":
                    out.append(Case(key, "product", shape))
                    out.append(Case(key, "plain", shape, act=1 + i))
                    out.append(Case(key, "plain", shape, act=i, layout="padded"))
                    out.append(Case(key, "plain", shape, act=(i + 2) % 4, outs="h2"))
                    out.append(Case(key, "plain", shape, act=(i + 3) % 4, outs="f32"))
                elif k.kind == "epi1":
                    out.append(Case(key, "ln_fold", shape, act=i))
                else:
                    out.append(Case(key, "h2_residual", shape))
            if k.kind == "epi0":
                out += [Case(key, "head_major", TALL_HEAD_MAJOR, nolo=nolo) for nolo in (0, 2, 5)]
        elif k.kind == "t192":
            out += [Case(key, "h2_residual", s) for s in T192_SHAPES]
        elif k.kind == "conv":
            out += [Case(key, "conv", s) for s in S1.CONV_SHAPES]
    for k in KERNELS.values():
        if k.il:
            out += _il_cases(k)
    return tuple(out)


CASES = _cases()
# one launch on every kernel of a tiling (bit for bit) and across tilings (4e-6): one workgroup per tile ...
PARITY_CASES = tuple(Case(k, "plain", PARITY_SHAPE, act=1) for k in
                     ("r2", "r3", "r4", "r5", "w128", "w128-w", "w128-wa", "w64", "w64-w", "w64-wa", "k2", "k2-w", "k2-wa", "e0", "e0-w", "e0-wa"))
# ... more tiles than CUs: one-pass against persistent, per epilogue form ...
PERSIST_PARITY = {form: tuple(Case(f"{k}{i}{il}", form, (TALL, 264, 160), act=1) for k, il in (("e", ""), ("p", ""), ("p", "-w"), ("p", "-wa")))
                  for i, form in enumerate(("plain", "ln_fold", "h2_residual"))}
# ... and 192-row tiles against 256-row tiles
T192_PARITY = tuple(Case(k, "h2_residual", T192_SHAPES[0]) for k in ("t192", "t192-w", "t192-wa", "e2"))
EXTRA_CASES = PARITY_CASES + tuple(c for cs in PERSIST_PARITY.values() for c in cs) + T192_PARITY


def of(form: str = None, il: bool = False, tail: bool = None):
    return [c for c in CASES if (form is None or c.form == form) and bool(c.k.il) == il and (tail is None or c.tail == tail)]


def planar_twin(case: Case) -> Case:
    """the same launch on planar operands and outputs: the kernel an image twin is compared with"""
    return dataclasses.replace(case, kernel=case.k.base, out_il=False)


def launch(case: Case, hip, device, guard=8, workspace=None, cus=256):
    """gemm_split1_cases.launch of the (resolved) case with split = 3, its images and `guard` rows behind every output"""
    c = case.resolve(cus)
    L = S1.launch(c, hip, device, split=3, guard=guard, w_il=c.k.il != "", a_il=c.k.il == "wa", out_il=c.out_il,
                  workspace=workspace if c.needs_ws else None)
    if c.outs == "h2":
        L.kw.pop("out_f32"), L.kw.pop("ldo")
        L.out_f32 = None
    elif c.outs == "f32":
        L.kw.pop("out_h2"), L.kw.pop("ldoh", None)
        L.out_h2 = L.out_img = None
    L.case = c
    return L


def expected_plan(case: Case, M: int, N: int) -> dict:
    """what the planner must answer for the case"""
    k = case.k
    t5 = -(-M // 256) * -(-N // 256)
    return dict(kernel=k.name, sk_parts=case.parts if k.kind == "sk" else 1, tail_split=case.parts if case.tail else 1,
                tail_rem=t5 % 256 if case.tail else 0, uses_workspace=int(case.needs_ws))
