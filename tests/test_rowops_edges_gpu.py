"""The row kernels of csrc/rowops.hip at the shapes, strides and aliasings where they can go wrong, against tests/rowops_oracle.py.

Three kinds of assertion:
  1. bit equality wherever the operation is a copy or at most one f32 rounding per element (against the same expression in torch
     float32 on the CPU, or against hip.H2.pack of the gathered values);
  2. h2 planes == hip.H2.pack of the f32 output of the same launch, bit for bit, for every kernel that emits both -- this pins
     split_h2 (csrc/common.h) without naming a tolerance;
  3. rowerr against fp64: the tolerance tests/test_ops_gpu.py uses for the kernel, applied per row of the kernel's own kind (a
     LayerNorm row, an image plane, a (b, q) row, a prompt plane, an image's logits), not per tensor.
Every output starts as NaN (-7 for integers) between two guard bands of a sentinel; a test asserts that every element was written
and that the bands are intact.  Every launch here has valid arguments on buffers of the stated size.

The grid-stride kernels cap their grids (grid_for in csrc/rowops.hip: 8192 blocks of 256, 16384 for im2col, 1024 for the mask
head).  The `second trip` cases are just above cap x 256 elements with a ragged tail and assert that they are: a later change of a
cap fails the case rather than silently un-testing the loop."""
import math

import pytest
import torch

import rowops_oracle as O

pytestmark = pytest.mark.gpu

# grid_for(n, block = 256, cap) in csrc/rowops.hip: elements one trip of the grid-stride loop covers
TRIP = 8192 * 256                  # add_rows, split, patchify, bilinear, dense_pe, assemble / overwrite / gather
TRIP_IM2COL = 16384 * 256
TRIP_MASK_HEAD = 1024 * 256

NAN = float("nan")
BAND = {torch.float32: -12345.0, torch.float16: -1234.0, torch.int64: -99}
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    return h


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


class Out:
    """A device buffer of `shape` (with `planes` leading planes: 2 for an h2 pair) between two guard bands of GUARD_ROWS rows.  The
    inside starts as NaN (-7 for integers), or as `init` for a buffer that is read and written in place."""

    def __init__(self, *shape, dtype=torch.float32, planes=0, init=None):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.g = min(-(-GUARD_ROWS * shape[-1] // 8) * 8, 8192)       # whole 16-byte vectors of either type; a flat buffer is one long row
        lead = (planes,) if planes else ()
        buf = torch.full(lead + (2 * self.g + self.n,), BAND[dtype], dtype=dtype)
        buf[..., self.g:self.g + self.n] = (-7 if dtype == torch.int64 else NAN) if init is None else init.reshape(lead + (self.n,))
        self.buf = buf.cuda()
        self.t = self.buf[..., self.g:self.g + self.n].view(lead + self.shape)

    def h2(self, hip):
        return hip.H2(self.t)

    def ptr(self, plane=None):
        return (self.t if plane is None else self.t[plane]).data_ptr()

    def read(self):
        """The inside, on the CPU, after checking that the bands are intact and that nothing inside was left unwritten."""
        torch.cuda.synchronize()
        b = self.buf.cpu()
        band = BAND[b.dtype]
        assert bool((b[..., :self.g] == band).all()) and bool((b[..., self.g + self.n:] == band).all()), "a guard band was written"
        inside = b[..., self.g:self.g + self.n]
        if b.dtype == torch.int64:
            assert bool((inside != -7).all()), "an element was not written"
        else:
            assert not bool(torch.isnan(inside).any()), "an element was not written"
        return inside.reshape(b.shape[:-1] + self.shape).clone()


def pack(hip, x):
    """hip.H2.pack as a (2, ...) fp16 tensor."""
    return hip.H2.pack(x).t


def assert_h2_is_pack_of(hip, planes, f32):
    assert O.same_bits(planes, pack(hip, f32)), "h2 planes differ from H2.pack of the f32 output of the same launch"


# the worst measured figures, printed by -s: each test reports what it measured before it asserts
def report(what, err, tol):
    print(f"[rowops] {what}: {err:.3e} (tolerance {tol:.1e})")


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
# M, D, add_rows (None: no add; "M": one per row), act, outputs, x a column block of a wider matrix, eps, sum_out
LN_CASES = [
    (1, 4, 1, 1, "both", False, 1e-6, True),
    (3, 8, 7, 2, "both", False, 1e-5, True),
    (5, 252, "M", 3, "both", True, 1e-6, True),
    (37, 256, 7, 1, "both", False, 1e-6, False),
    (5, 260, 1, 2, "both", True, 1e-5, True),
    (37, 1280, "M", 1, "both", False, 1e-6, True),
    (3, 2044, 7, 3, "both", True, 1e-6, False),
    (5, 2048, "M", 1, "both", False, 1e-5, True),
    (37, 1280, None, 0, "f32", False, 1e-6, False),
    (37, 2048, None, 0, "h2", True, 1e-6, False),
    (37, 260, None, 0, "hi", False, 1e-5, False),
    (37, 2044, None, 2, "f32", False, 1e-6, True),
    (37, 4, None, 0, "both", True, 1e-5, False),
    (37, 8, None, 3, "h2", False, 1e-6, False),
    (37, 252, None, 1, "both", False, 1e-6, False),
    (37, 256, None, 0, "hi", True, 1e-6, True),
]


def ln_inputs(M, D, add_rows, strided, case):
    x = O.layernorm_rows(M, D, seed=100 + case, shift=case)
    add = None if add_rows is None else rnd(M if add_rows == "M" else add_rows, D, seed=200 + case, scale=0.5)
    gamma, beta = 1.0 + 0.3 * rnd(D, seed=300 + case), rnd(D, seed=400 + case)
    if not strided:
        return x, add, gamma, beta, D, None
    wide = torch.full((M, D + 12), 7e7)                               # columns 4 .. 4 + D of a wider matrix; 7e7: what a wrong pitch reads
    wide[:, 4:4 + D] = x
    return x, add, gamma, beta, D + 12, wide.cuda()


def ln_launch(hip, xdev_ptr, ldx, add, gamma, beta, eps, act, M, D, sum_out, out_f32, out_hi, out_lo):
    hip._call("cvlm_layernorm", xdev_ptr, ldx, hip._p(add), 0 if add is None else add.shape[0], sum_out, gamma.data_ptr(), beta.data_ptr(),
              eps, act, out_f32, out_hi, out_lo, M, D)


@pytest.mark.parametrize("case", range(len(LN_CASES)))
def test_layernorm(hip, case):
    M, D, add_rows, act, outs, strided, eps, want_sum = LN_CASES[case]
    x, add, gamma, beta, ldx, wide = ln_inputs(M, D, add_rows, strided, case)
    xptr = wide.data_ptr() + 16 if strided else None
    xd = None if strided else x.cuda()
    addd, gd, bd = (None if add is None else add.cuda()), gamma.cuda(), beta.cuda()
    of = Out(M, D) if outs in ("f32", "both") else None
    oh = Out(M, D, dtype=torch.float16, planes=1 if outs == "hi" else 2) if outs != "f32" else None
    so = Out(M, D) if want_sum else None
    ln_launch(hip, xptr if strided else xd.data_ptr(), ldx, addd, gd, bd, eps, act, M, D, so and so.ptr(), of and of.ptr(),
              oh and oh.ptr(0), oh.ptr(1) if oh is not None and outs != "hi" else None)
    s, ref, r = O.layernorm(x, gamma, beta, eps, add=add, act=act)
    tol = O.layernorm_tolerance(r)
    # measured on an MI355X: the worst ratio of a row's error to this bound over all the cases of this file is 0.23, f32 and h2 alike (an
    # offset-100 row at D = 256); rows without an offset stay below 2.5e-7 of the 3e-6
    if so is not None:
        want = x if add is None else x + add[torch.arange(M) % add.shape[0]]
        assert O.same_bits(so.read(), want)                           # one f32 add per element
    if of is not None:
        got = of.read()
        ratio = O.rowerrs(got, ref) / tol
        report(f"layernorm f32 M={M} D={D} act={act} (worst row {LN_FAMILY(case, int(ratio.argmax()))}) rowerr / bound", float(ratio.max()), 1.0)
        assert float(ratio.max()) < 1.0
        plain = O.rowerrs(got, ref)[r < 1.0]
        if plain.numel():
            report(f"layernorm f32 M={M} D={D} rows without an offset, rowerr", float(plain.max()), 3e-6)
    if oh is not None:
        planes = oh.read()
        if of is not None:
            assert_h2_is_pack_of(hip, planes, got)
        val = planes.float().sum(0)
        if outs == "hi":                                              # out_lo = NULL: the hi plane of the two-plane launch, and fp16 of the row
            both = Out(M, D, dtype=torch.float16, planes=2)
            ln_launch(hip, xptr if strided else xd.data_ptr(), ldx, addd, gd, bd, eps, act, M, D, None, None, both.ptr(0), both.ptr(1))
            assert O.same_bits(planes[0], both.read()[0])
            assert float((O.rowerrs(val, ref) / (tol + 2.0 ** -11)).max()) < 1.0
        else:
            ratio = O.rowerrs(val, ref) / tol
            report(f"layernorm h2 M={M} D={D} act={act} rowerr / bound", float(ratio.max()), 1.0)
            assert float(ratio.max()) < 1.0


def LN_FAMILY(case, row):
    return O.LN_FAMILIES[(row + case) % len(O.LN_FAMILIES)]


@pytest.mark.parametrize("D", [4, 260, 1280, 2048])
def test_layernorm_in_place(hip, D):
    """The engine's layernorm(x, ..., out_f32=x), also with add=, and sum_out=x: the bits of the out-of-place launch (include/cvlm.h
    states the aliasing contract)."""
    M, case = 37, 50
    x, add, gamma, beta, _, _ = ln_inputs(M, D, 7, False, case)
    xd, addd, gd, bd = x.cuda(), add.cuda(), gamma.cuda(), beta.cuda()
    for use_add in (None, addd):
        of, so = Out(M, D), Out(M, D)
        ln_launch(hip, xd.data_ptr(), D, use_add, gd, bd, 1e-6, 1, M, D, so.ptr(), of.ptr(), None, None)
        want_out, want_sum = of.read(), so.read()
        a = Out(M, D, init=x)                                         # out_f32 = x
        ln_launch(hip, a.ptr(), D, use_add, gd, bd, 1e-6, 1, M, D, None, a.ptr(), None, None)
        assert O.same_bits(a.read(), want_out)
        b, ob = Out(M, D, init=x), Out(M, D)                          # sum_out = x
        ln_launch(hip, b.ptr(), D, use_add, gd, bd, 1e-6, 1, M, D, b.ptr(), ob.ptr(), None, None)
        assert O.same_bits(b.read(), want_sum) and O.same_bits(ob.read(), want_out)
        c, oc = Out(M, D, init=x), Out(M, D, dtype=torch.float16, planes=2)      # out_f32 = x with the h2 planes beside it
        ln_launch(hip, c.ptr(), D, use_add, gd, bd, 1e-6, 1, M, D, None, c.ptr(), oc.ptr(0), oc.ptr(1))
        assert O.same_bits(c.read(), want_out)
        assert_h2_is_pack_of(hip, oc.read(), want_out)


# ---- add_rows / split ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,b_rows,scale", [(10, 4, 1, 2.0), (10, 64, 5, 0.3), (10, 4, 7, 0.3), (10, 64, 7, 2.0), (10, 64, 10, 0.3),
                                              (10, 4, None, 0.25), (10, 64, None, 0.25), (8161, 1028, 7, 0.3)])
def test_add_rows(hip, M, D, b_rows, scale):
    if M > 10:
        assert M * D // 4 > TRIP and (M * D // 4) % 256 != 0          # second trip of the grid-stride loop, ragged tail
    a = rnd(M, D, seed=1)
    b = None if b_rows is None else rnd(b_rows, D, seed=2)
    want = O.add_rows_f32(a, b, scale)
    ad, bd = a.cuda(), None if b is None else b.cuda()
    of, oh = Out(M, D), Out(M, D, dtype=torch.float16, planes=2)
    hip.add_rows(ad, bd, b_rows or 0, M, D, scale=scale, out_f32=of.t, out_h2=oh.h2(hip))
    got = of.read()
    assert O.same_bits(got, want)                                     # (a + b) * scale: two f32 roundings, no fusing possible
    assert_h2_is_pack_of(hip, oh.read(), got)
    o2 = Out(M, D, dtype=torch.float16, planes=2)                     # h2 only
    hip.add_rows(ad, bd, b_rows or 0, M, D, scale=scale, out_h2=o2.h2(hip))
    assert_h2_is_pack_of(hip, o2.read(), want)
    ip = Out(M, D, init=a)                                            # in place: out_f32 = a (x + pos_embed on the stream)
    hip.add_rows(ip.t, bd, b_rows or 0, M, D, scale=scale, out_f32=ip.t)
    assert O.same_bits(ip.read(), want)


@pytest.mark.parametrize("n", [4, 1028, 8192 * 1024 + 1028])
def test_split_f32(hip, n):
    if n > 1028:
        assert n // 4 > TRIP and n % 1024 != 0
    adv = O.split_adversaries()
    v = rnd(n, seed=3) * torch.pow(10.0, rnd(n, seed=4).clamp(-3, 1))  # magnitudes over several fp16 exponents
    v = v.clamp(-65504.0, 65504.0)
    v[v.abs() < 2.0 ** -25] = 0.0
    if n >= adv.numel():
        v[:adv.numel()] = adv
        v[n - adv.numel():] = adv.flip(0)                             # and in the ragged tail of the last trip
    else:
        v[:] = torch.tensor([1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -10 + 2.0 ** -11), -0.0, 2.0 ** -14 - 2.0 ** -38])
    out = Out(n, dtype=torch.float16, planes=2)
    hip.split_f32(v.cuda(), out.h2(hip))
    planes = out.read()
    assert O.same_bits(planes, pack(hip, v))
    # hi + lo gives v back to 2^-22 |v| -- or to 2^-25 where lo is an fp16 subnormal (spacing 2^-24), that is for |v| below 2^-3
    back = planes[0].double() + planes[1].double()
    assert bool(((back - v.double()).abs() <= torch.maximum(2.0 ** -22 * v.double().abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    big = v.abs() >= 2.0 ** -3
    assert bool(((back - v.double()).abs()[big] <= 2.0 ** -22 * v.double().abs()[big]).all())
    hi_only = Out(n, dtype=torch.float16, planes=1)                   # out_lo = NULL
    vd = v.cuda()
    hip._call("cvlm_split_f32", vd.data_ptr(), hi_only.ptr(0), None, n)
    assert O.same_bits(hi_only.read()[0], v.half())


# ---- gathers into h2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C0,C1,H,W,p,ldk", [(1, 3, 0, 28, 42, 14, 608), (3, 3, 0, 42, 28, 14, 608), (3, 3, 1, 42, 28, 14, 800),
                                               (1, 3, 1, 14, 28, 14, 832), (4600, 3, 0, 28, 42, 14, 608)])
def test_patchify(hip, B, C0, C1, H, W, p, ldk):
    rows, K = B * (H // p) * (W // p), (C0 + C1) * p * p
    if B > 3:
        assert rows * ldk // 8 > TRIP and (rows * ldk // 8) % 256 != 0
    s0, s1 = rnd(B, C0, H, W, seed=5), (rnd(B, C1, H, W, seed=6) if C1 else None)
    out = Out(rows, ldk, dtype=torch.float16, planes=2)
    hip.patchify(s0.cuda(), None if s1 is None else s1.cuda(), p, out.h2(hip), ldk)
    planes = out.read()
    assert O.same_bits(planes, pack(hip, O.patchify(s0, s1, p, ldk)))
    assert int(O.bits(planes[:, :, K:]).abs().max() if ldk > K else 0) == 0            # the pad columns are +0 in both planes


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 1, 5, 8), (1, 5, 1, 16), (3, 9, 7, 64), (2, 170, 172, 64)])
def test_im2col3x3(hip, B, H, W, C):
    if H > 9:
        assert B * H * W * 9 * C // 8 > TRIP_IM2COL and (B * H * W * 9 * C // 8) % 256 != 0
    x = rnd(B, H, W, C, seed=7)
    out = Out(B * H * W, 9 * C, dtype=torch.float16, planes=2)
    hip.im2col3x3(x.cuda(), B, H, W, C, out.h2(hip))
    assert O.same_bits(out.read(), pack(hip, O.im2col3x3(x)))


@pytest.mark.parametrize("B,T,D,scale,lo", [(1, 1, 1, 1.0, True), (2, 33, 31, 0.25, True), (2, 33, 31, 1.0, False), (3, 100, 48, 0.25, True),
                                            (3, 100, 48, 1.0, True), (1, 1, 1, 0.25, True)])
def test_reinterpret_transpose(hip, B, T, D, scale, lo):
    x = rnd(B, T, D, seed=8)
    out = Out(B * T, D, dtype=torch.float16, planes=2 if lo else 1)
    hip._call("cvlm_reinterpret_transpose", x.cuda().data_ptr(), B, T, D, scale, out.ptr(0), out.ptr(1) if lo else None)
    want = pack(hip, O.reinterpret_transpose(x, B, T, D, scale))
    assert O.same_bits(out.read(), want if lo else want[:1])


# ---- decoder side ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 6, 256])
@pytest.mark.parametrize("size", [1, 7, 20])
def test_dense_pe(hip, size, C):
    gm = rnd(2, C // 2, seed=9)
    out = Out(size * size, C)
    hip.dense_pe(gm.cuda(), size, C, out.t)
    err = float((out.read().double() - O.dense_pe(gm, size)).abs().max())
    report(f"dense_pe size={size} C={C} abs", err, 2e-5)
    assert err < 2e-5


@pytest.mark.parametrize("with_edge", [True, False])
@pytest.mark.parametrize("B,HW,C", [(1, 1, 4), (3, 300, 32), (3, 1025, 36), (1, 300, 36), (3, 1, 32), (1, 1025, 4), (1, 1024 * 256 + 37, 4)])
def test_mask_head(hip, B, HW, C, with_edge):
    if HW > 1025:
        assert HW > TRIP_MASK_HEAD and HW % 256 != 0
    u, e, h = rnd(B, HW, C, seed=10), (rnd(B, HW, C, seed=11) if with_edge else None), rnd(B, 5, C, seed=12)
    low = Out(B, HW)
    hip.mask_head(u.cuda(), None if e is None else e.cuda(), h.cuda(), B, HW, C, low.t)
    err = O.rowerr(low.read(), O.mask_head(u, e, h))                  # a row = a prompt's plane
    report(f"mask_head B={B} HW={HW} C={C} edge={with_edge} rowerr", err, 3e-6)
    assert err < 3e-6


BILINEAR_SHAPES = [(37, 53, 101, 67), (64, 48, 21, 29), (1, 9, 5, 30), (9, 1, 30, 5), (96, 64, 37, 1), (336, 224, 100, 75), (5, 7, 5, 7),
                   (7, 5, 1, 1), (40, 24, 1024, 768)]


@pytest.mark.parametrize("sigmoid_in", [False, True])
@pytest.mark.parametrize("hin,win,hout,wout", BILINEAR_SHAPES)
def test_bilinear(hip, hin, win, hout, wout, sigmoid_in):
    N = 3
    if hout == 1024:
        assert N * hout * wout > TRIP and N * hout * wout % TRIP != 0   # a second, partial trip of the grid
    x = rnd(N, hin, win, seed=13) * 2.0
    out = Out(N, hout, wout)
    hip.bilinear(x.cuda(), N, hin, win, out.t, hout, wout, sigmoid_in=sigmoid_in)
    got = out.read()
    err = O.rowerr(got, O.bilinear(x, hout, wout, sigmoid_in=sigmoid_in), row_dims=2)       # a row = an image plane
    report(f"bilinear {hin}x{win} -> {hout}x{wout} sigmoid={sigmoid_in} rowerr", err, 1e-6)
    assert err < 1e-6
    if (hin, win) == (hout, wout) and not sigmoid_in:
        assert O.same_bits(got, x)                                    # an identity: weights 1 and 0


# ---- CLIP side ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nctx", [0, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W", [4, 64])
def test_assemble_overwrite_gather(hip, W, B, nctx):
    P = 5
    L = 1 + P + nctx
    pt, cls, pos, ctx = rnd(B, P, W, seed=14), rnd(W, seed=15), rnd(1 + P, W, seed=16), rnd(max(nctx, 1), W, seed=17)
    tok = Out(B, L, W)
    hip.clip_assemble(pt.cuda(), cls.cuda(), pos.cuda(), ctx.cuda(), B, P, W, nctx, tok.t)
    ref = O.clip_assemble(pt, cls, pos, ctx, nctx)
    assert O.same_bits(tok.read(), ref)
    # overwrite: the whole sequence, then its last row only; every row outside the range keeps its bits
    for first, n in ((L - 1, 1), (0, L)):
        src = rnd(n, W, seed=18 + n)
        hip.overwrite_rows(tok.t, B, L, W, first, n, src.cuda())
        ref[:, first:first + n] = src
        assert O.same_bits(tok.read(), ref)
    # gather: idx with a repeat, the first and the last row; idx = NULL with the first / last row fixed
    idx = torch.tensor(([0, L - 1, L - 1] if B == 3 else [L - 1]), dtype=torch.int32)
    for ix, fixed in ((idx, 0), (None, 0), (None, L - 1)):
        g = Out(B, W)
        hip.gather_rows(tok.t, B, L, W, None if ix is None else ix.cuda(), fixed, g.t)
        rows = ix.long() if ix is not None else torch.full((B,), fixed)
        assert O.same_bits(g.read(), ref[torch.arange(B), rows])
    # the same pick from an h2 stream, scaled
    planes = pack(hip, ref * 3.7)
    xh = hip.H2(planes.cuda())
    for scale in (0.25, 3.0):
        for ix, fixed in ((idx, 0), (None, 0), (None, L - 1)):
            g = Out(B, W)
            hip.gather_rows_h2(xh, scale, B, L, W, None if ix is None else ix.cuda(), fixed, g.t)
            rows = ix.long() if ix is not None else torch.full((B,), fixed)
            want = (planes[0].float() + planes[1].float())[torch.arange(B), rows] * torch.tensor(scale)   # the sum is exact in f32
            assert O.same_bits(g.read(), want)


@pytest.mark.parametrize("W", [4, 64])
def test_gather_from_sequences_of_one_row(hip, W):
    B, L = 3, 1
    x = rnd(B, L, W, seed=19)
    for ix in (torch.zeros(B, dtype=torch.int32).cuda(), None):
        g, g2 = Out(B, W), Out(B, W)
        hip.gather_rows(x.cuda(), B, L, W, ix, 0, g.t)
        assert O.same_bits(g.read(), x[:, 0])
        hip.gather_rows_h2(hip.H2(pack(hip, x).cuda()), 3.0, B, L, W, ix, 0, g2.t)
        assert O.same_bits(g2.read(), (pack(hip, x)[0].float() + pack(hip, x)[1].float())[:, 0] * 3.0)


def clip_head_run(hip, img, txt, B, C, D):
    img_n, logits, pred, sel = Out(B, D), Out(B, C), Out(B, dtype=torch.int64), Out(B, D)
    hip.clip_head(img.cuda(), txt.cuda(), 100.0, B, C, D, img_n.t, logits.t, pred.t, sel.t)
    return img_n.read(), logits.read(), pred.read(), sel.read()


@pytest.mark.parametrize("B,C,D", [(1, 1, 100), (3, 15, 768), (3, 16, 1024), (1, 17, 1088), (3, 61, 1088), (3, 1024, 100), (1, 1024, 1088),
                                   (3, 61, 768), (3, 17, 1024)])
def test_clip_head(hip, B, C, D):
    """D = 1088 takes the loop path (D > 1024: the row no longer fits the lane's registers)."""
    img, txt = rnd(B, D, seed=20) * 3.0, rnd(C, D, seed=21)
    img_n, logits, pred, sel = clip_head_run(hip, img, txt, B, C, D)
    n_ref, l_ref = O.clip_head(img, txt, 100.0)
    e_n, e_l = O.rowerr(img_n, n_ref), O.rowerr(logits, l_ref)        # a row = an image
    report(f"clip_head B={B} C={C} D={D} img_n rowerr", e_n, 1e-6)
    report(f"clip_head B={B} C={C} D={D} logits rowerr", e_l, 3e-6)
    assert e_n < 1e-6 and e_l < 3e-6
    if C > 1:                                                         # the seeds leave no row undecided: nothing is skipped
        top2 = l_ref.topk(2, dim=1).values
        assert bool(((top2[:, 0] - top2[:, 1]) > 1e-4 * top2[:, 0].abs()).all())
    assert pred.tolist() == l_ref.argmax(1).tolist()
    assert O.same_bits(sel, txt[l_ref.argmax(1)])


@pytest.mark.parametrize("D", [768, 1088])
def test_clip_head_tie_goes_to_the_lower_index(hip, D):
    """Two bit-identical text rows hold the maximum: pred is the lower index (the strict-`>` scan of include/cvlm.h)."""
    C = 61
    img, txt = rnd(1, D, seed=22), rnd(C, D, seed=23)
    txt[5] = img[0] * 2.0                                             # aligned with the image: far above every random row
    txt[40] = txt[5]
    _, logits, pred, sel = clip_head_run(hip, img, txt, 1, C, D)
    assert O.same_bits(logits[0, 5], logits[0, 40]) and float(logits[0, 5]) == float(logits.max())
    assert pred.tolist() == [5] and O.same_bits(sel[0], txt[5])


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("D", [1, 4, 100, 768])
def test_normalize_add(hip, D, R, with_add):
    x, ad = rnd(R, D, seed=24) * 5.0, (rnd(R, D, seed=25) if with_add else None)
    out = Out(R, D)
    hip.normalize_add(x.cuda(), None if ad is None else ad.cuda(), R, D, out.t)
    err = O.rowerr(out.read(), O.normalize_add(x, ad))
    report(f"normalize_add R={R} D={D} add={with_add} rowerr", err, 1e-6)
    assert err < 1e-6


# ---- the decoder's small attention ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("nk", [1, 63, 64, 65, 255, 256, 257, 1024, 1025])
def test_small_attention(hip, nk, hd, nq):
    """nk <= 64: one thread per (b, q, head); above: a workgroup per (b, q, head), whose waves (255 / 256 / 257 keys) and lanes may
    hold no key at all, and whose threads take a second batch of four keys from 1025 on.  q, k and v are column blocks of wider
    matrices (row pitch 3 D), the f32 and h2 outputs come from one launch."""
    B, heads = 2, 3
    D = heads * hd
    q, k, v = rnd(B, nq, D, seed=26), rnd(B, nk, D, seed=27), rnd(B, nk, D, seed=28)
    wq = torch.full((B * nq, 3 * D), 7e7)
    wkv = torch.full((B * nk, 3 * D), 7e7)
    wq[:, :D] = q.reshape(B * nq, D)
    wkv[:, D:2 * D], wkv[:, 2 * D:] = k.reshape(B * nk, D), v.reshape(B * nk, D)
    wq, wkv = wq.cuda(), wkv.cuda()
    of, oh = Out(B * nq, D), Out(B * nq, D, dtype=torch.float16, planes=2)
    hip.small_attention(wq[:, :D], wkv[:, D:2 * D], wkv[:, 2 * D:], of.t, B, nq, nk, heads, hd, out_h2=oh.h2(hip))
    got, planes = of.read(), oh.read()
    assert_h2_is_pack_of(hip, planes, got)
    ref = O.small_attention(q, k, v, heads, hd).reshape(B * nq, D)
    err = O.rowerr(got, ref)                                          # a row = one (b, q)
    report(f"small_attention nk={nk} hd={hd} nq={nq} rowerr", err, 3e-6)
    assert err < 3e-6
    o2 = Out(B * nq, D, dtype=torch.float16, planes=2)                # h2 only
    hip.small_attention(wq[:, :D], wkv[:, D:2 * D], wkv[:, 2 * D:], None, B, nq, nk, heads, hd, out_h2=o2.h2(hip))
    assert O.same_bits(o2.read(), planes)
