"""Per-operator parity of the HIP kernels (through the C ABI) against fp64 torch-CPU restatements.

Tolerances: split=3 (hi*hi + lo*hi + hi*lo) is the parity mode and is held to ~fp32 accuracy;
split=1 (fp16 operands) is the fast mode and is held to fp16-operand accuracy.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    return h


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def dev_h2(hip, x):
    return hip.H2(hip.H2.pack(x).t.cuda())


def relerr(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 200, 96), (70, 36, 64), (1000, 384, 1280)])
@pytest.mark.parametrize("split", [3, 1])
def test_gemm_plain(hip, M, N, K, split):
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    out = torch.full((M, N), float("nan"), device="cuda")
    hip.gemm(A, W, M, N, K, out_f32=out, split=split)
    if split == 3:
        ref = A.float().cpu().double() @ W.float().cpu().double().t()
        assert relerr(out, ref) < 2e-6
    else:
        ref = A.hi.float().cpu().double() @ W.hi.float().cpu().double().t()
        assert relerr(out, ref) < 2e-6          # same fp16 operands, fp32 accumulate
    ref32 = a.double() @ w.double().t()
    assert relerr(out, ref32) < (1e-5 if split == 3 else 3e-3)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_epilogue(hip, act):
    M, N, K = 200, 136, 64
    a, w, bias, res = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.1), rnd(N, seed=5), rnd(M, N, seed=6)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    out = torch.empty(M, N, device="cuda")
    oh = hip.H2.empty(M, N)
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), residual=res.cuda(), out_f32=out, out_h2=oh, act=act, alpha=0.5)
    z = 0.5 * (A.float().cpu().double() @ W.float().cpu().double().t()) + bias.double()
    z = {0: z, 1: F.gelu(z), 2: z * torch.sigmoid(1.702 * z), 3: F.relu(z)}[act] + res.double()
    assert relerr(out, z) < 3e-6
    assert relerr(oh.float(), z) < 3e-6


def test_gemm_abs_post_and_batch(hip):
    Bz, M, N, K = 3, 96, 80, 64
    a, w, res = rnd(M, K, seed=7), rnd(Bz, N, K, seed=8), rnd(Bz, M, N, seed=9)
    A, W = dev_h2(hip, a), dev_h2(hip, w.reshape(Bz * N, K))
    out = torch.empty(Bz, M, N, device="cuda")
    hip.gemm(A, W, M, N, K, residual=res.cuda(), out_f32=out, act=hip.ACT_ABS_POST, alpha=-1.0, batch=Bz,
             stride_a=0, stride_w=N * K, stride_r=M * N, stride_o=M * N)
    Wf = W.float().cpu().double().reshape(Bz, N, K)
    ref = (res.double() - torch.einsum("mk,bnk->bmn", A.float().cpu().double(), Wf)).abs()
    assert relerr(out, ref) < 3e-6


def test_gemm_pixel_shuffle(hip):
    Bn, H, Wd, Cin, Cout = 2, 6, 5, 64, 16
    x = rnd(Bn, Cin, H, Wd, seed=10)
    wt = rnd(Cin, Cout, 2, 2, seed=11, scale=0.1)
    bias = rnd(Cout, seed=12)
    ref = F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2).permute(0, 2, 3, 1)  # NHWC
    a = x.permute(0, 2, 3, 1).reshape(Bn * H * Wd, Cin)
    wg = wt.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)          # rows (dy, dx, co)
    A, W = dev_h2(hip, a), dev_h2(hip, wg)
    out = torch.full((Bn, 2 * H, 2 * Wd, Cout), float("nan"), device="cuda")
    hip.gemm(A, W, Bn * H * Wd, 4 * Cout, Cin, bias=bias.repeat(4).cuda(), out_f32=out,
             pixel_shuffle=(H, Wd, 2 * Cout))
    assert relerr(out, ref) < 1e-5


@pytest.mark.parametrize("M,N,K,why", [
    (512, 512, 8192, "4 tiles, long K -> 4 chained K-parts each"),
    (700, 1000, 1024, "ragged 3 x 4 tiles -> 2 parts, clamped rows / columns"),
    (4648, 1024, 4096, "CLIP c_proj: 76 tiles -> 3 parts"),
    (256 * 33, 256 * 8, 256, "264 tiles, short K: the cost model leaves the 8 tail tiles whole"),
    (39200, 1280, 1280, "770 tiles = 3 rounds + 2 tail tiles in 2 parts, chip fully loaded"),
])
def test_gemm_tail_split(hip, M, N, K, why, monkeypatch):
    """256^2 kernel with its last partial round cut along K: partial slabs handed between workgroups
    (possibly across XCDs) must be complete and fresh, whichever order the partners finish in."""
    monkeypatch.setenv("CVLM_GEMM_VARIANT", "7")
    monkeypatch.setenv("CVLM_GEMM_TAIL", "1")
    ws = hip.new_gemm_workspace("cuda")                                                # caller-owned slabs + hand-off words
    a, w, bias = rnd(M, K, seed=61), rnd(N, K, seed=62, scale=0.05), rnd(N, seed=63)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    ref = A.float().double() @ W.float().double().t() + bias.cuda().double()            # on the GPU: 39200-row case
    outs = []
    for rep in range(3):                                                               # slabs and hand-off words are reused
        out = torch.full((M, N), float("nan"), device="cuda")
        oh = hip.H2.empty(M, N)
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_f32=out, out_h2=oh, workspace=ws)
        outs.append(out)
        assert float((out.double() - ref).abs().max() / ref.abs().max()) < 2e-6, why
        assert float((oh.float().double() - ref).abs().max() / ref.abs().max()) < 2e-6, why
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])             # fixed summation order
    plain = torch.empty(M, N, device="cuda")
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_f32=plain)                           # no workspace: every tile whole
    assert float((plain - outs[0]).abs().max() / ref.abs().max()) < 4e-6               # same values up to fp32 sum order
    assert hip.gemm_workspace_errors(ws) == 0                                          # no abandoned hand-off
    assert int(ws[:2048].view(torch.int32).abs().sum()) == 0                           # hand-off words are back to zero


@pytest.mark.parametrize("M,N,K", [(4096, 5120, 1280), (4000, 4360, 256), (3840, 4608, 64)])
def test_gemm_column_split_one_image(hip, monkeypatch, M, N, K):
    """One image's lin1 (4096 x 5120: 320 tiles of 256^2 on 256 CUs) goes out as two launches -- the columns that make one round of
    256^2 tiles, the rest as 128^2 tiles (CVLM_GEMM_COLSPLIT).  Whole tiles in both: same bits as the single launch, for the plain
    and the LayerNorm-folded epilogue, ragged M / N included."""
    from camouflaged_vlm_amd.engine import LnLinear
    a, w, bias = rnd(M, K, seed=51), rnd(N, K, seed=52, scale=K ** -0.5), rnd(N, seed=53)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double()
    ws = hip.new_gemm_workspace("cuda")
    XS = 0.25
    x = rnd(M, K, seed=55) * 2.0
    gamma, beta = 1.0 + 0.1 * rnd(K, seed=56), 0.05 * rnd(K, seed=57)
    xh, st, mrg = hip.H2.empty(M, K), torch.empty(hip.stats_pieces(K), M, 2, device="cuda"), torch.empty(M, 2, device="cuda")
    hip.row_stats_split(x.cuda(), XS, xh, st, M, K)
    hip.ln_stats_merge(st, M, K, 1e-6, mrg, ws)
    lin = LnLinear(w, bias, gamma, beta, "cuda")
    got = {}
    for cs in ("0", "1"):
        monkeypatch.setenv("CVLM_GEMM_COLSPLIT", cs)
        o = torch.full((M, N), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_f32=o, workspace=ws)
        oh = hip.H2.empty(M, N + 64)                                  # a leading dimension wider than N, as lin1's output has
        oh.t.fill_(float("nan"))
        hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=1, out_h2=oh, ldoh=N + 64, ln_fold=(mrg, lin.colsum),
                 workspace=ws)
        torch.cuda.synchronize()
        assert relerr(o.cpu().double(), ref) < 3e-6, cs
        got[cs] = (o, oh.t.clone())
    assert torch.equal(got["0"][0], got["1"][0])
    assert torch.equal(got["0"][1][:, :, :N], got["1"][1][:, :, :N])
    assert bool(torch.isnan(got["1"][1][:, :, N:]).all())                # nothing written beyond column N
    z = F.gelu(F.layer_norm(xh.float().cpu().double()[:, :K] / XS, (K,), gamma.double(), beta.double(), 1e-6) @ w.double().t() + bias.double())
    got_fold = (got["1"][1][0].float() + got["1"][1][1].float())[:, :N].cpu().double()
    assert float((got_fold - z).abs().max()) < 2e-5 * max(1.0, float(z.abs().max()))
    assert hip.gemm_workspace_errors(ws) == 0


@pytest.mark.parametrize("M,N,K,variant,use_ws", [(16640, 1280, 256, "7", False),      # 325 tiles: persistent 256^2 kernel
                                                   (8192, 1280, 320, "7", True),        # 160 tiles: one-pass 256^2 kernel
                                                   (9296, 1024, 512, "0", True),        # 192-row tiles (h2-residual form), 256^2 otherwise
                                                   (8200, 1160, 256, "2", True),        # 256 x 128 tiles, ragged M / N
                                                   (4096, 5120, 256, "0", True),        # one image's lin1: column split + interleaved
                                                   (581, 1024, 1024, "0", True),        # small grid: 64 x 128 tiles on the deep ring
                                                   (581, 4096, 1024, "0", True),        # small grid: 128^2 tiles, eight waves
                                                   (581, 1024, 4096, "0", True)])       # small grid: split-K parts
def test_gemm_interleaved_weights_same_bits(hip, monkeypatch, M, N, K, variant, use_ws):
    """ABI 6: the big-tile kernels stage the weight from the image whose planes are interleaved per 32 k-elements (whole 128-byte
    lines).  Same fragments, same MFMA order: plain, LayerNorm-folded and h2-residual launches give the bits of the planar launch."""
    from camouflaged_vlm_amd.engine import LnLinear
    monkeypatch.setenv("CVLM_GEMM_VARIANT", variant)
    a, w, bias, res = rnd(M, K, seed=71), rnd(N, K, seed=72, scale=K ** -0.5), rnd(N, seed=73), rnd(M, N, seed=74)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    Wil = hip.interleave_planes(W)
    assert Wil.shape == (N, 2 * K) and torch.equal(Wil[5, 32:64], W.lo[5, 0:32]) and torch.equal(Wil[5, 64:96], W.hi[5, 32:64])
    ws = hip.new_gemm_workspace("cuda") if use_ws else None
    XS = 0.25
    x = rnd(M, K, seed=75) * 2.0
    gamma, beta = 1.0 + 0.1 * rnd(K, seed=76), 0.05 * rnd(K, seed=77)
    xh, st, mrg = hip.H2.empty(M, K), torch.empty(hip.stats_pieces(K), M, 2, device="cuda"), torch.empty(M, 2, device="cuda")
    hip.row_stats_split(x.cuda(), XS, xh, st, M, K)
    hip.ln_stats_merge(st, M, K, 1e-6, mrg, hip.new_gemm_workspace("cuda"))
    lin = LnLinear(w, bias, gamma, beta, "cuda")
    lin_il = hip.interleave_planes(lin.w)
    got = {}
    for tag, wil, lil in (("planar", None, None), ("interleaved", Wil, lin_il)):
        o = torch.full((M, N), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_f32=o, workspace=ws, w_il=wil)
        oh = hip.H2.empty(M, N)
        oh.t.fill_(float("nan"))
        hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=1, out_h2=oh, ln_fold=(mrg, lin.colsum), workspace=ws,
                 w_il=lil)
        o2 = hip.H2(hip.H2.pack(res * XS).t.cuda())
        st_out = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o2, residual_h2=(o2, 1.0 / XS), out_scale=XS, row_stats=st_out, workspace=ws,
                 w_il=wil)
        torch.cuda.synchronize()
        got[tag] = (o, oh.t.clone(), o2.t.clone(), st_out)
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double()
    assert relerr(got["interleaved"][0].cpu().double(), ref) < 3e-6
    for i in range(4):
        assert torch.equal(got["planar"][i], got["interleaved"][i]), i
    if ws is not None:
        assert hip.gemm_workspace_errors(ws) == 0


@pytest.mark.parametrize("M,N,K,variant,use_ws", [(16640, 1280, 256, "7", False),      # persistent 256^2 kernel
                                                   (8192, 1280, 320, "7", True),        # one-pass 256^2 kernel
                                                   (33000, 1280, 128, "0", True),       # 2.5+ rounds: tail parts behind the whole tiles
                                                   (8200, 1160, 256, "2", True),        # 256 x 128 tiles, ragged M / N
                                                   (4096, 3840, 256, "0", True),        # one image: one round of 256^2 tiles
                                                   (4096, 5120, 256, "0", True),        # one image's lin1: column split, image output
                                                   (4096, 1280, 1280, "0", True),       # one image: K-parts / tail chain
                                                   (581, 1024, 1024, "0", True),        # small grid: 64 x 128 tiles on the deep ring
                                                   (581, 4096, 1024, "0", True),        # small grid: 128^2 tiles, eight waves
                                                   (581, 1024, 4096, "0", True)])       # small grid: split-K parts
def test_gemm_interleaved_activations_same_bits(hip, monkeypatch, M, N, K, variant, use_ws):
    """ABI 6: activations that only GEMMs touch travel as 128-byte-row images (a_il / out_il / res_il).  Operand image in, output image
    out, residual image in place: the bits of the planar launches, for the plain, LayerNorm-folded and h2-residual epilogues."""
    from camouflaged_vlm_amd.engine import LnLinear
    monkeypatch.setenv("CVLM_GEMM_VARIANT", variant)
    a, w, bias, res = rnd(M, K, seed=81), rnd(N, K, seed=82, scale=K ** -0.5), rnd(N, seed=83), rnd(M, N, seed=84)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    Wil, Ail = hip.interleave_planes(W), hip.H2IL.from_planes(A)
    assert torch.equal(Ail.planes().t, A.t)
    ws = hip.new_gemm_workspace("cuda") if use_ws else None
    XS = 0.25
    x = rnd(M, K, seed=85) * 2.0
    gamma, beta = 1.0 + 0.1 * rnd(K, seed=86), 0.05 * rnd(K, seed=87)
    xh, st, mrg = hip.H2.empty(M, K), torch.empty(hip.stats_pieces(K), M, 2, device="cuda"), torch.empty(M, 2, device="cuda")
    hip.row_stats_split(x.cuda(), XS, xh, st, M, K)
    hip.ln_stats_merge(st, M, K, 1e-6, mrg, hip.new_gemm_workspace("cuda"))
    xil = hip.H2IL.from_planes(xh)
    lin = LnLinear(w, bias, gamma, beta, "cuda")
    lin_il = hip.interleave_planes(lin.w)
    NP = N + 64 - N % 32 if N % 32 else N + 64                                  # image width: a multiple of 32, wider than N
    # planar reference launches
    o = hip.H2.empty(M, N); oh = hip.H2.empty(M, N)
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o, workspace=ws, w_il=Wil)
    hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=1, out_h2=oh, ln_fold=(mrg, lin.colsum), workspace=ws, w_il=lin_il)
    o2 = hip.H2(hip.H2.pack(res * XS).t.cuda())
    st_ref = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device="cuda")
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o2, residual_h2=(o2, 1.0 / XS), out_scale=XS, row_stats=st_ref, workspace=ws, w_il=Wil)
    # the same through images
    oi = hip.H2IL(torch.full((M, 2 * NP), float("nan"), dtype=torch.float16, device="cuda"))
    hip.gemm(Ail, W, M, N, K, bias=bias.cuda(), out_h2=oi, workspace=ws, w_il=Wil)
    ohi = hip.H2IL(torch.full((M, 2 * NP), float("nan"), dtype=torch.float16, device="cuda"))
    hip.gemm(xil, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=1, out_h2=ohi, ln_fold=(mrg, lin.colsum), workspace=ws, w_il=lin_il)
    r_pl = hip.H2.zeros(M, NP)
    r_pl.t[:, :, :N] = hip.H2.pack(res * XS).t.cuda()
    o2i = hip.H2IL.from_planes(r_pl)
    st_il = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device="cuda")
    hip.gemm(Ail, W, M, N, K, bias=bias.cuda(), out_h2=o2i, residual_h2=(o2i, 1.0 / XS), out_scale=XS, row_stats=st_il, workspace=ws, w_il=Wil)
    torch.cuda.synchronize()
    N8 = N
    assert torch.equal(oi.planes().t[:, :, :N8], o.t)
    assert torch.equal(ohi.planes().t[:, :, :N8], oh.t)
    assert torch.equal(o2i.planes().t[:, :, :N8], o2.t) and torch.equal(st_il, st_ref)
    assert bool(torch.isnan(oi.planes().t[:, :, N8 + (-N8) % 32:]).all())            # nothing written past the last chunk of N
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double()
    assert relerr(oi.float()[:, :N].cpu().double(), ref) < 3e-6
    if ws is not None:
        assert hip.gemm_workspace_errors(ws) == 0


def test_gemm_column_split_partial_round_h2res(hip, monkeypatch):
    """A grid of several rounds with a partial last one (32 x 10 tiles of 256^2 = 1.25 rounds), h2-residual form.  The column split of
    such grids (once CVLM_GEMM_COLSPLIT=2) is gone: any non-zero value now means the one-round split of csrc/gemm_plan.h, which this
    launch (M > 4096, h2 residual) does not take.  Under both values outputs, in-place residual and the statistics pieces carry the
    same bits, and they are right."""
    M, N, K, XS = 8192, 2560, 256, 0.25
    a, w, bias, res = rnd(M, K, seed=61), rnd(N, K, seed=62, scale=K ** -0.5), rnd(N, seed=63), rnd(M, N, seed=64)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    ws = hip.new_gemm_workspace("cuda")
    got = {}
    for cs in ("1", "2"):
        monkeypatch.setenv("CVLM_GEMM_COLSPLIT", cs)
        o2 = hip.H2(hip.H2.pack(res * XS).t.cuda())
        st_out = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o2, residual_h2=(o2, 1.0 / XS), out_scale=XS, row_stats=st_out, workspace=ws)
        torch.cuda.synchronize()
        got[cs] = (o2.t.clone(), st_out)
    assert torch.equal(got["1"][0], got["2"][0]) and torch.equal(got["1"][1], got["2"][1])
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double() + hip.H2.pack(res * XS).float().double() / XS
    assert relerr((got["2"][0][0].float() + got["2"][0][1].float()).cpu().double() / XS, ref) < 3e-6
    assert hip.gemm_workspace_errors(ws) == 0


@pytest.mark.parametrize("M,N,K,sk", [(581, 1024, 1024, "0"), (581, 1024, 4096, "4"), (300, 264, 96, "0"), (581, 3072, 1024, "0"),
                                       (130, 1024, 64, "0"), (581, 1024, 1024, "1")])
def test_gemm_small_grid_ring_depth(hip, monkeypatch, M, N, K, sk):
    """Small grids run the 128^2 kernels over a deep LDS ring (CVLM_GEMM_RING slots, 3-5 K-tiles of DMA in flight: cold weights
    bound a workgroup that has its CU to itself).  The depth changes when a K-tile is fetched, never the order of the
    accumulation: every depth gives the bits of the two-slot loop, for whole tiles and for K-parts, K-tile counts below and above
    the depth included."""
    a, w, bias = rnd(M, K, seed=41), rnd(N, K, seed=42, scale=K ** -0.5), rnd(N, seed=43)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double()
    ws = hip.new_gemm_workspace("cuda")
    monkeypatch.setenv("CVLM_GEMM_SK", sk)
    outs = {}
    for ring, w8 in (("2", "0"), ("3", "0"), ("4", "0"), ("5", "0"), ("4", "1"), ("4", "2"), ("4", "3")):   # w8: eight waves; 2: 64 x 128 tiles, 3: 128^2 tiles, 1: the launcher's pick
        monkeypatch.setenv("CVLM_GEMM_RING", ring)
        monkeypatch.setenv("CVLM_GEMM_W8", w8)
        o = torch.full((M, N), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_f32=o, workspace=ws)
        torch.cuda.synchronize()
        assert relerr(o.cpu().double(), ref) < 3e-6, (ring, w8)
        outs[ring + w8] = o
    for k in ("30", "40", "50", "41", "42", "43"):
        assert torch.equal(outs[k], outs["20"]), k
    assert hip.gemm_workspace_errors(ws) == 0
    assert int(ws[:4096].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("M,N,K,parts", [(581, 1024, 4096, 8), (581, 3072, 1024, 4), (1162, 1024, 1024, 2), (4096, 1280, 5184, 3),
                                          (300, 264, 512, 4)])
def test_gemm_split_k_small_grids(hip, monkeypatch, M, N, K, parts):
    """Split-K form for small grids (one image, CLIP at M = 581): every 128^2 tile cut into K-parts, the last arriver adds the
    slabs in index order.  Same values as the whole-tile launch up to fp32 summation order, bit-identical from run to run
    (the order does not depend on which part arrived last), arrival counters back at zero, every epilogue form."""
    from camouflaged_vlm_amd.engine import LnLinear
    a, w, bias, res = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=K ** -0.5), rnd(N, seed=33), rnd(M, N, seed=34)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    ref = A.float().cpu().double() @ W.float().cpu().double().t() + bias.double() + res.double()
    ws = hip.new_gemm_workspace("cuda")
    outs = []
    for sk in ("0", str(parts), str(parts), "1"):                                   # off, forced, forced again, automatic
        monkeypatch.setenv("CVLM_GEMM_SK", sk)
        o = torch.full((M, N), float("nan"), device="cuda")
        hip.gemm(A, W, M, N, K, bias=bias.cuda(), residual=res.cuda(), out_f32=o, workspace=ws)
        torch.cuda.synchronize()
        outs.append(o)
        assert relerr(o.cpu().double(), ref) < 3e-6, sk
    assert torch.equal(outs[1], outs[2])                                             # fixed summation order
    assert float((outs[0] - outs[1]).abs().max() / ref.abs().max()) < 4e-6
    assert hip.gemm_workspace_errors(ws) == 0
    assert int(ws[:4096].view(torch.int32).abs().sum()) == 0                         # counters and hand-off words back to zero
    # LayerNorm-folded consumer + h2-residual producer through the split-K kernel (N % 8 == 0 shapes)
    if N % 8 == 0 and K % 64 == 0:
        XS = 0.25
        x = rnd(M, K, seed=35) * 2.0
        gamma, beta = 1.0 + 0.1 * rnd(K, seed=36), 0.05 * rnd(K, seed=37)
        xh, st = hip.H2.empty(M, K), torch.empty(hip.stats_pieces(K), M, 2, device="cuda")
        hip.row_stats_split(x.cuda(), XS, xh, st, M, K)
        lin = LnLinear(w, bias, gamma, beta, "cuda")
        got = {}
        for sk in ("0", str(parts)):
            monkeypatch.setenv("CVLM_GEMM_SK", sk)
            o = hip.H2.empty(M, N)
            o.t.fill_(float("nan"))
            st_out = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device="cuda")
            mrg = torch.empty(M, 2, device="cuda")
            hip.ln_stats_merge(st, M, K, 1e-6, mrg, ws)
            hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=1, out_h2=o, ln_fold=(mrg, lin.colsum),
                     workspace=ws)
            o2 = hip.H2(hip.H2.pack(res * XS).t.cuda())
            hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o2, residual_h2=(o2, 1.0 / XS), out_scale=XS, row_stats=st_out, workspace=ws)
            got[sk] = (o.float().cpu().double(), o2.float().cpu().double() / XS, st_out.cpu().double())
        z = F.gelu(F.layer_norm(xh.float().cpu().double() / XS, (K,), gamma.double(), beta.double(), 1e-6) @ w.double().t() + bias.double())
        assert float((got[str(parts)][0] - z).abs().max()) < 2e-5 * max(1.0, float(z.abs().max()))
        assert float((got[str(parts)][0] - got["0"][0]).abs().max()) < 1e-5
        ref2 = ref - res.double() + hip.H2.pack(res * XS).float().double() / XS
        assert relerr(got[str(parts)][1], ref2) < 3e-6
        s_ref, s_mag = piece_stats_ref(ref2)
        assert float(((got[str(parts)][2] - s_ref).abs() / s_mag).max()) < 5e-6
        assert hip.gemm_workspace_errors(ws) == 0


@pytest.mark.parametrize("M,D,N,act", [(700, 160, 480, 0), (4096 + 40, 1280, 768, 1), (520, 1024, 264, 2)])
def test_gemm_layernorm_fold_and_h2_residual(hip, M, D, N, act):
    """The pair of epilogue forms that keep a pre-norm residual stream in h2 (include/cvlm.h, ABI 3):
    producer: x_new = a0 . w0^T + b0 + x_old (residual as h2 planes), stored as h2 and leaving (sum, sum of squares) per row;
    consumer: act(LayerNorm(x_new) . W^T + b) computed from the UN-normalised x_new with the norm folded into the GEMM.
    Rows carry massive channels (x 1e3) like real ViT residual streams."""
    from camouflaged_vlm_amd.engine import LnLinear, Linear
    K0, XS = 96, 2.0 ** -8
    x_old = rnd(M, D, seed=71)
    x_old[:, 3] *= 1e3
    x_old[:, D // 2] *= 300.0
    a0, w0, b0 = rnd(M, K0, seed=72), rnd(D, K0, seed=73, scale=0.1), rnd(D, seed=74)
    gamma, beta = 1.0 + 0.1 * rnd(D, seed=75), 0.05 * rnd(D, seed=76)
    W, b = rnd(N, D, seed=77, scale=D ** -0.5), rnd(N, seed=78, scale=0.05)
    dev = "cuda"
    # ---- producer
    xh = hip.H2.pack(x_old * XS)
    xh = hip.H2(xh.t.to(dev))
    lin0 = Linear(w0, b0, dev)
    A0 = dev_h2(hip, a0)
    stats = torch.full((hip.stats_pieces(D), M, 2), float("nan"), device=dev)      # plain stores: nothing to zero
    hip.gemm(A0, lin0.w, M, D, lin0.K, bias=lin0.bias, alpha=lin0.alpha, out_h2=xh, residual_h2=(xh, 1.0 / XS), out_scale=XS,
             row_stats=stats)
    x_ref = A0.float().cpu().double() @ w0.double().t() + b0.double() + hip.H2.pack(x_old * XS).float().double() / XS
    got = xh.float().cpu().double() / XS
    assert relerr(got, x_ref) < 3e-6
    s_ref, s_mag = piece_stats_ref(x_ref)
    assert float(((stats.cpu().double() - s_ref).abs() / s_mag).max()) < 2e-6
    stats_again = torch.full_like(stats, float("nan"))                              # bit-reproducible: no atomics
    xh_b = hip.H2(hip.H2.pack(x_old * XS).t.to(dev))
    hip.gemm(A0, lin0.w, M, D, lin0.K, bias=lin0.bias, alpha=lin0.alpha, out_h2=xh_b, residual_h2=(xh_b, 1.0 / XS), out_scale=XS,
             row_stats=stats_again)
    assert torch.equal(stats, stats_again) and torch.equal(xh.t, xh_b.t)
    # ---- consumer
    lin = LnLinear(W, b, gamma, beta, dev)
    out = hip.H2.empty(M, N, device=dev)
    out.t.fill_(float("nan"))
    merged = torch.full((M, 2), float("nan"), device=dev)
    hip.ln_stats_merge(stats, M, D, 1e-6, merged)
    mu_ref, var_ref = x_ref.mean(1), x_ref.var(1, unbiased=False)
    rs_ref = (var_ref + 1e-6).rsqrt()
    assert float(((merged[:, 0].cpu().double() - rs_ref).abs() / rs_ref).max()) < 5e-6           # v_rsq: 1 ulp
    assert float(((merged[:, 1].cpu().double() - mu_ref * rs_ref).abs() / (mu_ref.abs() * rs_ref + 1e-3)).max()) < 1e-5
    hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, act=act, out_h2=out, out_scale=0.25,
             ln_fold=(merged, lin.colsum))
    xn = F.layer_norm(got, (D,), gamma.double(), beta.double(), 1e-6)
    z = xn @ W.double().t() + b.double()
    z = {0: z, 1: F.gelu(z), 2: z * torch.sigmoid(1.702 * z)}[act]
    err = float((out.float().cpu().double() / 0.25 - z).abs().max())
    print(f"LN-fold GEMM M={M} D={D} N={N} act={act}: max abs err {err:.2e} (|z| max {float(z.abs().max()):.1f})")
    assert err < 2e-5 * max(1.0, float(z.abs().max()))
    # the row kernel that seeds the stream gives the same planes and statistics as the producer
    xh2, st2 = hip.H2.empty(M, D, device=dev), torch.full((hip.stats_pieces(D), M, 2), float("nan"), device=dev)
    hip.row_stats_split(x_ref.float().to(dev), XS, xh2, st2, M, D)
    assert relerr(xh2.float().cpu().double() / XS, x_ref) < 3e-7
    assert float(((st2.cpu().double() - s_ref).abs() / s_mag).max()) < 2e-6


def piece_stats_ref(x):
    """fp64 piece statistics of rows x [M][D] in the layout of include/cvlm.h: [ceil(D/64)][M][(sum, centred sum of squares)],
    and the magnitudes fp32 errors are relative to (sum |x|, sum x^2 of the piece)."""
    M, D = x.shape
    P = (D + 63) // 64
    ref, mag = torch.zeros(P, M, 2, dtype=torch.float64), torch.ones(P, M, 2, dtype=torch.float64)
    for p in range(P):
        xp = x[:, 64 * p:64 * p + 64].double()
        ref[p, :, 0] = xp.sum(1)
        ref[p, :, 1] = ((xp - xp.mean(1, keepdim=True)) ** 2).sum(1)
        mag[p, :, 0] = xp.abs().sum(1) + 1e-30
        mag[p, :, 1] = (xp * xp).sum(1) + 1e-30
    return ref, mag


@pytest.mark.parametrize("mean,std", [(1e2, 1.0), (-30.0, 0.3), (1e3, 1.0)])
def test_layernorm_fold_common_mode_offset(hip, mean, std):
    """rows whose mean dwarfs their spread through row statistics + folded consumer, against a two-pass fp64
    LayerNorm at the 1e-3 budget.  The statistics are merged as centred moments, so the VARIANCE does not cancel; what is
    left is `alpha * acc - mu * colsum`, which costs |mu| / sigma of the h2 format's 22 bits.  Guaranteed range
    (include/cvlm.h): |mu| / sigma <= 128 within budget; beyond it the row is refused -- NaN outputs and a count in the
    workspace (cvlm_ln_stats_merge), never a finite wrong value."""
    from camouflaged_vlm_amd.engine import LnLinear
    M, D, N, XS = 600, 1280, 256, 0.25
    dev = "cuda"
    x = mean + std * rnd(M, D, seed=81)
    gamma, beta = 1.0 + 0.1 * rnd(D, seed=82), 0.05 * rnd(D, seed=83)
    W, b = rnd(N, D, seed=84, scale=D ** -0.5), rnd(N, seed=85, scale=0.05)
    xh, st = hip.H2.empty(M, D, device=dev), torch.empty(hip.stats_pieces(D), M, 2, device=dev)
    hip.row_stats_split(x.to(dev), XS, xh, st, M, D)
    lin = LnLinear(W, b, gamma, beta, dev)
    out = hip.H2.empty(M, N, device=dev)
    ws = hip.new_gemm_workspace(dev)
    mrg = torch.empty(M, 2, device=dev)
    hip.ln_stats_merge(st, M, D, 1e-6, mrg, ws)
    hip.gemm(xh, lin.w, M, N, lin.K, bias=lin.bias, alpha=lin.alpha / XS, out_h2=out, ln_fold=(mrg, lin.colsum), workspace=ws)
    got = out.float().cpu().double()
    if abs(mean) / std > 128:
        assert bool(torch.isnan(got).all()) and hip.gemm_workspace_errors(ws) == M
        return
    z = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-6) @ W.double().t() + b.double()
    err = float((got - z).abs().max())
    print(f"LN fold, mean {mean:g} std {std:g} (ratio {abs(mean) / std:g}): max abs err {err:.2e} vs two-pass fp64 LayerNorm of the "
          f"f32 input (|z| max {float(z.abs().max()):.2f})")
    assert err < 1e-3 and hip.gemm_workspace_errors(ws) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["h2", "f32_residual", "head_major", "ln_fold_gelu", "h2_residual_stats"])
def test_gemm_persistent_equals_plain(hip, form, monkeypatch):
    """The persistent form of the 256^2 kernel (more tiles than CUs, no tail parts; CVLM_GEMM_PERSIST, default on) gives
    bit-identical outputs to one-workgroup-per-tile launches in every LDS-staged epilogue form, ragged last tiles included."""
    monkeypatch.setenv("CVLM_GEMM_TAIL", "0")
    monkeypatch.setenv("CVLM_GEMM_VARIANT", "7")                       # the 256^2 kernel whatever the tile model prefers
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *sh, scale=1.0: torch.randn(*sh, device=dev, generator=g) * scale
    if form == "head_major":
        Bn, S, Hh, hd = 9, 1024, 8, 80                                 # M = 9216, N = 1920: 36 x 8 = 288 tiles
        M, N, K = Bn * S, 3 * Hh * hd, 96
    else:
        M, N, K = 4648 + 8, 4096 - 8, 128                              # 19 x 16 = 304 tiles, ragged in M and N
    A = hip.H2(rn(2, M, K).half() * torch.tensor([1.0, 2.0 ** -11], device=dev).view(2, 1, 1).half())
    W = hip.H2(rn(2, N, K, scale=0.1).half() * torch.tensor([1.0, 2.0 ** -11], device=dev).view(2, 1, 1).half())
    bias = rn(N)
    res, cs = rn(M, N), rn(N)
    st_in = torch.stack([0.5 + rn(M).abs(), rn(M) * 0.3], 1).contiguous()                     # merged pairs (rstd, mu * rstd)
    x_in = rn(2, M, N).half() * torch.tensor([1.0, 2.0 ** -11], device=dev).view(2, 1, 1).half()
    outs = {}
    for persist in ("0", "1"):
        monkeypatch.setenv("CVLM_GEMM_PERSIST", persist)
        kw = {}
        if form == "h2":
            o = hip.H2.empty(M, N); o.t.fill_(float("nan")); kw = dict(out_h2=o, act=1)
        elif form == "f32_residual":
            o = torch.full((M, N), float("nan"), device=dev); kw = dict(out_f32=o, residual=res)
        elif form == "head_major":
            o = hip.H2.empty(M, N); o.t.fill_(float("nan")); kw = dict(out_h2=o, head_major=(S, Hh, hd))
        elif form == "ln_fold_gelu":
            o = hip.H2.empty(M, N); o.t.fill_(float("nan"))
            kw = dict(out_h2=o, act=1, ln_fold=(st_in, cs), out_scale=0.25)
        else:
            xh = hip.H2(x_in.clone())
            o = hip.H2.empty(M, N); o.t.fill_(float("nan"))
            st = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device=dev)
            kw = dict(out_h2=o, residual_h2=(xh, 4.0), out_scale=0.25, row_stats=st)
        torch.manual_seed(0)
        hip.gemm(A, W, M, N, K, bias=bias, workspace=hip.new_gemm_workspace(dev), **kw)
        torch.cuda.synchronize()
        outs[persist] = (o.t.clone() if isinstance(o, hip.H2) else o.clone(), kw.get("row_stats"))
    a, b = outs["0"][0], outs["1"][0]
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b)
    if form == "h2_residual_stats":                                    # piece statistics: plain stores, bit-identical too
        assert torch.equal(outs["0"][1], outs["1"][1]) and bool(torch.isfinite(outs["0"][1]).all())


@pytest.mark.parametrize("M,N,K", [(9296, 1024, 256), (9296 - 100, 1024, 4096), (6000, 768, 128), (4104, 2056, 512)])
def test_gemm_192_row_tiles_equal_256_row_tiles(hip, monkeypatch, M, N, K):
    """Grids under one round of 256^2 tiles (CLIP out_proj / c_proj of the fused 16-image forward) run on 192 x 256 tiles
    (CVLM_GEMM_T192, h2-residual form): same K order, so outputs and piece statistics are bit-identical to the 256-row tiling,
    ragged last row tile included.  (tests/test_gemm_split3_cpu.py::test_relation_192_row_tiles: the K = 4096 and K = 512 cases reach
    the 192-row kernel; at K = 256 and 128 the model picks 256 x 128 tiles under both settings.)"""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(11)
    rn = lambda *sh, scale=1.0: torch.randn(*sh, device=dev, generator=g) * scale
    planes = torch.tensor([1.0, 2.0 ** -11], device=dev).view(2, 1, 1).half()
    A = hip.H2(rn(2, M, K).half() * planes)
    W = hip.H2(rn(2, N, K, scale=0.1).half() * planes)
    x0 = rn(2, M, N).half() * planes
    bias = rn(N)
    ws = hip.new_gemm_workspace(dev)
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("CVLM_GEMM_T192", flag)
        x = hip.H2(x0.clone())
        st = torch.full((hip.stats_pieces(N), M, 2), float("nan"), device=dev)
        hip.gemm(A, W, M, N, K, bias=bias, out_h2=x, residual_h2=(x, 4.0), out_scale=0.25, row_stats=st, workspace=ws)
        torch.cuda.synchronize()
        got[flag] = (x.t.clone(), st)
    assert bool(torch.isfinite(got["1"][0].float()).all()) and bool(torch.isfinite(got["1"][1]).all())
    assert torch.equal(got["0"][0], got["1"][0]) and torch.equal(got["0"][1], got["1"][1])
    ref = (A.float().double() @ W.float().double().t() + bias.double() + hip.H2(x0).float().double() * 4.0)
    assert float((got["1"][0].float().sum(0).double() / 0.25 - ref).abs().max() / ref.abs().max()) < 3e-6


@pytest.mark.parametrize("Bn,H,W,Cc,N", [(2, 20, 24, 32, 64), (1, 64, 64, 256, 256), (3, 9, 7, 64, 32)])
def test_gemm_implicit_conv3x3(hip, Bn, H, W, Cc, N):
    """conv3x3 = (H, W, C) on the NHWC image == cvlm_im2col3x3 + plain GEMM (same K order: bit-identical), and both match
    torch's conv2d on the fp64 values of the h2 operands (image_encoder.py:150, mask_decoder_edge.py:88-93)."""
    M, K = Bn * H * W, 9 * Cc
    x = rnd(M, Cc, seed=91)
    w = rnd(N, K, seed=92, scale=K ** -0.5)
    bias, res = rnd(N, seed=93), rnd(M, N, seed=94)
    X, Wt = hip.H2.empty(M, Cc), dev_h2(hip, w)
    hip.split_f32(x.cuda(), X)                                       # the same device split im2col applies
    col = hip.H2.empty(M, K)
    hip.im2col3x3(x.cuda(), Bn, H, W, Cc, col)
    o_ref, o_imp = torch.empty(M, N, device="cuda"), torch.full((M, N), float("nan"), device="cuda")
    hip.gemm(col, Wt, M, N, K, bias=bias.cuda(), residual=res.cuda(), out_f32=o_ref)
    hip.gemm(X, Wt, M, N, K, bias=bias.cuda(), residual=res.cuda(), out_f32=o_imp, conv3x3=(H, W, Cc))
    assert torch.equal(o_ref, o_imp)
    xi = X.float().cpu().double().reshape(Bn, H, W, Cc).permute(0, 3, 1, 2)
    wk = Wt.float().cpu().double().reshape(N, 3, 3, Cc).permute(0, 3, 1, 2)
    ref = F.conv2d(xi, wk, bias.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N) + res.double()
    assert relerr(o_imp.cpu().double(), ref) < 3e-6


def test_row_stats_split_copies(hip):
    """cvlm_row_stats_split with copies: the MaPLe deep prompts overwrite the last n rows of every image on an h2 stream."""
    Bn, L, D, n, first, XS = 3, 21, 160, 4, 17, 0.25                  # D = 160: two full pieces and one of 32 columns
    base = rnd(Bn * L, D, seed=61)
    src = rnd(n, D, seed=62) * 3.0
    xh, st = hip.H2.empty(Bn * L, D), torch.full((hip.stats_pieces(D), Bn * L, 2), float("nan"), device="cuda")
    hip.row_stats_split(base.cuda(), XS, xh, st, Bn * L, D)
    hip.row_stats_split(src.cuda(), XS, xh, st, n, D, row0=first, copies=Bn, dst_row_stride=L)
    want = base.clone().reshape(Bn, L, D)
    want[:, first:first + n] = src
    want = want.reshape(Bn * L, D)
    assert relerr(xh.float().cpu().double() / XS, want.double()) < 3e-7
    s_ref, s_mag = piece_stats_ref(want.double())
    assert float(((st.cpu().double() - s_ref).abs() / s_mag).max()) < 2e-6


def to_head_major(qkv, Bn, S, Hh, hd):
    """[B*S][3][H][hd] -> [3][B][H][S][hd] flattened back to the same (B*S, 3*H*hd) buffer shape."""
    return qkv.reshape(Bn, S, 3, Hh, hd).permute(2, 0, 3, 1, 4).contiguous().reshape(Bn * S, 3 * Hh * hd)


def test_gemm_head_major_store(hip):
    Bn, S, Hh, hd, K = 2, 200, 2, 80, 64
    M, N = Bn * S, 3 * Hh * hd
    a, w, bias = rnd(M, K, seed=50), rnd(N, K, seed=51, scale=0.1), rnd(N, seed=52)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    o0, o1 = hip.H2.empty(M, N), hip.H2.empty(M, N)
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o0)
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=o1, head_major=(S, Hh, hd))
    assert torch.equal(o1.t[0].cpu(), to_head_major(o0.t[0].cpu(), Bn, S, Hh, hd))
    assert torch.equal(o1.t[1].cpu(), to_head_major(o0.t[1].cpu(), Bn, S, Hh, hd))


@pytest.mark.parametrize("S,hd,nolo", [(256, 80, 2), (256, 80, 5), (200, 80, 2), (50, 20, 2)])
def test_gemm_head_major_store_without_a_lo_plane(hip, S, hd, nolo):
    """cvlm_gemm_args.hm_nolo (ABI 12): bit w set = the lo plane of third w (q / k / v) of a head-major store is NOT written -- the attention
    kernels' split (1, 2) never reads K's.  Everything else is the bits of the plain head-major store; the skipped thirds keep what was
    there.  (256, 80): the LDS-staged epilogue; (200, 80) and (50, 20): the direct store of the accumulator layout (S below a wave's rows /
    head dim not a multiple of 8)."""
    Bn, Hh, K = 2, 2, 64
    M, N = Bn * S, 3 * Hh * hd
    a, w, bias = rnd(M, K, seed=53), rnd(N, K, seed=54, scale=0.1), rnd(N, seed=55)
    A, W = dev_h2(hip, a), dev_h2(hip, w)
    full, part = hip.H2.empty(M, N), hip.H2.empty(M, N)
    part.t.fill_(7.0)
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=full, head_major=(S, Hh, hd))
    hip.gemm(A, W, M, N, K, bias=bias.cuda(), out_h2=part, head_major=(S, Hh, hd), head_major_nolo=nolo)
    torch.cuda.synchronize()
    assert torch.equal(part.t[0], full.t[0])                            # hi planes: all three thirds
    lo_f, lo_p = full.t[1].reshape(3, -1), part.t[1].reshape(3, -1)     # head-major: the thirds are contiguous
    for which in range(3):
        if (nolo >> which) & 1:
            assert bool((lo_p[which] == 7.0).all()), which
        else:
            assert torch.equal(lo_p[which], lo_f[which]), which


def test_layernorm(hip):
    for M, D, eps in [(37, 1280, 1e-6), (10, 160, 1e-6), (5, 64, 1e-6), (300, 1024, 1e-5)]:
        x, add = rnd(M, D, seed=13) * 3 + 1, rnd(7, D, seed=14)
        g, b = rnd(D, seed=15), rnd(D, seed=16)
        of, oh, so = torch.empty(M, D, device="cuda"), hip.H2.empty(M, D), torch.empty(M, D, device="cuda")
        hip.layernorm(x.cuda(), g.cuda(), b.cuda(), eps, M, D, add=add.cuda(), add_rows=7, sum_out=so, act=1,
                      out_f32=of, out_h2=oh)
        s = x.double() + add.double()[torch.arange(M) % 7]
        ref = F.gelu(F.layer_norm(s, (D,), g.double(), b.double(), eps))
        assert relerr(so, s) < 1e-7
        assert relerr(of, ref) < 3e-6
        assert relerr(oh.float(), ref) < 3e-6


def ref_attention(q, k, v, scale, bias=None, causal=False):
    s = (q * scale) @ k.transpose(-1, -2)
    if bias is not None:
        s = s + bias
    if causal:
        L = s.shape[-1]
        s = s + torch.full((L, L), float("-inf"), dtype=s.dtype).triu_(1)
    return s.softmax(-1) @ v


@pytest.mark.parametrize("split", [(3, 3), (3, 1), (1, 1)])
@pytest.mark.parametrize("S,causal", [(581, False), (77, True), (64, False), (21, False)])
def test_attention_plain(hip, S, causal, split):
    Bn, Hh, hd = 2, 3, 64
    D = Hh * hd
    qkv = rnd(Bn * S, 3 * D, seed=17)
    Q = dev_h2(hip, qkv)
    out = hip.H2.empty(Bn * S, D)
    out.t.fill_(float("nan"))
    hip.attention(Q, out, Bn, S, Hh, hd, mode=0, causal=causal, split_qk=split[0], split_pv=split[1])
    x = Q.float().cpu().double().reshape(Bn, S, 3, Hh, hd).permute(2, 0, 3, 1, 4)
    ref = ref_attention(x[0], x[1], x[2], hd ** -0.5, causal=causal).permute(0, 2, 1, 3).reshape(Bn * S, D)
    tol = {(3, 3): 5e-6, (3, 1): 2e-3, (1, 1): 4e-3}[split]
    assert relerr(out.float(), ref) < tol


@pytest.mark.parametrize("S,q_rows", [(581, 1), (581, 130), (77, 1), (581, 600)])
def test_attention_leading_queries_only(hip, S, q_rows):
    """cvlm_attn_args.q_rows (ABI 9): only the leading query blocks are computed -- the bits of the whole launch in the rows of the
    blocks touched, nothing written behind them (the class-token tail of the CLIP tower asks for q_rows = 1)."""
    Bn, Hh, hd = 3, 4, 64
    D = Hh * hd
    Q = dev_h2(hip, rnd(Bn * S, 3 * D, seed=23))
    full, part = hip.H2.empty(Bn * S, D), hip.H2.empty(Bn * S, D)
    full.t.fill_(float("nan"))
    part.t.fill_(7.0)
    hip.attention(Q, full, Bn, S, Hh, hd, mode=0)
    hip.attention(Q, part, Bn, S, Hh, hd, mode=0, q_rows=q_rows)
    torch.cuda.synchronize()
    rows = min(S, -(-min(q_rows, S) // 128) * 128)                    # whole 128-query blocks
    f, g = full.t.view(2, Bn, S, D), part.t.view(2, Bn, S, D)
    assert torch.equal(g[:, :, :rows], f[:, :, :rows]) and bool(torch.isfinite(f.float()).all())
    assert bool((g[:, :, rows:] == 7.0).all())
    with pytest.raises(RuntimeError):                                  # the relative-position modes have no such form
        hip.attention(Q, part, Bn, S, Hh, hd, mode=1, grid=1, q_rows=1)


def relpos_bias(q, rel_h, rel_w, L):
    """image_encoder.py:589-625 on (N, L*L, hd) queries."""
    idx = torch.arange(L)[:, None] - torch.arange(L)[None, :] + (L - 1)
    Rh, Rw = rel_h[idx], rel_w[idx]
    rq = q.reshape(q.shape[0], L, L, -1)
    bh = torch.einsum("bhwc,hkc->bhwk", rq, Rh)
    bw = torch.einsum("bhwc,wkc->bhwk", rq, Rw)
    return (bh[:, :, :, :, None] + bw[:, :, :, None, :]).reshape(q.shape[0], L * L, L * L)


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("split", [(3, 3), (2, 2), (1, 2), (1, 1)])
@pytest.mark.parametrize("G", [20, 64, 96])
def test_attention_global_relpos(hip, G, split, hm):
    Bn, Hh, hd = (2, 2, 80) if G == 20 else (1, 2, 80)
    D, S = Hh * hd, G * G
    qkv = rnd(Bn * S, 3 * D, seed=18)
    rel_h, rel_w = rnd(2 * G - 1, hd, seed=19, scale=0.2), rnd(2 * G - 1, hd, seed=20, scale=0.2)
    Q, RH, RW = dev_h2(hip, qkv), dev_h2(hip, rel_h), dev_h2(hip, rel_w)
    out = hip.H2.empty(Bn * S, D)
    out.t.fill_(float("nan"))
    Qk = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)])) if hm else Q
    hip.attention(Qk, out, Bn, S, Hh, hd, mode=1, grid=G, rel_h=RH, rel_w=RW, split_qk=split[0], split_pv=split[1],
                  head_major=hm)
    x = Q.float().cpu().double().reshape(Bn, S, 3, Hh, hd).permute(2, 0, 3, 1, 4).reshape(3, Bn * Hh, S, hd)
    bias = relpos_bias(x[0], RH.float().cpu().double(), RW.float().cpu().double(), G)
    ref = ref_attention(x[0], x[1], x[2], hd ** -0.5, bias=bias)
    ref = ref.reshape(Bn, Hh, S, hd).permute(0, 2, 1, 3).reshape(Bn * S, D)
    err = relerr(out.float(), ref)
    print(f"global attention G={G} split={split} head-major={hm}: {err:.2e}")
    assert err < SPLIT_TOL[split]
    if split in ((2, 2), (1, 2)) and G in (64, 96):            # the ViT-H maps have kernels of their own for them (include/cvlm.h ABI 11 / 12), G = 20 runs them as (3, 3)
        assert err > 5e-6
    if split in ((2, 2), (1, 2)) and G == 20:
        full = hip.H2.empty(Bn * S, D)
        hip.attention(Qk, full, Bn, S, Hh, hd, mode=1, grid=G, rel_h=RH, rel_w=RW, split_qk=3, split_pv=3, head_major=hm)
        assert torch.equal(full.t, out.t)                      # "every other shape runs (2, 2) as (3, 3)": the same bits


# (2, 2): K and V with their lo planes, Q and the probabilities without (include/cvlm.h): one fp16 rounding of P and of q, 2^-12 rms each.
# On these operands (scores ~ N(0, 1): thousands of keys share a query's weight) the OUTPUT is an average ~ |v| / sqrt(N_eff) and the
# rounding noise averages the same way: 1.4e-4 rms of the output, 2.8e-4 at the worst of 1.3 M elements (measured).
# (1, 2), ABI 12: K as its hi plane too -- one more rounding of the same size in the scores.
SPLIT_TOL = {(3, 3): 5e-6, (2, 2): 6e-4, (1, 2): 7e-4, (3, 1): 5e-3, (1, 1): 5e-3}


def test_attention_is_deterministic_under_load(hip):
    """Race screen for the LDS-DMA rings (counted vmcnt + raw barriers): repeated launches on a fully loaded chip
    (B = 8 cascade shape) must reproduce the first result bit for bit."""
    B, H, hd, G = 8, 16, 80, 64
    D, S = H * hd, G * G
    g = torch.Generator(device="cuda").manual_seed(5)
    qkv = hip.H2(torch.randn(2, B * S, 3 * D, device="cuda", generator=g).half())
    rg = hip.H2((torch.randn(2, 2 * G - 1, hd, device="cuda", generator=g) * 0.1).half())
    rw = hip.H2((torch.randn(2, 27, hd, device="cuda", generator=g) * 0.1).half())
    pad = hip.H2((torch.randn(2, 3 * D, device="cuda", generator=g) * 0.1).half())
    for sp in (3, 2, 1):
        for kw in (dict(mode=1, grid=G, rel_h=rg, rel_w=rg), dict(mode=2, grid=G, window=14, pad=pad, rel_h=rw, rel_w=rw)):
            outs = []
            for _ in range(4 if sp == 3 else 3):
                out = hip.H2.empty(B * S, D)
                out.t.fill_(float("nan"))
                hip.attention(qkv, out, B, S, H, hd, split_qk=sp, split_pv=max(sp, 2), head_major=True, **kw)
                outs.append(out.t.clone())
            assert not torch.isnan(outs[0].float()).any()
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (sp, kw["mode"])


def ref_window_attention(x, pad, rel_h, rel_w, Bn, G, ws, Hh, hd, scale):
    """image_encoder.py:488-504, 507-553 on token-major qkv rows x [Bn*G*G][3*Hh*hd]: pad the token map with the pad vector (= qkv of a
    zero token), partition, attend with the rel-pos bias, unpartition -> [Bn*G*G][Hh*hd], in the precision of its arguments"""
    D = Hh * hd
    Gp = -(-G // ws) * ws
    xp = pad.expand(Bn, Gp, Gp, 3 * D).clone()
    xp[:, :G, :G] = x.reshape(Bn, G, G, 3 * D)
    nw = Gp // ws
    win = xp.reshape(Bn, nw, ws, nw, ws, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(Bn * nw * nw, ws * ws, 3, Hh, hd)
    win = win.permute(2, 0, 3, 1, 4).reshape(3, -1, ws * ws, hd)
    bias = relpos_bias(win[0], rel_h, rel_w, ws)
    o = ref_attention(win[0], win[1], win[2], scale, bias=bias)
    o = o.reshape(Bn * nw * nw, Hh, ws * ws, hd).permute(0, 2, 1, 3).reshape(Bn, nw, nw, ws, ws, D)
    return o.permute(0, 1, 3, 2, 4, 5).reshape(Bn, Gp, Gp, D)[:, :G, :G].reshape(Bn * G * G, D)


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("split", [(3, 3), (2, 2), (1, 2), (3, 1), (1, 1)])
@pytest.mark.parametrize("G", [20, 64])
def test_attention_window_relpos(hip, G, split, hm):
    """Bn = 2, two heads: 16 (G = 20) or 100 (G = 64) pairs, so every workgroup of the persistent kernel runs one pair and exits;
    tests/test_attention_window_pairs_gpu.py is where pairs follow each other in a workgroup."""
    ws, Bn, Hh, hd = 14, 2, 2, 80
    D, S = Hh * hd, G * G
    qkv = rnd(Bn * S, 3 * D, seed=21)
    pad = rnd(3 * D, seed=22, scale=0.3)
    rel_h, rel_w = rnd(2 * ws - 1, hd, seed=23, scale=0.2), rnd(2 * ws - 1, hd, seed=24, scale=0.2)
    Q, P, RH, RW = dev_h2(hip, qkv), dev_h2(hip, pad), dev_h2(hip, rel_h), dev_h2(hip, rel_w)
    out = hip.H2.empty(Bn * S, D)
    out.t.fill_(float("nan"))
    Qk = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)])) if hm else Q
    hip.attention(Qk, out, Bn, S, Hh, hd, mode=2, grid=G, window=ws, pad=P, rel_h=RH, rel_w=RW,
                  split_qk=split[0], split_pv=split[1], head_major=hm)
    o = ref_window_attention(Q.float().cpu().double(), P.float().cpu().double(), RH.float().cpu().double(), RW.float().cpu().double(),
                             Bn, G, ws, Hh, hd, hd ** -0.5)
    err = relerr(out.float(), o)
    print(f"window attention G={G} split={split} head-major={hm}: {err:.2e}")
    assert err < SPLIT_TOL[split]
    assert not torch.isnan(out.t).any()                      # every row of the output was written


def test_small_attention(hip):
    for (Bn, nq, nk, Hh, hd) in [(2, 6, 400, 8, 16), (2, 400, 6, 8, 16), (2, 6, 6, 8, 32), (1, 400, 2, 8, 16), (1, 6, 4096, 8, 16),
                                 (2, 5, 1300, 8, 32)]:
        D = Hh * hd
        q, k, v = rnd(Bn, nq, D, seed=25), rnd(Bn, nk, D, seed=26), rnd(Bn, nk, D, seed=27)
        out = torch.empty(Bn, nq, D, device="cuda")
        hip.small_attention(q.cuda(), k.cuda(), v.cuda(), out, Bn, nq, nk, Hh, hd)
        sp = lambda t, n: t.double().reshape(Bn, n, Hh, hd).transpose(1, 2)
        ref = ref_attention(sp(q, nq), sp(k, nk), sp(v, nk), 1 / math.sqrt(hd)).transpose(1, 2).reshape(Bn, nq, D)
        assert relerr(out, ref) < 3e-6
        # ABI 7: q | k | v as column blocks of one merged projection (row pitch 3 D), the result as h2 planes only / as both
        if nq == nk:
            qkv = torch.cat([q, k, v], dim=-1).reshape(Bn * nq, 3 * D).cuda().contiguous()
            blocks = (qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:])
        else:
            kv = torch.cat([k, v], dim=-1).reshape(Bn * nk, 2 * D).cuda().contiguous()
            blocks = (q.reshape(Bn * nq, D).cuda(), kv[:, :D], kv[:, D:])
        oh = hip.H2.empty(Bn * nq, D)
        hip.small_attention(*blocks, None, Bn, nq, nk, Hh, hd, out_h2=oh)
        assert relerr(oh.float().reshape(Bn, nq, D), ref) < 3e-6
        out2, oh2 = torch.empty(Bn * nq, D, device="cuda"), hip.H2.empty(Bn * nq, D)
        hip.small_attention(*blocks, out2, Bn, nq, nk, Hh, hd, out_h2=oh2)
        assert torch.equal(out2.reshape(Bn, nq, D), out) and torch.equal(oh2.t, oh.t)
    with pytest.raises(RuntimeError):                                  # head dims other than the decoder's two are refused, loudly
        hip.small_attention(torch.zeros(1, 2, 24, device="cuda"), torch.zeros(1, 2, 24, device="cuda"), torch.zeros(1, 2, 24, device="cuda"),
                            torch.empty(1, 2, 24, device="cuda"), 1, 2, 2, 1, 24)


def test_patchify_and_im2col(hip):
    Bn, H, Wd, p = 2, 28, 42, 14
    img, al = rnd(Bn, 3, H, Wd, seed=28), rnd(Bn, 1, H, Wd, seed=29)
    K = 4 * p * p
    ldk = (K + 31) // 32 * 32
    out = hip.H2.empty(Bn * (H // p) * (Wd // p), ldk)
    out.t.fill_(float("nan"))
    hip.patchify(img.cuda(), al.cuda(), p, out, ldk)
    cat = torch.cat([img, al], 1)
    ref = F.unfold(cat, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, K)     # (c, iy, ix) column order
    got = out.float().cpu()
    assert relerr(got[:, :K], ref) < 1e-6 and float(got[:, K:].abs().max()) == 0.0
    Bn, H, Wd, Cc = 2, 9, 7, 32
    x = rnd(Bn, H, Wd, Cc, seed=30)
    out = hip.H2.empty(Bn * H * Wd, 9 * Cc)
    hip.im2col3x3(x.cuda(), Bn, H, Wd, Cc, out)
    u = F.unfold(x.permute(0, 3, 1, 2), kernel_size=3, padding=1)                   # (B, C*9, HW), (c, ky, kx)
    ref = u.reshape(Bn, Cc, 9, H * Wd).permute(0, 3, 2, 1).reshape(Bn * H * Wd, 9 * Cc)
    assert relerr(out.float(), ref) < 1e-6


def test_misc_rowops(hip):
    Bn, T, D = 2, 100, 48
    x = rnd(Bn, T, D, seed=31)
    out = hip.H2.empty(Bn * T, D)
    hip.reinterpret_transpose(x.cuda(), Bn, T, D, out)
    assert relerr(out.float(), x.reshape(Bn, D, T).permute(0, 2, 1).reshape(Bn * T, D)) < 1e-6
    # dense PE
    gm = rnd(2, 128, seed=32)
    pe = torch.empty(20 * 20, 256, device="cuda")
    hip.dense_pe(gm.cuda(), 20, 256, pe)
    from oracle import cvlm_oracle as O
    ref = O.dense_pe({"pe_layer.positional_encoding_gaussian_matrix": gm.double()}, 20).permute(1, 2, 0).reshape(400, 256)
    assert float((pe.cpu().double() - ref).abs().max()) < 2e-5
    # bilinear up x4 and down 1024->336 with sigmoid
    a = rnd(2, 40, 40, seed=33)
    up = torch.empty(2, 160, 160, device="cuda")
    hip.bilinear(a.cuda(), 2, 40, 40, up, 160, 160)
    assert relerr(up, F.interpolate(a.double()[:, None], (160, 160), mode="bilinear", align_corners=False)[:, 0]) < 1e-6
    a = rnd(1, 320, 320, seed=34) * 3
    dn = torch.empty(1, 56, 56, device="cuda")
    hip.bilinear(a.cuda(), 1, 320, 320, dn, 56, 56, sigmoid_in=True)
    # source coordinates are computed in fp32 like torch's fp32 CPU kernel (the reference's dtype)
    ref = F.interpolate(torch.sigmoid(a)[:, None], (56, 56), mode="bilinear", align_corners=False)[:, 0]
    assert relerr(dn, ref) < 3e-6
    # mask head
    Bn, HW, Cc = 2, 300, 32
    u, e, h = rnd(Bn, HW, Cc, seed=35), rnd(Bn, HW, Cc, seed=36), rnd(Bn, 5, Cc, seed=37)
    low = torch.empty(Bn, HW, device="cuda")
    hip.mask_head(u.cuda(), e.cuda(), h.cuda(), Bn, HW, Cc, low)
    m = torch.einsum("bpc,bc->bp", u.double(), h.double()[:, 0])
    g = torch.sigmoid(torch.einsum("bpc,bc->bp", e.double(), h.double()[:, 4]))
    assert relerr(low, m * g + m) < 3e-6
    # clip head
    Bn, Cc, D = 3, 61, 768
    img, txt = rnd(Bn, D, seed=38), rnd(Cc, D, seed=39)
    img_n, logits = torch.empty(Bn, D, device="cuda"), torch.empty(Bn, Cc, device="cuda")
    pred, sel = torch.empty(Bn, dtype=torch.int64, device="cuda"), torch.empty(Bn, D, device="cuda")
    hip.clip_head(img.cuda(), txt.cuda(), 100.0, Bn, Cc, D, img_n, logits, pred, sel)
    n = img.double() / img.double().norm(dim=-1, keepdim=True)
    rl = 100.0 * n @ txt.double().t()
    assert relerr(img_n, n) < 1e-6 and relerr(logits, rl) < 3e-6
    assert pred.cpu().tolist() == rl.argmax(1).tolist() and relerr(sel, txt[rl.argmax(1)]) == 0.0
    # add_rows / split / assemble / overwrite / gather / normalize_add
    a, b = rnd(10, 64, seed=40), rnd(5, 64, seed=41)
    of, oh = torch.empty(10, 64, device="cuda"), hip.H2.empty(10, 64)
    hip.add_rows(a.cuda(), b.cuda(), 5, 10, 64, scale=2.0, out_f32=of, out_h2=oh)
    ref = 2.0 * (a + b[torch.arange(10) % 5])
    assert relerr(of, ref) == 0.0 and relerr(oh.float(), ref) < 1e-6
    pt, cls, pos, ctx = rnd(2, 16, 64, seed=42), rnd(64, seed=43), rnd(17, 64, seed=44), rnd(4, 64, seed=45)
    tok = torch.empty(2, 21, 64, device="cuda")
    hip.clip_assemble(pt.cuda(), cls.cuda(), pos.cuda(), ctx.cuda(), 2, 16, 64, 4, tok)
    ref = torch.cat([torch.cat([cls.expand(2, 1, 64), pt], 1) + pos, ctx.expand(2, 4, 64)], 1)
    assert relerr(tok, ref) == 0.0
    src = rnd(4, 64, seed=46)
    hip.overwrite_rows(tok, 2, 21, 64, 17, 4, src.cuda())
    ref[:, 17:] = src
    assert relerr(tok, ref) == 0.0
    g0 = torch.empty(2, 64, device="cuda")
    hip.gather_rows(tok, 2, 21, 64, torch.tensor([3, 20], dtype=torch.int32).cuda(), 0, g0)
    assert relerr(g0, torch.stack([ref[0, 3], ref[1, 20]])) == 0.0
    x, ad = rnd(5, 768, seed=47), rnd(5, 768, seed=48)
    o = torch.empty(5, 768, device="cuda")
    hip.normalize_add(x.cuda(), ad.cuda(), 5, 768, o)
    assert relerr(o, x.double() / x.double().norm(dim=-1, keepdim=True) + ad.double()) < 1e-6
