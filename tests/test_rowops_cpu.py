"""The oracles of tests/rowops_oracle.py against torch's own operators, and the refusals of the row-kernel launchers (csrc/rowops.hip).

Neither half needs a GPU.  The library loads without a device (tests/test_gemm_plan_cpu.py), and a launcher that refuses its arguments
returns before it launches anything -- so every refusal below is held to its exact code: without a device a call that is NOT refused
fails as well, with a HIP error, and a test that only asked for a failure would pass either way.  Pointers are made-up addresses:
no refused call reads one."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowops_oracle as O
from camouflaged_vlm_amd import hip

E_BADARG, E_UNSUPPORTED = -1, -2


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


# ---- the oracles ---------------------------------------------------------------------------------------------------------------------
def test_rowerr_sees_the_row_the_global_measure_hides():
    ref = torch.ones(3, 8, dtype=torch.float64)
    ref[0] *= 1000.0
    ref[2] *= 1e-3
    got = ref.clone()
    got[2, 5] += 1e-6                                                 # 1e-3 of its row, 1e-9 of the tensor's maximum
    assert O.globalerr(got, ref) < 3e-6
    assert O.rowerr(got, ref) > 5e-4
    assert O.rowerrs(got, ref).tolist()[:2] == [0.0, 0.0]
    planes = ref.reshape(3, 2, 4)                                     # row_dims = 2: a plane is a row
    assert O.rowerrs(got.reshape(3, 2, 4), planes, 2).shape == (3,) and O.rowerr(got.reshape(3, 2, 4), planes, 2) > 5e-4
    got[0, 0] = float("nan")
    assert math.isnan(O.rowerr(got, ref))                             # an unwritten element never passes a `<`
    assert not O.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and O.same_bits(torch.tensor([-0.0]), torch.tensor([-0.0]))


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("M,D,add_rows", [(5, 4, None), (37, 260, 7), (3, 2048, 1)])
def test_layernorm_oracle(M, D, add_rows, act):
    x = O.layernorm_rows(M, D, seed=1)
    add = None if add_rows is None else rnd(add_rows, D, seed=2)
    g, b = rnd(D, seed=3), rnd(D, seed=4)
    s, y, r = O.layernorm(x, g, b, 1e-5, add=add, act=act)
    s_ref = x.double() if add is None else x.double() + add.double()[torch.arange(M) % add_rows]
    z = F.layer_norm(s_ref, (D,), g.double(), b.double(), 1e-5)
    z = {0: z, 1: F.gelu(z), 2: z * torch.sigmoid(1.702 * z), 3: F.relu(z)}[act]
    assert torch.equal(s, s_ref)
    assert O.rowerr(y, z) < 1e-12
    r_ref = s_ref.mean(1).abs() / (s_ref.var(1, unbiased=False) + 1e-5).sqrt()
    assert float((r - r_ref).abs().max() / r_ref.abs().max().clamp_min(1.0)) < 1e-12
    if add is None and M >= 8:                                        # the families are what they say
        assert float(r[3]) > 90 and float(r[4]) > 90 and float(r[5]) > 30 and float(r[6]) == 0.0 and float(r[0]) < 1.0


def test_layernorm_offset_yardstick():
    """The bound of layernorm_tolerance is four times what torch's own float32 LayerNorm loses on rows with a common offset."""
    D = 1280
    for off, std, want_r in ((100.0, 1.0, 100.0), (-30.0, 0.3, 100.0), (1000.0, 1.0, 1000.0)):
        x = rnd(16, D, seed=5) * std + off
        g, b = torch.ones(D), torch.zeros(D)
        _, y, r = O.layernorm(x, g, b, 1e-6)
        assert abs(float(r.mean()) / want_r - 1.0) < 0.1
        ratio = O.rowerrs(F.layer_norm(x, (D,), g, b, 1e-6), y) / (2.0 ** -24 * r)
        print(f"float32 F.layer_norm, offset {off:g} std {std:g}: rowerr = {float(ratio.max()):.2f} * 2^-24 r")
        assert float(ratio.max()) < 4.0


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 1, 5, 8), (1, 5, 1, 16), (3, 9, 7, 64)])
def test_im2col_oracle(B, H, W, C):
    x = rnd(B, H, W, C, seed=6)
    u = F.unfold(x.permute(0, 3, 1, 2), kernel_size=3, padding=1)                     # (B, C * 9, HW), (c, ky, kx)
    ref = u.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    assert torch.equal(O.im2col3x3(x), ref)


@pytest.mark.parametrize("B,C0,C1,H,W,p,ldk", [(1, 3, 0, 28, 42, 14, 608), (3, 3, 1, 42, 28, 14, 800), (2, 1, 2, 6, 4, 2, 16)])
def test_patchify_oracle(B, C0, C1, H, W, p, ldk):
    s0, s1 = rnd(B, C0, H, W, seed=7), (rnd(B, C1, H, W, seed=8) if C1 else None)
    K = (C0 + C1) * p * p
    got = O.patchify(s0, s1, p, ldk)
    cat = s0 if s1 is None else torch.cat([s0, s1], 1)
    ref = F.unfold(cat, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, K)       # (c, iy, ix) column order
    assert got.shape == (B * (H // p) * (W // p), ldk)
    assert torch.equal(got[:, :K], ref) and O.same_bits(got[:, K:], torch.zeros(got.shape[0], ldk - K))


BILINEAR_SHAPES = [(37, 53, 101, 67), (64, 48, 21, 29), (1, 9, 5, 30), (9, 1, 30, 5), (96, 64, 37, 1), (336, 224, 100, 75), (5, 7, 5, 7),
                   (7, 5, 1, 1), (40, 24, 1024, 768)]


@pytest.mark.parametrize("hin,win,hout,wout", BILINEAR_SHAPES)
def test_bilinear_oracle_is_float32_interpolate(hin, win, hout, wout):
    """Float32 coordinates: the oracle is within coordinate rounding of torch's float32 operator (measured <= 3.4e-6), which an
    fp64-coordinate evaluation is not (3.7e-5 at 336 x 224 -> 100 x 75)."""
    x = rnd(3, hin, win, seed=9)
    for sig in (False, True):
        src = torch.sigmoid(x) if sig else x
        ref = F.interpolate(src[:, None], (hout, wout), mode="bilinear", align_corners=False)[:, 0]
        assert O.globalerr(O.bilinear(x, hout, wout, sigmoid_in=sig), ref) < 1e-5
    if (hin, win) == (hout, wout):
        assert torch.equal(O.bilinear(x, hout, wout), x.double())


def test_bilinear_oracle_coordinates():
    i0, i1, lam = O.bilinear_axis(4, 8)                               # scale 0.5: src = -0.25 (clamped), 0.25, 0.75, ..., 3.25
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25] and lam.dtype.name == "float32"
    i0, i1, lam = O.bilinear_axis(7, 1)
    assert (i0.tolist(), i1.tolist(), lam.tolist()) == ([3], [4], [0.0])


@pytest.mark.parametrize("nq,nk,heads,hd", [(1, 1, 1, 16), (3, 65, 2, 32), (2, 257, 3, 16)])
def test_small_attention_oracle(nq, nk, heads, hd):
    B, D = 2, heads * hd
    q, k, v = rnd(B, nq, D, seed=10), rnd(B, nk, D, seed=11), rnd(B, nk, D, seed=12)
    sp = lambda t, n: t.double().reshape(B, n, heads, hd).transpose(1, 2)
    dense = (torch.softmax(sp(q, nq) @ sp(k, nk).transpose(-1, -2) / math.sqrt(hd), -1) @ sp(v, nk)).transpose(1, 2).reshape(B, nq, D)
    assert O.rowerr(O.small_attention(q, k, v, heads, hd), dense) < 1e-12


def test_remaining_oracles():
    x = rnd(2, 5, 3, seed=13)                                         # reinterpret_transpose: out[b][t][c] = flat[b][c * T + t]
    got = O.reinterpret_transpose(x, 2, 5, 3, 0.25)
    assert got.shape == (10, 3) and float(got[5 + 4, 2]) == float(x[1].reshape(-1)[2 * 5 + 4]) * 0.25
    a, b = rnd(10, 4, seed=14), rnd(7, 4, seed=15)
    assert torch.equal(O.add_rows_f32(a, b, 0.25)[9], (a[9] + b[2]) * 0.25) and torch.equal(O.add_rows_f32(a, None, 0.25), a * 0.25)
    pt, cls, pos, ctx = rnd(2, 3, 4, seed=16), rnd(4, seed=17), rnd(4, 4, seed=18), rnd(4, 4, seed=19)
    tok = O.clip_assemble(pt, cls, pos, ctx, 2)
    assert tok.shape == (2, 6, 4) and torch.equal(tok[1, 0], cls + pos[0]) and torch.equal(tok[1, 2], pt[1, 1] + pos[2])
    assert torch.equal(tok[0, 5], ctx[1]) and O.clip_assemble(pt, cls, pos, ctx, 0).shape == (2, 4, 4)
    gm = rnd(2, 3, seed=20)
    pe = O.dense_pe(gm, 7)                                            # token (y, x) = (2, 5), frequency 1
    ph = 2 * math.pi * ((2 * 5.5 / 7 - 1) * float(gm[0, 1]) + (2 * 2.5 / 7 - 1) * float(gm[1, 1]))
    assert pe.shape == (49, 6) and abs(float(pe[2 * 7 + 5, 1]) - math.sin(ph)) < 1e-12 and abs(float(pe[2 * 7 + 5, 4]) - math.cos(ph)) < 1e-12
    u, e, h = rnd(2, 5, 4, seed=21), rnd(2, 5, 4, seed=22), rnd(2, 5, 4, seed=23)
    m = float(u[1, 3].double() @ h[1, 0].double())
    s = 1.0 / (1.0 + math.exp(-float(e[1, 3].double() @ h[1, 4].double())))
    assert abs(float(O.mask_head(u, e, h)[1, 3]) - (m * s + m)) < 1e-12 and abs(float(O.mask_head(u, None, h)[1, 3]) - m) < 1e-12
    img, txt = rnd(3, 8, seed=24), rnd(5, 8, seed=25)
    n, lg = O.clip_head(img, txt, 100.0)
    assert O.rowerr(n, F.normalize(img.double(), dim=-1)) < 1e-12 and O.rowerr(lg, 100.0 * F.normalize(img.double(), dim=-1) @ txt.double().t()) < 1e-12
    assert O.rowerr(O.normalize_add(img, img), F.normalize(img.double(), dim=-1) + img.double()) < 1e-12
    v = O.split_adversaries()
    assert float(v.abs().max()) == 65504.0 and float(v[v != 0].abs().min()) >= 2.0 ** -25 and v.numel() > 400
    for mid, even in ((1.0 + 2.0 ** -11, 1.0), (1.0 + 2.0 ** -10 + 2.0 ** -11, 1.0 + 2.0 ** -9), (2.0 ** -25, 0.0)):
        assert bool((v == mid).any()) and float(torch.tensor(mid).half()) == even    # exact midpoints: ties go to the even mantissa


# ---- the launchers' refusals ---------------------------------------------------------------------------------------------------------
P = [0x1000000 * (i + 1) for i in range(10)]                          # made-up, 16-byte aligned, distinct


@pytest.fixture(scope="module")
def lib():
    return hip.load()


def test_layernorm_refusals(lib):
    ln = lambda D, ldx=None, add=None, add_rows=0, M=3: lib.cvlm_layernorm(P[0], D if ldx is None else ldx, add, add_rows, None, P[1], P[2],
                                                                          1e-6, 0, P[3], None, None, M, D, None)
    assert ln(6) == E_BADARG                                          # D % 4
    assert ln(2052) == E_BADARG                                       # D > 2048: the row no longer fits a wave's registers
    assert ln(64, add=P[4], add_rows=0) == E_BADARG                   # add without add_rows
    assert ln(64, ldx=66) == E_BADARG and ln(64, M=0) == E_BADARG
    assert lib.cvlm_add_rows(P[0], P[1], 0, 1.0, P[2], None, None, 3, 64, None) == E_BADARG
    assert lib.cvlm_add_rows(P[0], None, 0, 1.0, P[2], None, None, 3, 6, None) == E_BADARG
    assert lib.cvlm_split_f32(P[0], P[1], P[2], 6, None) == E_BADARG


def test_small_attention_refusals(lib):
    sa = lambda hd, ldq=64, heads=2: lib.cvlm_small_attention_h2(P[0], ldq, P[1], 64, P[2], 64, P[3], 64, None, None, 0, 1, 2, 2, heads, hd, None)
    assert sa(24) == E_UNSUPPORTED                                    # the decoder's head dims only
    assert sa(16, ldq=34) == E_BADARG                                 # a pitch that is no multiple of four floats
    assert lib.cvlm_small_attention(P[0], 64, P[1], 64, P[2], 64, P[3], 64, 1, 2, 2, 1, 24, None) == E_UNSUPPORTED
    assert lib.cvlm_small_attention(P[0] + 4, 64, P[1], 64, P[2], 64, P[3], 64, 1, 2, 2, 2, 16, None) == E_BADARG


def test_gather_and_im2col_and_head_refusals(lib):
    pf = lambda H, W, p, ldk: lib.cvlm_patchify(P[0], 3, None, 0, 1, H, W, p, P[1], P[2], ldk, None)
    assert pf(28, 42, 14, 584) == E_BADARG                            # ldk < K = 588
    assert pf(30, 42, 14, 608) == E_BADARG and pf(28, 40, 14, 608) == E_BADARG       # H % p, W % p
    assert pf(28, 42, 14, 604) == E_BADARG                            # ldk % 8
    assert lib.cvlm_patchify(P[0], 3, None, 1, 1, 28, 42, 14, P[1], P[2], 800, None) == E_BADARG      # C1 without src1
    assert lib.cvlm_im2col3x3(P[0], 1, 4, 4, 12, P[1], P[2], None) == E_BADARG       # C % 8
    assert lib.cvlm_clip_head(P[0], P[1], 100.0, 1, 1025, 64, P[2], P[3], P[4], P[5], None) == E_BADARG  # C > 1024
    assert lib.cvlm_clip_head(P[0], P[1], 100.0, 1, 0, 64, P[2], P[3], P[4], P[5], None) == E_BADARG


@pytest.mark.parametrize("B,L,W,fixed", [(2, 5, 64, 5), (2, 5, 64, -1), (2, 1, 64, 1), (0, 5, 64, 0), (2, 0, 64, 0), (2, 5, 0, 0),
                                          (2, 5, 6, 0), (2, 5, 64, 2 ** 31 - 1)])
def test_gather_rows_refuses_a_fixed_row_outside_the_sequence(lib, B, L, W, fixed):
    """idx == NULL: the row is the launcher's to check -- a `fixed` outside [0, L) would read outside x.  (A given idx is the caller's
    contract, include/cvlm.h.)  Refused before any launch, so this runs without a device; it has no GPU twin."""
    assert lib.cvlm_gather_rows(P[0], B, L, W, None, fixed, P[1], None) == E_BADARG
    assert lib.cvlm_gather_rows_h2(P[0], P[1], 0.25, B, L, W, None, fixed, P[2], None) == E_BADARG
