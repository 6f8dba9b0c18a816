"""Precision `fast` (split = 1) of cvlm_gemm: the four instantiations that exist for split 1 only, in every launch form of the cascade,
against fp64 of the planes they read (tests/gemm_split1_cases.py holds the cases and why those shapes).

Operands are H2.pack of N(0, 1) activations and K ** -0.5 weights with the lo planes of A and W set to NaN: a split-1 launch must not
read them, and any read shows as a NaN.  With the reference computed from the same fp16 hi planes the error left is fp32 accumulation
and the epilogue's rounding, so the bounds are those the split-3 tests of tests/test_ops_gpu.py use for the same forms: 2e-6 of |ref|max
for the bias-free product, 3e-6 for every epilogue form (h2 outputs after dividing by out_scale), 2e-5 * max(1, |z|max) absolute for the
LayerNorm fold, 2e-6 of piece_stats_ref's magnitudes for the row statistics, 3e-3 against the unrounded f32 operands.  Outputs are
prefilled (NaN; 7.0 in the half planes of the head-major cases): every element of the M x N result must be finite afterwards, every
padding column and every skipped lo third must still hold its prefill."""
import pytest
import torch
import torch.nn.functional as F

import gemm_split1_cases as S1
from test_ops_gpu import piece_stats_ref, to_head_major

pytestmark = pytest.mark.gpu

WORST = {}                                                            # (kernel, form, what) -> largest error seen, printed at the end


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    yield h
    for (k, form, what), e in sorted(WORST.items()):
        print(f"split-1 worst error: kernel {k:>4}  {form:<14} {what:<12} {e:.3e}")


def ids(cases):
    return [c.id for c in cases]


def note(case, what, err):
    key = (case.kernel, case.form, what)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"{case.id} {what}: {err:.3e}")
    return err


def relerr(got, ref):
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def run(case, hip, monkeypatch, true_lo=False, **override):
    """Launch the case under its variant; the planner names the kernel the case is about."""
    if case.kernel == "conv":
        monkeypatch.delenv("CVLM_GEMM_VARIANT", raising=False)
    else:
        monkeypatch.setenv("CVLM_GEMM_VARIANT", case.kernel)
    L = S1.launch(case, hip, "cuda", true_lo)
    for name in override.pop("drop", ()):
        L.kw.pop(name)
    prefill = override.pop("prefill_h2", None)
    if prefill is not None:
        L.out_h2.t.fill_(prefill)
    L.kw.update(override)
    assert hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, **L.kw)[0]["kernel"] == S1.KERNELS[case.kernel]
    hip.gemm(L.A, L.W, L.M, L.N, L.K, **L.kw)
    torch.cuda.synchronize()
    return L


def hi64(x):
    return x.hi.float().cpu().double()


def acc64(L):
    """fp64 product of the planes a split-1 launch reads"""
    return hi64(L.A) @ hi64(L.W).t()


def act64(z, act):
    return {0: z, 1: F.gelu(z), 2: z * torch.sigmoid(1.702 * z), 3: F.relu(z)}[act]


def h2_value(t, N, scale):
    """hi + lo of the first N columns of planes [2][M][ld], in the caller's units"""
    return (t[0, :, :N].float() + t[1, :, :N].float()).cpu().double() / scale


def all_finite(t):
    return bool(torch.isfinite(t.float()).all())


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S1.of("product"), ids=ids(S1.of("product")))
def test_product(hip, monkeypatch, case):
    L = run(case, hip, monkeypatch)
    assert all_finite(L.out_f32)
    assert note(case, "f32", relerr(L.out_f32, acc64(L))) < 2e-6         # same fp16 operands, fp32 accumulate
    if case.shape == (300, 264, 1280):                                   # once per kernel: the unrounded operands, fp16-operand accuracy
        assert note(case, "vs_f32_ops", relerr(L.out_f32, L.host.a.double() @ L.host.w.double().t())) < 3e-3


@pytest.mark.parametrize("case", S1.of("plain"), ids=ids(S1.of("plain")))
def test_plain(hip, monkeypatch, case):
    """bias, alpha, activation, f32 residual; f32 and h2 outputs of one launch, tight / padded / odd leading dimensions"""
    L = run(case, hip, monkeypatch)
    N = L.N
    z = act64(S1.ALPHA * acc64(L) + L.host.bias.double(), case.act) + L.host.res[:, :N].double()
    assert all_finite(L.out_f32[:, :N]) and all_finite(L.out_h2.t[:, :, :N])
    assert all_nan(L.out_f32[:, N:]) and all_nan(L.out_h2.t[:, :, N:])  # padding columns keep their prefill
    assert note(case, "f32", relerr(L.out_f32[:, :N], z)) < 3e-6
    assert note(case, "h2", relerr(h2_value(L.out_h2.t, N, S1.OUT_SCALE), z)) < 3e-6


@pytest.mark.parametrize("case", S1.of("batched"), ids=ids(S1.of("batched")))
def test_batched_abs_post(hip, monkeypatch, case):
    """the high-pass filter's form (engine.py, SamEncoder.highpass): one activation against a batch of weights, |residual - product|"""
    L = run(case, hip, monkeypatch)
    Bz, M, N, K = case.shape
    ref = (L.host.res.double() - torch.einsum("mk,bnk->bmn", hi64(L.A), hi64(L.W).reshape(Bz, N, K))).abs()
    assert all_finite(L.out_f32)
    assert note(case, "f32", relerr(L.out_f32, ref)) < 3e-6


@pytest.mark.parametrize("case", S1.of("pixel_shuffle"), ids=ids(S1.of("pixel_shuffle")))
def test_pixel_shuffle(hip, monkeypatch, case):
    """ConvTranspose2d(k = 2, s = 2) as a GEMM whose store scatters (dy, dx, co) columns: against conv_transpose2d of the hi planes"""
    L = run(case, hip, monkeypatch)
    Bn, H, Wd, Cin, Cout = case.shape
    x = hi64(L.A).reshape(Bn, H, Wd, Cin).permute(0, 3, 1, 2)
    wt = hi64(L.W).reshape(2, 2, Cout, Cin).permute(3, 2, 0, 1)
    ref = F.conv_transpose2d(x, wt, L.host.bias.double(), stride=2).permute(0, 2, 3, 1)
    assert all_finite(L.out_f32)
    assert note(case, "f32", relerr(L.out_f32, ref)) < 3e-6


@pytest.mark.parametrize("case", S1.of("head_major"), ids=ids(S1.of("head_major")))
def test_head_major(hip, monkeypatch, case):
    """the bits of to_head_major of the plain h2 launch of the same kernel; lo thirds named in head_major_nolo keep their 7.0"""
    S, hd = case.shape
    Bn, Hh = 2, 2
    P = run(case, hip, monkeypatch, drop=("head_major", "head_major_nolo"), prefill_h2=float("nan"))
    assert all_finite(P.out_h2.t)
    assert note(case, "h2", relerr(h2_value(P.out_h2.t, P.N, 1.0), acc64(P) + P.host.bias.double())) < 3e-6
    L = run(case, hip, monkeypatch)
    assert torch.equal(L.out_h2.t[0], to_head_major(P.out_h2.t[0], Bn, S, Hh, hd))
    want_lo = to_head_major(P.out_h2.t[1], Bn, S, Hh, hd).reshape(3, -1)      # head-major: the thirds are contiguous
    got_lo = L.out_h2.t[1].reshape(3, -1)
    for which in range(3):
        if (case.nolo >> which) & 1:
            assert bool((got_lo[which] == 7.0).all()), which
        else:
            assert torch.equal(got_lo[which], want_lo[which]), which


@pytest.mark.parametrize("case", S1.of("ln_fold"), ids=ids(S1.of("ln_fold")))
def test_ln_fold(hip, monkeypatch, case):
    """the kernel's documented arithmetic, act(alpha * acc * rstd[m] - c[m] * colsum[n] + bias[n]), on arbitrary (rstd, c) and colsum"""
    L = run(case, hip, monkeypatch)
    st = L.host.stats.double()
    z = act64(S1.ALPHA * acc64(L) * st[:, :1] - st[:, 1:] * L.host.colsum.double() + L.host.bias.double(), case.act)
    assert all_finite(L.out_h2.t)
    err = float((h2_value(L.out_h2.t, L.N, S1.OUT_SCALE) - z).abs().max())
    bound = 2e-5 * max(1.0, float(z.abs().max()))
    note(case, "abs/bound", err / bound)
    assert err < bound


@pytest.mark.parametrize("case", S1.of("h2_residual"), ids=ids(S1.of("h2_residual")))
def test_h2_residual_and_row_stats(hip, monkeypatch, case):
    """in place on a residual stream in h2 planes (massive channels, both planes read), piece statistics of the result rows; a second
    launch gives the same bits"""
    L = run(case, hip, monkeypatch)
    stats = L.kw["row_stats"]
    x_ref = S1.ALPHA * acc64(L) + L.host.bias.double() + L.host.x_old.float().double() / S1.XS
    assert all_finite(L.out_h2.t) and not bool(torch.isnan(stats).any())
    assert note(case, "h2", relerr(h2_value(L.out_h2.t, L.N, S1.XS), x_ref)) < 3e-6
    s_ref, s_mag = piece_stats_ref(x_ref)
    assert note(case, "stats", float(((stats.cpu().double() - s_ref).abs() / s_mag).max())) < 2e-6
    again = run(case, hip, monkeypatch)
    assert torch.equal(again.out_h2.t, L.out_h2.t) and torch.equal(again.kw["row_stats"], stats)


@pytest.mark.parametrize("case", S1.of("conv"), ids=ids(S1.of("conv")))
def test_conv3x3(hip, monkeypatch, case):
    """implicit 3x3 convolution on an NHWC image, bias and f32 residual: against conv2d of the hi planes"""
    L = run(case, hip, monkeypatch)
    Bn, H, Wd, Cc, N = case.shape
    xi = hi64(L.A).reshape(Bn, H, Wd, Cc).permute(0, 3, 1, 2)
    wk = hi64(L.W).reshape(N, 3, 3, Cc).permute(0, 3, 1, 2)
    ref = F.conv2d(xi, wk, L.host.bias.double(), padding=1).permute(0, 2, 3, 1).reshape(L.M, N) + L.host.res.double()
    assert all_finite(L.out_f32)
    assert note(case, "f32", relerr(L.out_f32, ref)) < 3e-6


@pytest.mark.parametrize("case", S1.TRUE_LO_CASES, ids=ids(S1.TRUE_LO_CASES))
def test_true_lo_planes_change_no_bit(hip, monkeypatch, case):
    a, b = run(case, hip, monkeypatch), run(case, hip, monkeypatch, true_lo=True)
    assert all_finite(b.A.t) and all_finite(b.W.t) and all_nan(a.A.lo) and all_nan(a.W.lo)
    assert all_finite(a.out_f32) and torch.equal(a.out_f32, b.out_f32)
    if a.out_h2 is not None:
        assert all_finite(a.out_h2.t) and torch.equal(a.out_h2.t, b.out_h2.t)


def test_the_three_plain_kernels_agree(hip, monkeypatch):
    """one case on the three tilings: the same values up to the order of the fp32 sums (4e-6 of |ref|max, the bound the K-split tests
    use between two summation orders)"""
    outs = {k: run(S1.Case(k, "plain", S1.PARITY_SHAPE), hip, monkeypatch) for k in S1.PLAIN_KERNELS}
    L = outs["1"]
    ref_max = float((S1.ALPHA * acc64(L) + L.host.bias.double() + L.host.res.double()).abs().max())
    for x, y in (("1", "2"), ("1", "5"), ("2", "5")):
        d = float((outs[x].out_f32 - outs[y].out_f32).abs().max()) / ref_max
        print(f"kernels {x} / {y}: {d:.3e}")
        assert d < 4e-6, (x, y)
