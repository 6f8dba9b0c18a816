"""Precision `exact` (split = 3) of cvlm_gemm: every gemm_nt_kernel instantiation that exists for split 3, in every launch form the
planner admits on it, against fp64 of the planes it reads (tests/gemm_split3_cases.py holds the cases, the environment that forces
each kernel and why those shapes; tests/test_gemm_split3_cpu.py proves without a GPU that each case reaches the kernel it names).

Operands are H2.pack of N(0, 1) activations and K ** -0.5 weights, both planes real; the reference is fp64 of hi + lo of A and W,
computed on the device once per (form, shape) and shared by every kernel that runs the shape.  Bounds, relative to |ref|max, are the
project's own for the same forms (tests/test_ops_gpu.py): 2e-6 for the bias-free product, 3e-6 for every epilogue form (h2 outputs
after dividing by out_scale), 2e-5 * max(1, |z|max) absolute for the LayerNorm fold, 2e-6 of piece_stats_ref's magnitudes for the row
statistics, 1e-5 against the unrounded f32 operands (once per kernel, at its long-K shape), 4e-6 between two summation orders (K-parts
against whole tiles, one tiling against another).

Every launch starts with hip.gemm_plan and asserts the kernel, the K-parts and the workspace use the case names.  Outputs are
prefilled (NaN; 7.0 in the half planes of the head-major cases): every element of the M x N result must be finite afterwards, every
padding column and every skipped lo third must still hold its prefill, and so must the 8 guard rows allocated behind row M of every
output and of the row-statistics pieces.  A case given a workspace leaves no error word and a zero flag page; it and every in-place
case run twice and give the same bits."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import gemm_split1_cases as S1
import gemm_split3_cases as S3
from test_ops_gpu import piece_stats_ref, to_head_major

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}                                                            # (kernel, form, what) -> largest error seen, printed at the end
ACC = {}                                                              # (form, shape) -> fp64 product of the planes, on the device


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    yield h
    ACC.clear()
    for (k, form, what), e in sorted(WORST.items()):
        print(f"split-3 worst error: kernel {k:>9}  {form:<14} {what:<12} {e:.3e}")


@pytest.fixture(scope="module")
def ws(hip):
    return hip.new_gemm_workspace(DEV)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ids(cases):
    return [c.id for c in cases]


def note(case, what, err):
    key = (case.kernel, case.form, what)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"{case.id} {what}: {err:.3e}")
    return err


def relerr(got, ref):
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30))


def d64(x):
    return x.to(DEV).double()


def planes64(x):
    return x.t[0].double() + x.t[1].double()


def all_finite(t):
    return bool(torch.isfinite(t.float()).all())


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def set_env(monkeypatch, env):
    import os
    for name in [n for n in os.environ if n.startswith("CVLM_GEMM_") and n != "CVLM_GEMM_VARIANT_LIVE"]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def run(case, hip, monkeypatch, ws, cus, drop=(), prefill_h2=None):
    """Launch the case under its environment; the planner names the kernel, the K-parts and the workspace use the case is about.
    Afterwards the guard rows hold their prefill and the workspace, if given, records no error and has a zero flag page."""
    set_env(monkeypatch, case.env)
    L = S3.launch(case, hip, DEV, workspace=ws, cus=cus)
    for name in drop:
        L.kw.pop(name)
    if prefill_h2 is not None:
        L.out_h2.t.fill_(prefill_h2)
        for g in L.guards:
            g.fill_(prefill_h2)
    plan = hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, cus=cus, **L.kw)
    want = S3.expected_plan(L.case, L.M, L.N)
    assert len(plan) == 1 and {k: plan[0][k] for k in want} == want, (case.id, plan, want)
    hip.gemm(L.A, L.W, L.M, L.N, L.K, **L.kw)
    torch.cuda.synchronize()
    fill = 7.0 if case.form == "head_major" and prefill_h2 is None else None
    assert len(L.guards) >= 1 and all(g.numel() > 0 for g in L.guards)
    for i, g in enumerate(L.guards):
        assert bool((g == fill).all()) if fill is not None else all_nan(g), (case.id, "guard rows written", i)
    if case.needs_ws:
        assert hip.gemm_workspace_errors(ws) == 0, case.id
        assert int(ws[:4096].view(torch.int32).abs().sum()) == 0, (case.id, "flag page not back to zero")
    return L


def acc64(L):
    """fp64 product of the planes a split-3 launch reads (hi + lo of A and W); one per (form, shape), whichever kernel runs it"""
    key = (L.case.form, L.case.shape)
    if key not in ACC:
        a, w = planes64(L.planar_A), planes64(L.W)
        f = L.case.form
        if f == "batched":
            Bz, M, N, K = L.case.shape
            ACC[key] = torch.einsum("mk,bnk->bmn", a, w.reshape(Bz, N, K))
        elif f == "pixel_shuffle":
            Bn, H, Wd, Cin, Cout = L.case.shape
            ACC[key] = F.conv_transpose2d(a.reshape(Bn, H, Wd, Cin).permute(0, 3, 1, 2), w.reshape(2, 2, Cout, Cin).permute(3, 2, 0, 1),
                                          None, stride=2).permute(0, 2, 3, 1)
        elif f == "conv":
            Bn, H, Wd, Cc, N = L.case.shape
            ACC[key] = F.conv2d(a.reshape(Bn, H, Wd, Cc).permute(0, 3, 1, 2), w.reshape(N, 3, 3, Cc).permute(0, 3, 1, 2),
                                None, padding=1).permute(0, 2, 3, 1).reshape(L.M, N)
        else:
            ACC[key] = a @ w.t()
    return ACC[key]


def act64(z, act):
    return {0: z, 1: F.gelu(z), 2: z * torch.sigmoid(1.702 * z), 3: F.relu(z)}[act]


def h2_out(L):
    """the h2 output as planes [2][M][columns]: of the planar tensor, or decoded from the image"""
    return L.out_h2.t if L.out_img is None else L.out_img.planes().t


def h2_value(t, N, scale):
    return (t[0, :, :N].double() + t[1, :, :N].double()) / scale


def check_h2_padding(L):
    t = h2_out(L)
    first = L.N if L.out_img is None else L.N + (-L.N) % 32          # an image: nothing written past the last 32-column chunk of N
    assert all_finite(t[:, :, :L.N]) and all_nan(t[:, :, first:]), L.case.id


def expected(L):
    """fp64 value of the form's output"""
    f, c, h = L.case.form, L.case, L.host
    acc = acc64(L)
    if f == "product":
        return acc
    if f == "plain":
        return act64(S1.ALPHA * acc + d64(h.bias), c.act) + d64(h.res)[:, :L.N]
    if f == "batched":
        return (d64(h.res) - acc).abs()
    if f == "pixel_shuffle":
        return acc + d64(h.bias)
    if f == "head_major":
        return acc + d64(h.bias)
    if f == "ln_fold":
        st = d64(h.stats)
        return act64(S1.ALPHA * acc * st[:, :1] - st[:, 1:] * d64(h.colsum) + d64(h.bias), c.act)
    if f == "h2_residual":
        return S1.ALPHA * acc + d64(h.bias) + planes64(h.x_old).to(DEV) / S1.XS
    if f == "conv":
        return acc + d64(h.bias) + d64(h.res)
    raise ValueError(f)


def check(L):
    """every output of the launch against fp64, finite inside, prefill outside"""
    f, c, N = L.case.form, L.case, L.N
    z = expected(L)
    if f in ("product", "batched", "pixel_shuffle", "conv"):
        assert all_finite(L.out_f32), c.id
        assert note(c, "f32", relerr(L.out_f32, z)) < (2e-6 if f == "product" else 3e-6)
        if f == "product" and c.shape[2] >= 1280 and not c.k.il:       # once per kernel: the unrounded operands
            assert note(c, "vs_f32_ops", relerr(L.out_f32, d64(L.host.a) @ d64(L.host.w).t())) < 1e-5
    elif f == "plain":
        if L.out_f32 is not None:
            assert all_finite(L.out_f32[:, :N]) and all_nan(L.out_f32[:, N:]), c.id
            assert note(c, "f32", relerr(L.out_f32[:, :N], z)) < 3e-6
        if L.out_h2 is not None or L.out_img is not None:
            check_h2_padding(L)
            assert note(c, "h2", relerr(h2_value(h2_out(L), N, S1.OUT_SCALE), z)) < 3e-6
    elif f == "ln_fold":
        check_h2_padding(L)
        err = float((h2_value(h2_out(L), N, S1.OUT_SCALE) - z).abs().max())
        bound = 2e-5 * max(1.0, float(z.abs().max()))
        note(c, "abs/bound", err / bound)
        assert err < bound
    elif f == "h2_residual":
        stats = L.kw["row_stats"]
        check_h2_padding(L)
        assert not bool(torch.isnan(stats).any()), c.id
        assert note(c, "h2", relerr(h2_value(h2_out(L), N, S1.XS), z)) < 3e-6
        s_ref, s_mag = piece_stats_ref(z.cpu())
        assert note(c, "stats", float(((stats.cpu().double() - s_ref).abs() / s_mag).max())) < 2e-6
    else:
        raise ValueError(f)


def outputs(L):
    """the bits a launch left: for comparisons between two launches"""
    out = []
    if L.out_f32 is not None:
        out.append(L.out_f32[..., :L.N] if L.case.form == "plain" else L.out_f32)
    if L.out_h2 is not None or L.out_img is not None:
        out.append(h2_out(L)[:, :, :L.N])
    if "row_stats" in L.kw:
        out.append(L.kw["row_stats"])
    return out


def same_bits(a, b):
    x, y = outputs(a), outputs(b)
    return len(x) == len(y) and len(x) > 0 and all(torch.equal(p, q) for p, q in zip(x, y))


def run_checked(case, hip, monkeypatch, ws, cus):
    """run, check against fp64, and where a workspace or an in-place output is involved run again for the same bits"""
    L = run(case, hip, monkeypatch, ws, cus)
    check(L)
    if case.needs_ws or case.form == "h2_residual":
        assert same_bits(run(case, hip, monkeypatch, ws, cus), L), (case.id, "second launch differs")
    return L


def whole_tile_twin(case):
    """the launch of the same problem that runs every tile whole: the 128^2 kernel of the same ring for an SK case (the eight-wave one
    for sk_w8), the same 256^2 kernel without a workspace for a tail case"""
    if case.tail:
        return dataclasses.replace(case, parts=1, tail=False)
    return dataclasses.replace(case, kernel={"sk_r2": "r2", "sk_r3": "r3", "sk_r4": "r4", "sk_w8": "w128"}[case.kernel], parts=1)


def check_k_parts(L, hip, monkeypatch, ws, cus):
    """K-parts against whole tiles: the same values up to the order of the fp32 sums"""
    c = L.case
    if c.parts == 1 or c.k.il or c.form not in ("product", "plain", "h2_residual"):
        return
    Wt = run(whole_tile_twin(c), hip, monkeypatch, ws, cus)
    scale = {"product": 1.0, "plain": S1.OUT_SCALE, "h2_residual": S1.XS}[c.form]
    ref_max = float(expected(L).abs().max())
    if L.out_f32 is not None:
        assert note(c, "vs_whole", float((L.out_f32[..., :L.N] - Wt.out_f32[..., :L.N]).abs().max()) / ref_max) < 4e-6
    if L.out_h2 is not None:
        d = float((h2_value(L.out_h2.t, L.N, scale) - h2_value(Wt.out_h2.t, L.N, scale)).abs().max()) / ref_max
        assert note(c, "vs_whole_h2", d) < 4e-6


PLANAR = [c for c in S3.CASES if not c.k.il]


def planar(*forms):
    return [c for c in PLANAR if c.form in forms]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", planar("product"), ids=ids(planar("product")))
def test_product(hip, monkeypatch, ws, cus, case):
    check_k_parts(run_checked(case, hip, monkeypatch, ws, cus), hip, monkeypatch, ws, cus)


@pytest.mark.parametrize("case", planar("plain"), ids=ids(planar("plain")))
def test_plain(hip, monkeypatch, ws, cus, case):
    """bias, alpha, activation, f32 residual; f32 and h2 outputs of one launch (or one of them), tight / padded / odd leading dimensions"""
    check_k_parts(run_checked(case, hip, monkeypatch, ws, cus), hip, monkeypatch, ws, cus)


@pytest.mark.parametrize("case", planar("batched", "pixel_shuffle", "conv"), ids=ids(planar("batched", "pixel_shuffle", "conv")))
def test_batched_pixel_shuffle_conv(hip, monkeypatch, ws, cus, case):
    """batched |residual - product| (the high-pass filter's form); ConvTranspose2d(k = 2, s = 2) as a GEMM whose store scatters (dy, dx,
    co) columns, against conv_transpose2d; the implicit 3 x 3 convolution on an NHWC image, against conv2d"""
    run_checked(case, hip, monkeypatch, ws, cus)


@pytest.mark.parametrize("case", planar("head_major"), ids=ids(planar("head_major")))
def test_head_major(hip, monkeypatch, ws, cus, case):
    """the plain h2 launch of the same kernel against fp64, then the bits of its to_head_major; lo thirds named in head_major_nolo keep
    their 7.0"""
    P = run(case, hip, monkeypatch, ws, cus, drop=("head_major", "head_major_nolo"), prefill_h2=float("nan"))
    c = P.case
    S, hd = c.shape[:2]
    Bn, Hh = P.M // S, P.N // (3 * hd)
    assert all_finite(P.out_h2.t)
    assert note(c, "h2", relerr(h2_value(P.out_h2.t, P.N, 1.0), expected(P))) < 3e-6
    L = run(case, hip, monkeypatch, ws, cus)
    assert torch.equal(L.out_h2.t[0], to_head_major(P.out_h2.t[0], Bn, S, Hh, hd))
    want_lo = to_head_major(P.out_h2.t[1], Bn, S, Hh, hd).reshape(3, -1)      # head-major: the thirds are contiguous
    got_lo = L.out_h2.t[1].reshape(3, -1)
    for which in range(3):
        if (c.nolo >> which) & 1:
            assert bool((got_lo[which] == 7.0).all()), which
        else:
            assert torch.equal(got_lo[which], want_lo[which]), which


@pytest.mark.parametrize("case", planar("ln_fold"), ids=ids(planar("ln_fold")))
def test_ln_fold(hip, monkeypatch, ws, cus, case):
    """the kernel's documented arithmetic, act(alpha * acc * rstd[m] - c[m] * colsum[n] + bias[n]), on arbitrary (rstd, c) and colsum"""
    run_checked(case, hip, monkeypatch, ws, cus)


@pytest.mark.parametrize("case", planar("h2_residual"), ids=ids(planar("h2_residual")))
def test_h2_residual_and_row_stats(hip, monkeypatch, ws, cus, case):
    """in place on a residual stream in h2 planes (massive channels, both planes read), piece statistics of the result rows; a second
    launch gives the same bits"""
    check_k_parts(run_checked(case, hip, monkeypatch, ws, cus), hip, monkeypatch, ws, cus)


IMAGE = [c for c in S3.CASES if c.k.il]


@pytest.mark.parametrize("case", IMAGE, ids=ids(IMAGE))
def test_image_twins(hip, monkeypatch, ws, cus, case):
    """the kernels that stage the weight (and the activation) from 128-byte-row images: the value against fp64 and the bits of the
    planar launch of the same form on the planar kernel; an image output has nothing past the last 32-column chunk of N"""
    if case.form == "head_major":
        L = run(case, hip, monkeypatch, ws, cus)
        P = run(S3.planar_twin(case), hip, monkeypatch, ws, cus)
        plain = run(S3.planar_twin(case), hip, monkeypatch, ws, cus, drop=("head_major", "head_major_nolo"), prefill_h2=float("nan"))
        assert note(case, "h2", relerr(h2_value(plain.out_h2.t, plain.N, 1.0), expected(plain))) < 3e-6
        S, hd = L.case.shape[:2]
        assert torch.equal(P.out_h2.t[0], to_head_major(plain.out_h2.t[0], L.M // S, S, L.N // (3 * hd), hd))
        assert torch.equal(L.out_h2.t, P.out_h2.t)
        return
    L = run_checked(case, hip, monkeypatch, ws, cus)
    P = run(S3.planar_twin(case), hip, monkeypatch, ws, cus)
    assert same_bits(L, P), (case.id, "image launch differs from the planar launch")


# ---------------------------------------------------------------------------------------------
def test_kernels_of_a_tiling_agree(hip, monkeypatch, ws, cus):
    """One plain launch on every one-workgroup-per-tile kernel that takes it: ring depths, wave forms, planar or image operands give the
    same bits within a tiling (same K-tile order); two tilings agree up to the order of the fp32 sums (4e-6 of |ref|max)."""
    outs = {}
    for c in S3.PARITY_CASES:
        L = run(c, hip, monkeypatch, ws, cus)
        outs.setdefault(c.k.tiling, []).append(L)
    assert set(outs) == {"128x128", "64x128", "256x128", "256x256"}
    ref_max = float(expected(outs["128x128"][0]).abs().max())
    for tiling, ls in outs.items():
        assert len(ls) >= 3
        for L in ls[1:]:
            assert same_bits(L, ls[0]), (tiling, L.case.id, ls[0].case.id)
    firsts = [ls[0] for ls in outs.values()]
    for i, x in enumerate(firsts):
        for y in firsts[i + 1:]:
            d = float((x.out_f32 - y.out_f32).abs().max()) / ref_max
            print(f"tilings {x.case.k.tiling} / {y.case.k.tiling}: {d:.3e}")
            assert d < 4e-6, (x.case.id, y.case.id)


@pytest.mark.parametrize("form", ["plain", "ln_fold", "h2_residual"])
def test_persistent_equals_one_pass(hip, monkeypatch, ws, cus, form):
    """more tiles than CUs: the persistent kernel, its image twin and the one-pass kernel of the same epilogue give the same bits
    (the first of them is held to fp64 here; test_plain, test_ln_fold and test_h2_residual_and_row_stats hold each kernel on its own)"""
    ls = [run(c, hip, monkeypatch, ws, cus) for c in S3.PERSIST_PARITY[form]]
    check(ls[0])
    for L in ls[1:]:
        assert same_bits(L, ls[0]), (L.case.id, ls[0].case.id)


def test_192_row_tiles_agree(hip, monkeypatch, ws, cus):
    """192 x 256 tiles, planar and image operands: the same bits; against the 256-row tiling of the same epilogue 4e-6 of |ref|max"""
    ls = [run(c, hip, monkeypatch, ws, cus) for c in S3.T192_PARITY]
    check(ls[0])
    assert [L.case.kernel for L in ls] == ["t192", "t192-w", "t192-wa", "e2"]
    for L in ls[1:3]:
        assert same_bits(L, ls[0]), L.case.id
    ref_max = float(expected(ls[0]).abs().max())
    d = float((h2_value(ls[0].out_h2.t, ls[0].N, S1.XS) - h2_value(ls[3].out_h2.t, ls[3].N, S1.XS)).abs().max()) / ref_max
    print(f"tilings 192x256 / 256x256: {d:.3e} (same bits: {same_bits(ls[0], ls[3])})")
    assert d < 4e-6
