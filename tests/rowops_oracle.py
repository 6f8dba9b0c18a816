"""Plain torch / numpy restatements of the row kernels of csrc/rowops.hip, for tests/test_rowops_cpu.py (which checks them against
torch's own operators) and tests/test_rowops_edges_gpu.py (which holds the kernels to them).  CPU only; nothing here touches a device.

Arithmetic references are fp64.  Where an operation is a copy or one f32 rounding per element the reference is the same expression in
torch float32 (IEEE, correctly rounded), so the comparison is bit for bit."""
import math

import numpy as np
import torch

TINY = 1e-30


# ---- error measures ----------------------------------------------------------------------------------------------------------------
def rowerrs(got: torch.Tensor, ref: torch.Tensor, row_dims: int = 1) -> torch.Tensor:
    """Per row: max |got - ref| over the row / max(max |ref| over the row, TINY).  The last `row_dims` axes form a row."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    lead = ref.shape[:ref.dim() - row_dims]
    g = got.detach().cpu().double().reshape(int(np.prod(lead)) if lead else 1, -1)
    r = ref.detach().cpu().double().reshape(g.shape)
    return (g - r).abs().amax(1) / r.abs().amax(1).clamp_min(TINY)


def rowerr(got: torch.Tensor, ref: torch.Tensor, row_dims: int = 1) -> float:
    """The worst row of rowerrs.  NaN anywhere in `got` gives NaN, which fails every `<` comparison."""
    e = rowerrs(got, ref, row_dims)
    return float("nan") if bool(torch.isnan(e).any()) else float(e.max())


def globalerr(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Max error over the whole tensor / max of the whole reference: the measure of tests/test_ops_gpu.py (relerr)."""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + TINY))


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns as integers (distinguishes -0 from +0, compares NaNs)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def activation(z: torch.Tensor, act: int) -> torch.Tensor:
    """The activation codes of include/cvlm.h on fp64 values: 0 none, 1 exact-erf GELU, 2 x * sigmoid(1.702 x), 3 ReLU."""
    if act == 0:
        return z
    if act == 1:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == 2:
        return z / (1.0 + torch.exp(-1.702 * z))
    if act == 3:
        return z.clamp_min(0.0)
    raise ValueError(act)


def layernorm(x, gamma, beta, eps, add=None, act=0):
    """fp64: s = x + add[row % add_rows]; y = act((s - mean) / sqrt(biased var + eps) * gamma + beta).  Returns (s, y, r) with
    r = |mean| / sqrt(var + eps) per row: what an fp32 mean's rounding is multiplied by on its way to the output."""
    s = x.double()
    if add is not None:
        s = s + add.double()[torch.arange(s.shape[0]) % add.shape[0]]
    mu = s.sum(1, keepdim=True) / s.shape[1]
    d = s - mu
    var = (d * d).sum(1, keepdim=True) / s.shape[1]
    rstd = 1.0 / torch.sqrt(var + eps)
    y = activation(d * rstd * gamma.double() + beta.double(), act)
    return s, y, (mu.abs() * rstd)[:, 0]


def layernorm_tolerance(r: torch.Tensor) -> torch.Tensor:
    """Per-row bound on rowerr: the project's 3e-6 plus four times the rounding 2^-24 |mean| of an fp32 mean as the output sees it."""
    return 3e-6 + 4.0 * 2.0 ** -24 * r


LN_FAMILIES = ("normal", "tiny", "huge", "offset100", "offset-30", "constant", "zero", "outlier")


def layernorm_rows(M: int, D: int, seed: int, shift: int = 0) -> torch.Tensor:
    """f32 [M][D]: row m belongs to family LN_FAMILIES[(m + shift) % 8], so that one tensor mixes rows whose errors a per-tensor
    measure would hide behind one another."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g, dtype=torch.float32)
    for m in range(M):
        fam = LN_FAMILIES[(m + shift) % len(LN_FAMILIES)]
        if fam == "tiny":
            x[m] *= 1e-4                                              # variance 1e-8: eps dominates
        elif fam == "huge":
            x[m] *= 1e4
        elif fam == "offset100":
            x[m] += 100.0
        elif fam == "offset-30":
            x[m] = x[m] * 0.3 - 30.0
        elif fam == "constant":
            x[m] = 0.1                                                # no short binary fraction: the fp32 sum of D copies rounds
        elif fam == "zero":
            x[m] = 0.0
        elif fam == "outlier":
            x[m, (7 * m + 3) % D] = 1e4
    return x


# ---- f32 expressions with one rounding per element ----------------------------------------------------------------------------------
def add_rows_f32(a, b, scale):
    """(a + b[row % b_rows]) * scale in float32, the add rounded before the product."""
    t = a.float()
    if b is not None:
        t = t + b.float()[torch.arange(a.shape[0]) % b.shape[0]]
    return t * torch.tensor(scale, dtype=torch.float32)


def patchify(src0, src1, p: int, ldk: int):
    """f32 [B * gh * gw][ldk]: row (b, py, px), column c * p * p + iy * p + ix over the channels of src0 then src1, zeros from K on."""
    src = src0 if src1 is None else torch.cat([src0, src1], 1)
    B, Cc, H, W = src.shape
    gh, gw = H // p, W // p
    out = torch.zeros(B, gh, gw, ldk, dtype=torch.float32)
    for py in range(gh):
        for px in range(gw):
            out[:, py, px, :Cc * p * p] = src[:, :, py * p:(py + 1) * p, px * p:(px + 1) * p].reshape(B, -1)
    return out.reshape(B * gh * gw, ldk)


def im2col3x3(x):
    """x f32 [B][H][W][C] -> [B * H * W][9 * C]: column (ky * 3 + kx) * C + c = x[b][y + ky - 1][x + kx - 1][c], zero outside."""
    B, H, W, Cc = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cc, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    taps = [xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 3).reshape(B * H * W, 9 * Cc)


def reinterpret_transpose(x, B: int, T: int, D: int, scale: float):
    """out[b][t][c] = x.flat[b][c * T + t] * scale (f32, one rounding)."""
    return (x.reshape(B, D, T).permute(0, 2, 1) * torch.tensor(scale, dtype=torch.float32)).reshape(B * T, D).contiguous()


def clip_assemble(patches, cls, pos, ctx, nctx: int):
    """[B][1 + P + nctx][W] = [cls + pos[0] | patches + pos[1:] | ctx[:nctx]] in float32."""
    B, P, W = patches.shape
    tok = torch.cat([cls.reshape(1, 1, W).expand(B, 1, W), patches], 1) + pos[:1 + P]
    return torch.cat([tok, ctx[:nctx].reshape(1, nctx, W).expand(B, nctx, W)], 1).contiguous()


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------
def dense_pe(gauss, size: int):
    """gauss [2][C / 2] -> fp64 [size * size][C]: row y * size + x = [sin | cos](2 pi ((2 cx - 1) g0 + (2 cy - 1) g1)), c = (i + .5) / size."""
    g = gauss.double()
    c = (torch.arange(size, dtype=torch.float64) + 0.5) / size
    cx = (2 * c - 1).reshape(1, size, 1)
    cy = (2 * c - 1).reshape(size, 1, 1)
    v = 2 * math.pi * (cx * g[0] + cy * g[1])
    return torch.cat([v.sin(), v.cos()], -1).reshape(size * size, -1)


def mask_head(up, edge, hyper):
    """up, edge [B][HW][C], hyper [B][5][C] -> fp64 [B][HW]: m = hyper[b][0] . up; with edge: m * sigmoid(hyper[b][4] . edge) + m."""
    m = torch.einsum("bpc,bc->bp", up.double(), hyper.double()[:, 0])
    if edge is None:
        return m
    g = torch.einsum("bpc,bc->bp", edge.double(), hyper.double()[:, 4])
    return m / (1.0 + torch.exp(-g)) + m


def bilinear_axis(n_in: int, n_out: int):
    """Source rows and weight of F.interpolate(mode="bilinear", align_corners=False) on float32 tensors: coordinates in float32, every
    operation rounded.  Returns (i0, i1, lam) as int64, int64, float32 arrays of n_out entries."""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    src = scale * (o + np.float32(0.5)) - np.float32(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, np.float32(0.0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0.astype(np.float32)


def bilinear(x, hout: int, wout: int, sigmoid_in: bool = False):
    """x [N][hin][win] -> fp64 [N][hout][wout]: float32 coordinates and weights (bilinear_axis), the blend in fp64."""
    v = x.double()
    if sigmoid_in:
        v = 1.0 / (1.0 + torch.exp(-v))
    y0, y1, ly = bilinear_axis(x.shape[1], hout)
    x0, x1, lx = bilinear_axis(x.shape[2], wout)
    y0, y1, x0, x1 = (torch.from_numpy(i) for i in (y0, y1, x0, x1))
    ly = torch.from_numpy(ly.astype(np.float64)).reshape(1, hout, 1)
    lx = torch.from_numpy(lx.astype(np.float64)).reshape(1, 1, wout)
    top = (1 - lx) * v[:, y0][:, :, x0] + lx * v[:, y0][:, :, x1]
    bot = (1 - lx) * v[:, y1][:, :, x0] + lx * v[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def clip_head(img, txt, lscale: float):
    """fp64: (img / |img|, lscale * (img / |img|) . txt^T)."""
    n = img.double() / img.double().pow(2).sum(1, keepdim=True).sqrt()
    return n, lscale * (n @ txt.double().t())


def normalize_add(x, add):
    n = x.double() / x.double().pow(2).sum(1, keepdim=True).sqrt()
    return n if add is None else n + add.double()


def small_attention(q, k, v, heads: int, hd: int):
    """q [B][nq][heads * hd], k / v [B][nk][heads * hd] -> fp64 [B][nq][heads * hd]: per head softmax(q . k / sqrt(hd)) v, the softmax
    written out (max, exp, sum) one key after the other's weight."""
    B, nq, _ = q.shape
    out = torch.zeros(B, nq, heads * hd, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = torch.einsum("bqd,bkd->bqk", q.double()[..., sl], k.double()[..., sl]) / math.sqrt(hd)
        w = torch.exp(s - s.amax(2, keepdim=True))
        out[..., sl] = torch.einsum("bqk,bkd->bqd", w, v.double()[..., sl]) / w.sum(2, keepdim=True)
    return out


# ---- values that try the f32 -> (hi, lo) split ------------------------------------------------------------------------------------------
def split_adversaries() -> torch.Tensor:
    """f32 values on and next to the rounding boundaries of fp16: exact midpoints between neighbouring fp16 values (ties to an even and
    to an odd mantissa) and their f32 neighbours at several exponents, the same around the smallest normal 2^-14, 2^-24 (the smallest
    fp16 subnormal), 2^-25 (half of it: a tie with zero), +-0 and +-65504.  |v| <= 65504, no f32 subnormal."""
    vals = [0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -24, -2.0 ** -25]
    out = [torch.tensor(vals, dtype=torch.float32)]
    inf = torch.tensor(float("inf"))
    for e in (-14, -10, -3, 0, 5, 14):
        for k in (0, 1, 2, 511, 512, 1021, 1022):
            h = 2.0 ** e * (1.0 + k / 1024.0)
            mid = torch.tensor([h + 2.0 ** (e - 11)], dtype=torch.float32)          # halfway to the next fp16 value: exact in f32
            for base in (mid, torch.tensor([h], dtype=torch.float32)):
                trio = torch.cat([torch.nextafter(base, -inf), base, torch.nextafter(base, inf)])
                out += [trio, -trio]
    below = torch.tensor([2.0 ** -14], dtype=torch.float32)
    out.append(torch.cat([torch.nextafter(below, -inf), torch.nextafter(below, inf)]))
    v = torch.cat(out)
    return v[v.abs() <= 65504.0]
