"""fp64 emulation of the attention kernels' rounding points (include/cvlm.h, cvlm_attn_args; csrc/attention*.hip), importable without a GPU.

The operands are the fp16 planes the kernels read (hi, lo as H2.pack makes them).  Per product the emulation takes exactly the terms the
kernel multiplies, and rounds where the kernel rounds:
  q.k^T  "full"       (q_hi + q_lo).(k_hi + k_lo) * scale          split_qk 3 (three products: fp32-grade, taken as exact)
         "qhi_kfull"  fp16(q * scale).(k_hi + k_lo)                 (2, 2) on the ViT-H kernels: Q's hi plane with `scale` folded in
         "qhi_khi"    fp16(q * scale).k_hi                          (1, 2) on the ViT-H kernels: one MFMA per k-step
         "hihi"       (q_hi.k_hi) * scale                           split_qk 1 on the generic kernel (scale applied to the fp32 score)
  scores: + the rel-pos bias (three-term products everywhere: exact here), rounded to fp32 once
  P.v    "full"       softmax . (v_hi + v_lo)                       split_pv 3 (P as hi + exact remainder)
         "rn"         fp16_rn(e) . (v_hi + v_lo) / sum fp16_rn(e)   (2, 2) / (1, 2) on the ViT-H kernels: the denominator from the rounded P
         "rtz_vhi"    fp16_rz(e) . v_hi / sum e                     split_pv 1 on the generic kernel (cvt_pkrtz; the sum from the fp32 e)
with e = exp(s - max s) -- or, as the kernels form it (`online`): e = 2^fma(s, log2e, fp32(-m * log2e)) in fp32 against the reference
point m of the key's tile, the running maximum over key tiles of `tile` keys that moves only by more than `tau` (the lazy reference point
of csrc/attention.hip and attention_win2.hip, TAU = 5; the g64pp kernels move it on every new maximum: tau = 0).  That reference decides
which small probabilities fall into fp16's subnormal range, and the fp32 exponent argument carries |m| * 2^-24 of error common to a tile:
both matter once |s| reaches tens.  (The wave-uniform ballot of the lazy kernels is taken per query.)  Everything else is fp64.
"""
import numpy as np
import torch

GENERIC, VITH = "generic", "vith"
LOG2E32 = float(np.float32(1.4426950408889634))


def h16(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest fp16 (ties to even, subnormals kept), back in fp64."""
    return torch.from_numpy(x.double().numpy().astype(np.float16).astype(np.float64))


def rz16(x: torch.Tensor) -> torch.Tensor:
    """Round toward zero to fp16 (v_cvt_pkrtz_f16_f32), back in fp64."""
    a = x.double().numpy()
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(a)
    h[over] = np.nextafter(h[over], np.float16(0))
    return torch.from_numpy(h.astype(np.float64))


def pack(x: torch.Tensor):
    """hi = fp16(x), lo = fp16(x - hi): hip.H2.pack's planes, as fp64."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.double(), lo.double()


def rounding(kernel: str, split) -> tuple:
    """(q.k^T form, P.v form) of a split on a kernel family: VITH = the g64pp / win2 kernels (include/cvlm.h ABI 11 / 12), GENERIC = the
    kernel of csrc/attention.hip, which runs (2, 2) and (1, 2) as (3, 3)."""
    sq, sp = split
    if kernel == VITH and split in ((2, 2), (1, 2)):
        return ("qhi_kfull" if sq == 2 else "qhi_khi"), "rn"
    if split in ((2, 2), (1, 2), (3, 3)):
        return "full", "full"
    return ("full" if sq == 3 else "hihi"), ("full" if sp == 3 else "rtz_vhi")


def f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().double()


def reference_points(s: torch.Tensor, tile: int, tau: float) -> torch.Tensor:
    """Per key: the reference point of the online softmax when the key's tile is processed (rows x keys)."""
    R, Sk = s.shape
    nt = -(-Sk // tile)
    sp = torch.full((R, nt * tile), float("-inf"), dtype=s.dtype)
    sp[:, :Sk] = s
    tm = sp.view(R, nt, tile).amax(-1)
    if tau <= 0:
        ref = torch.cummax(tm, dim=1).values
    else:
        ref = torch.empty_like(tm)
        m = torch.full((R,), float("-inf"), dtype=s.dtype)
        for t in range(nt):
            m = torch.where(tm[:, t] > m + tau, torch.maximum(m, tm[:, t]), m)
            ref[:, t] = m
    return ref.repeat_interleave(tile, dim=1)[:, :Sk]


def emulate(q, k, v, scale, *, bias=None, causal=False, qk="full", pv="full", f32_scores=True, online=None, rows=None, chunk=1024,
            stats=None):
    """q, k, v: (hi, lo) fp64 plane pairs of shape (N, S, hd) (queries and keys may differ in S); bias: (N, Sq, Sk) fp64 or a callable
    (n, query indices) -> bias rows; online: (tile, tau) of the kernel's online softmax, None = exact maximum and exp in fp64;
    rows: the query indices to compute (default all).  Returns the (N, len(rows), hd) output in fp64.
    stats (a dict): filled with the score std, max |s| and the mean entropy / ln(keys seen) of the rows -- the regime's description."""
    qh, ql = q
    kh, kl = k
    vh, vl = v
    N, Sk = qh.shape[0], kh.shape[1]
    rows = torch.arange(qh.shape[1]) if rows is None else rows
    Sq = len(rows)
    out = torch.empty(N, Sq, vh.shape[-1], dtype=torch.float64)
    kf, vf = kh + kl, vh + vl
    acc = {"n": 0, "s1": 0.0, "s2": 0.0, "max": 0.0, "ent": 0.0}
    for n in range(N):
        for r0 in range(0, Sq, chunk):
            r1 = min(Sq, r0 + chunk)
            ri = rows[r0:r1]
            qf = qh[n, ri] + ql[n, ri]
            if qk == "full":
                s = (qf @ kf[n].T) * scale
            elif qk == "qhi_kfull":
                s = h16(qf * scale) @ kf[n].T
            elif qk == "qhi_khi":
                s = h16(qf * scale) @ kh[n].T
            elif qk == "hihi":
                s = (qh[n, ri] @ kh[n].T) * scale
            else:
                raise ValueError(qk)
            if bias is not None:
                s = s + (bias(n, ri) if callable(bias) else bias[n, ri])
            if f32_scores:
                s = s.float().double()
            if causal:
                s = s.masked_fill(torch.arange(Sk)[None, :] > ri[:, None], float("-inf"))
            M = s.amax(-1, keepdim=True)
            if online is None:
                e, w = torch.exp(s - M), 1.0
            else:
                ref = reference_points(s, *online)
                ref = torch.where(torch.isfinite(ref), ref, M)
                e = torch.exp2(f32(s * LOG2E32 + f32(-ref * LOG2E32)))
                w = torch.exp(ref - M)                               # the rescale factors: fp32 in the kernels, exact here
            if stats is not None:
                fin = torch.isfinite(s)
                sv = s[fin]
                acc["n"] += sv.numel(); acc["s1"] += float(sv.sum()); acc["s2"] += float((sv * sv).sum())
                acc["max"] = max(acc["max"], float(sv.abs().max()))
                p = e * w / (e * w).sum(-1, keepdim=True)
                ent = -(p * torch.log(p.clamp_min(1e-300))).sum(-1)
                nk = fin.sum(-1).double()
                acc["ent"] += float(torch.where(nk > 1, ent / torch.log(nk.clamp_min(2)), torch.ones_like(ent)).sum())
            if pv == "full":
                o = ((e * w) @ vf[n]) / (e * w).sum(-1, keepdim=True)
            elif pv == "rn":
                e = h16(e) * w
                o = (e @ vf[n]) / e.sum(-1, keepdim=True)
            elif pv == "rtz_vhi":
                o = ((rz16(e) * w) @ vh[n]) / (e * w).sum(-1, keepdim=True)
            else:
                raise ValueError(pv)
            out[n, r0:r1] = o
    if stats is not None:
        mean = acc["s1"] / acc["n"]
        stats.update(score_std=(acc["s2"] / acc["n"] - mean * mean) ** 0.5, max_abs_score=acc["max"], entropy_ratio=acc["ent"] / (N * Sq))
    return out


def relerr(got, ref) -> float:
    ref = ref.double()
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30))
