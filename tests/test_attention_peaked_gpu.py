"""The attention kernels on PEAKED softmaxes, against fp64 and against a CPU emulation of each split's rounding points (tests/attn_emulate.py).

tests/test_ops_gpu.py builds every operand with N(0, 1): scores of std 1, a nearly uniform softmax over thousands of keys, and rounding
noise that averages away.  Trained checkpoints concentrate a query's weight on few keys; there the lazy reference point of the online
softmax (TAU = 5 in csrc/attention.hip and attention_win2.hip) and the per-score rounding of the lossy splits stop averaging.  Three
families of operands, all built from the packed planes the kernels read:
  gauss  q, k scaled so that the score std is sigma (rel-pos bias about 0.3 sigma);
  peak   one key Delta above the rest for every query, in the first key tile, in the last one, or (windows) on the pad keys;
  ramp   a key-index term: +1 per 64-key tile (P grows towards e^TAU before one rescale), +6 per tile (a rescale every tile), +6 per tile
         for half of the queries of every 32-query group only (lanes rescale whose own max did not move), and a descending ramp.
Operands, the fp64 side and the bound live in tests/attn_cases.py, shared with tests/test_attention_edges_gpu.py.
Bound per case: err_kernel <= K_EMU * err_emulated + FLOOR (relative to max |reference|), with the emulation of THAT split on the same
operands; and, for the lossy ViT-H kernels, err_kernel > LOSSY_MIN * err_emulated (a silent fall-back to (3, 3) fails).  Every output row
is written (the output starts as NaN).  SPLIT_TOL of tests/test_ops_gpu.py is the flat regime's bar and is not used here.
"""
import math

import pytest
import torch

import attn_emulate as E
from attn_cases import (G64PAIR, G96PP, GENERIC64, SPLITS, WIN2, _fid, _gen, check, cpu_side, emulations, form_of, make_qkv, planes_bhsd,
                        relpos_rows, sampled_rows, sigma_of, to_head_major, unwindow, windows)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
GAUSS = [("gauss", s) for s in (1, 3, 6, 10)]
PEAK = [("peak", d, w) for d in (12, 25) for w in ("first", "last")]
RAMP = [("ramp", r) for r in ("slow", "fast", "half", "desc")]

MODE1 =([(20, f) for f in GAUSS + PEAK + RAMP] + [(64, f) for f in GAUSS + PEAK + RAMP] +
         [(96, f) for f in [("gauss", 1), ("gauss", 6)] + PEAK])


@pytest.mark.gpu
@pytest.mark.parametrize("G,fam", MODE1, ids=[f"G{G}-{_fid(f)}" for G, f in MODE1])
def test_global_relpos_peaked(hip, G, fam):
    """Mode 1: G = 64 / 96 take the g64pp kernels for (3, 3), (2, 2), (1, 2) and the generic kernel for (3, 1), (1, 1); G = 20 the generic
    kernel for every split."""
    Bn, Hh, hd = (2, 2, 80) if G == 20 else (1, 1, 80)
    D, S = Hh * hd, G * G
    splits = SPLITS if G != 96 else [(3, 3), (2, 2), (1, 2)]
    kernel_of = lambda sp: ((G64PAIR if G == 64 else G96PP) if (G in (64, 96) and sp in ((3, 3), (2, 2), (1, 2))) else GENERIC64)
    qkv, rstd = make_qkv(fam, Bn, S, Hh, hd, seed=100 + G)
    g = _gen(200 + G)
    rel_h, rel_w = torch.randn(2 * G - 1, hd, generator=g) * rstd, torch.randn(2 * G - 1, hd, generator=g) * rstd
    Q, RH, RW = hip.H2.pack(qkv), hip.H2.pack(rel_h), hip.H2.pack(rel_w)

    def build():
        q, k, v = (planes_bhsd(Q, w, Bn, S, Hh, hd) for w in range(3))
        bias = relpos_rows(q[0] + q[1], RH.float().double(), RW.float().double(), G)
        return emulations((q, k, v, bias, False, 1.0), kernel_of, splits, rows)
    rows = sampled_rows(S)
    res = cpu_side(("mode1", G, fam), build)
    Qd = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)]).cuda())
    for sp in splits:
        out = hip.H2.empty(Bn * S, D)
        out.t.fill_(float("nan"))
        hip.attention(Qd, out, Bn, S, Hh, hd, mode=1, grid=G, rel_h=hip.H2(RH.t.cuda()), rel_w=hip.H2(RW.t.cuda()), split_qk=sp[0],
                      split_pv=sp[1], scale=1.0, head_major=True)
        got = out.float().cpu().double().reshape(Bn, S, Hh, hd).permute(0, 2, 1, 3).reshape(Bn * Hh, S, hd)
        assert not torch.isnan(got).any()
        got = got[:, rows]
        check(f"mode 1 G={G} {_fid(fam)} {sp}", got, res, form_of(kernel_of, sp), kernel_of(sp)[0] == E.VITH and sp != (3, 3))


WPEAK = PEAK + [("peak", d, "pad") for d in (12, 25)]
MODE2 = ([(14, 20, f) for f in GAUSS + WPEAK + RAMP] + [(14, 64, f) for f in GAUSS + WPEAK + RAMP] +
         [(w, 20, f) for w in (8, 12) for f in GAUSS + WPEAK[::2] + RAMP])


@pytest.mark.gpu
@pytest.mark.parametrize("ws,G,fam", MODE2, ids=[f"w{w}-G{G}-{_fid(f)}" for w, G, f in MODE2])
def test_window_relpos_peaked(hip, ws, G, fam):
    """Mode 2: window 14 takes win2 for (3, 3), (2, 2), (1, 2) (padded windows on G = 20 and 64), the generic kernel with 7 waves for (3, 1),
    (1, 1); windows 8 (4 waves) and 12 (7 waves) the generic kernel for every split.
    Bn = 2, two heads: at most 100 pairs, one per workgroup of win2; tests/test_attention_window_pairs_gpu.py is where pairs follow each other."""
    Bn, Hh, hd = 2, 2, 80
    D, S = Hh * hd, G * G
    kernel_of = lambda sp: WIN2 if (ws == 14 and sp in ((3, 3), (2, 2), (1, 2))) else GENERIC64
    qkv, rstd = make_qkv(fam, Bn, S, Hh, hd, seed=300 + G + ws, window=ws, G=G)
    g = _gen(400 + G + ws)
    a = 1.0 / hd ** 0.25
    pad = torch.randn(3, Hh, hd, generator=g, dtype=torch.float64) * a
    if fam[0] == "peak":
        pad[0, :, 0] = 1.0
        pad[1, :, 0] = fam[1] if fam[-1] == "pad" else 0.0
    if fam[0] == "ramp":
        pad[0, :, 0], pad[1, :, 0] = 1.0, 0.0
    pad = pad.reshape(3 * D).float()
    rel_h, rel_w = torch.randn(2 * ws - 1, hd, generator=g) * rstd, torch.randn(2 * ws - 1, hd, generator=g) * rstd
    Q, P, RH, RW = hip.H2.pack(qkv), hip.H2.pack(pad), hip.H2.pack(rel_h), hip.H2.pack(rel_w)

    def build():
        q, k, v = (windows(Q, P, Bn, G, ws, Hh, hd, w) for w in range(3))
        bias = relpos_rows(q[0] + q[1], RH.float().double(), RW.float().double(), ws)
        return emulations((q, k, v, bias, False, 1.0), kernel_of, SPLITS)
    res = cpu_side(("mode2", ws, G, fam), build)
    Qd = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)]).cuda())
    for sp in SPLITS:
        out = hip.H2.empty(Bn * S, D)
        out.t.fill_(float("nan"))
        hip.attention(Qd, out, Bn, S, Hh, hd, mode=2, grid=G, window=ws, pad=hip.H2(P.t.cuda()), rel_h=hip.H2(RH.t.cuda()),
                      rel_w=hip.H2(RW.t.cuda()), split_qk=sp[0], split_pv=sp[1], scale=1.0, head_major=True)
        got = out.float().cpu().double()
        form = form_of(kernel_of, sp)
        r = {"ref": unwindow(res["ref"], Bn, G, ws, Hh, hd), form: unwindow(res[form], Bn, G, ws, Hh, hd), "stats": res["stats"]}
        check(f"mode 2 w={ws} G={G} {_fid(fam)} {sp}", got[None], {k: (v[None] if k != "stats" else v) for k, v in r.items()}, form,
              kernel_of(sp)[0] == E.VITH and sp != (3, 3))


MODE0 = [(S, c, f) for S in (577, 77) for c in (False, True) for f in GAUSS + PEAK + RAMP[:2] + RAMP[3:]]
MODE0_SPLITS = [(3, 3), (1, 2), (3, 1), (1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,causal,fam", MODE0, ids=[f"S{S}-{'causal' if c else 'full'}-{_fid(f)}" for S, c, f in MODE0])
def test_plain_peaked(hip, S, causal, fam):
    """Mode 0 (the CLIP towers, hd 64, generic kernel): (1, 2) runs as (3, 3).  Causal: the first rows see one to a few keys, so most of
    their weight sits on one key whatever the family -- checked on their own as well."""
    Bn, Hh, hd = 2, 2, 64
    D = Hh * hd
    qkv, _ = make_qkv(fam, Bn, S, Hh, hd, seed=500 + S)
    Q = hip.H2.pack(qkv)
    res = cpu_side(("mode0", S, causal, fam), lambda: emulations(
        tuple(planes_bhsd(Q, w, Bn, S, Hh, hd) for w in range(3)) + (None, causal, 1.0), lambda sp: GENERIC64, MODE0_SPLITS))
    Qd = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)]).cuda())
    for sp in MODE0_SPLITS:
        out = hip.H2.empty(Bn * S, D)
        out.t.fill_(float("nan"))
        hip.attention(Qd, out, Bn, S, Hh, hd, mode=0, causal=causal, split_qk=sp[0], split_pv=sp[1], scale=1.0, head_major=True)
        got = out.float().cpu().double().reshape(Bn, S, Hh, hd).permute(0, 2, 1, 3).reshape(Bn * Hh, S, hd)
        form = form_of(lambda sp: GENERIC64, sp)
        check(f"mode 0 S={S} causal={causal} {_fid(fam)} {sp}", got, res, form, False)
        if causal:
            check(f"mode 0 S={S} causal first rows {_fid(fam)} {sp}", got, res, form, False, rows=slice(0, 8))


SMALL = [(2, 6, 400, 8, 16), (2, 400, 6, 8, 16), (1, 6, 4096, 8, 16), (2, 5, 1300, 8, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", GAUSS + PEAK, ids=[_fid(f) for f in GAUSS + PEAK])
def test_small_attention_peaked(hip, fam):
    """The decoder's fp32 attention (cvlm_small_attention_h2): its emulation is fp32 scores on fp32 operands."""
    for i, (Bn, nq, nk, Hh, hd) in enumerate(SMALL):
        D = Hh * hd
        g = _gen(600 + i)
        b = math.sqrt(sigma_of(fam))                                       # the kernel applies 1 / sqrt(hd): score std = b^2
        q, k, v = (torch.randn(Bn, n, Hh, hd, generator=g) for n in (nq, nk, nk))
        q, k = q * b, k * b
        if fam[0] == "peak":
            j = 5 if fam[2] == "first" or nk <= 8 else nk - 3
            j = min(j, nk - 1)
            q[..., 0] = 1.0
            k[..., 0] = 0.0
            k[:, j, :, 0] = fam[1] * math.sqrt(hd)
        out = torch.empty(Bn, nq, D, device="cuda")
        out.fill_(float("nan"))
        hip.small_attention(q.reshape(Bn, nq, D).cuda(), k.reshape(Bn, nk, D).cuda(), v.reshape(Bn, nk, D).cuda(), out, Bn, nq, nk, Hh, hd)
        sp = lambda t: t.double().transpose(1, 2).reshape(Bn * Hh, t.shape[1], hd)
        z = lambda t: torch.zeros_like(t)
        qq, kk, vv = sp(q), sp(k), sp(v)
        ops = ((qq, z(qq)), (kk, z(kk)), (vv, z(vv)))
        st = {}
        res = {"ref": E.emulate(*ops, hd ** -0.5, f32_scores=False, stats=st), "stats": st}
        res[("full", "full")] = E.emulate(*ops, hd ** -0.5)
        got = out.cpu().double().reshape(Bn, nq, Hh, hd).transpose(1, 2).reshape(Bn * Hh, nq, hd)
        check(f"small attention {Bn, nq, nk, Hh, hd} {_fid(fam)}", got, res, ("full", "full"), False)


# ---------------------------------------------------------------------------------------------------------------------------------
# K's lo plane: read exactly where hip.attention_reads_k_lo says so
KLO = ([(1, G, 0, sp) for G in (20, 64, 96) for sp in SPLITS] + [(2, G, 14, sp) for G in (20, 64) for sp in SPLITS] +
       [(2, 20, w, sp) for w in (8, 12) for sp in SPLITS])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,G,ws,split", KLO, ids=[f"m{m}-G{G}-w{w}-{s[0]}{s[1]}" for m, G, w, s in KLO])
def test_k_lo_plane_read_exactly_where_the_predicate_says(hip, mode, G, ws, split):
    """Every mode-1 / mode-2 dispatch twice: with K's true lo plane and with K's lo plane NaN.  "Not read": the same bits.  "Read": NaN in
    the output.  (The engine's qkv projection skips that plane where the predicate says it is not read: SamEncoder._blocks_folded.)"""
    Bn, Hh, hd = (1, 2, 80)
    D, S = Hh * hd, G * G
    g = _gen(700 + G + ws)
    qkv = torch.randn(Bn * S, 3 * D, generator=g)
    pad = torch.randn(3 * D, generator=g) * 0.3
    L = ws or G
    rel_h, rel_w = torch.randn(2 * L - 1, hd, generator=g) * 0.2, torch.randn(2 * L - 1, hd, generator=g) * 0.2
    Q = hip.H2.pack(qkv)
    Qd = hip.H2(torch.stack([to_head_major(Q.t[i], Bn, S, Hh, hd) for i in range(2)]).cuda())
    Qn = hip.H2(Qd.t.clone())
    Qn.t[1].reshape(3, -1)[1].fill_(float("nan"))                       # head-major: the k third of the lo plane
    kw = dict(mode=mode, grid=G, rel_h=hip.H2(hip.H2.pack(rel_h).t.cuda()), rel_w=hip.H2(hip.H2.pack(rel_w).t.cuda()), split_qk=split[0],
              split_pv=split[1], head_major=True, scale=1.0)
    if mode == 2:
        kw.update(window=ws, pad=hip.H2(hip.H2.pack(pad).t.cuda()))
    outs = []
    for qq in (Qd, Qn):
        o = hip.H2.empty(Bn * S, D)
        o.t.fill_(7.0)
        hip.attention(qq, o, Bn, S, Hh, hd, **kw)
        outs.append(o.t.clone())
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any() and not bool((outs[0] == 7.0).all())
    reads = hip.attention_reads_k_lo(mode, G, ws, hd, *split)
    if reads:
        assert bool(torch.isnan(outs[1]).any()), "the predicate says K's lo plane is read, the kernel ignored it"
    else:
        assert torch.equal(outs[0], outs[1]), "the predicate says K's lo plane is not read, the kernel read it"
