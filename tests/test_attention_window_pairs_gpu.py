"""The persistent window-attention kernel (csrc/attention_win2.hip) on launches whose workgroups run SEVERAL (window, head) pairs, pair by
pair against fp64.

The kernel starts min(npairs, CUs) workgroups and carries three kinds of state from one pair of a workgroup into the next: the
three-slot K / V ring (seven key tiles per pair: every pair starts in another slot), the two row-offset tables (pair parity; refilled
three tiles before the stream enters a new pair) and the next pair's query rows (fetched at the top of a pair's last key tile).  The
other kernel-level tests stay below the CU count, one pair per workgroup.  Here tests/window_pairs.py picks, from the CU count of the
device, a batch that gives every workgroup three or four pairs which change head and go from padded windows to full ones and back; a
failure names the pair: image, head, window, workgroup and its position among that workgroup's items.

Token maps: G = 14 (no pad), 15 (remnant 1: the corner window holds ONE real token), 20 (remnant 6), 27 (remnant 13), 29 (3 x 3 windows,
full ones next to windows one token wide)."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import window_pairs as WP
from test_ops_gpu import SPLIT_TOL, ref_window_attention, relerr, rnd, to_head_major

pytestmark = pytest.mark.gpu

WS, HD = WP.WINDOW, 80
GUARD = 256            # rows of 7.0 in front of and behind the output rows
V_SPREAD = 2.0         # image b's V rows are shifted by V_SPREAD * b / B: consecutive pairs of a workgroup lie cus / (heads * nwin) images
                       # apart (a quarter of the batch and more), so a V tile taken from the neighbour in the stream moves every output
                       # of the pair by ~ 0.5 / 7 = 0.08, 1.5e-2 of max |ref| ~ 5 and twenty times the widest tolerance -- not by a random
                       # amount that an average hides.  (A common shift of V cancels in sum(p v) / sum(p): the errors are those without it.)
SPLITS = [(3, 3), (2, 2), (1, 2)]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    return h


def cu_count() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=1)
def case(cus, G, heads, B, prefold):
    """Host operands of one launch shape, packed to planes: Gaussian qkv, pad vector and rel-pos tables as in
    test_ops_gpu.test_attention_window_relpos, V shifted per image.  prefold: the engine's form -- hd^-0.5 folded into the q third of qkv
    and of the pad vector, its inverse into the tables, scale = 1.0 at the launch: the same scores, formed without the kernel's own
    rescaling of q.  The fp64 reference is computed at the first request and kept with the operands (one shape at a time)."""
    from camouflaged_vlm_amd.hip import H2
    D, S = heads * HD, G * G
    qkv = rnd(B * S, 3 * D, seed=21)
    qkv.view(B, S, 3, D)[:, :, 2] += (V_SPREAD * torch.arange(B, dtype=torch.float32) / B).view(B, 1, 1)
    pad = rnd(3 * D, seed=22, scale=0.3)
    rel_h, rel_w = rnd(2 * WS - 1, HD, seed=23, scale=0.2), rnd(2 * WS - 1, HD, seed=24, scale=0.2)
    if prefold:
        f = HD ** -0.5
        qkv.view(B * S, 3, D)[:, 0] *= f
        pad.view(3, D)[0] *= f
        rel_h, rel_w = rel_h / f, rel_w / f
    return SimpleNamespace(sched=WP.Schedule(cus, G, heads, B), G=G, heads=heads, B=B, D=D, S=S, scale=1.0 if prefold else HD ** -0.5,
                           prefold=prefold, Q=H2.pack(qkv), P=H2.pack(pad), RH=H2.pack(rel_h), RW=H2.pack(rel_w), ref=None)


def reference(c):
    """fp64 window attention of the packed operands (what the kernel is given), a few images at a time"""
    if c.ref is None:
        from camouflaged_vlm_amd.hip import H2
        f64 = lambda h: h.float().double()
        P, RH, RW = f64(c.P), f64(c.RH), f64(c.RW)
        parts = []
        for b0 in range(0, c.B, 16):
            nb = min(16, c.B - b0)
            x = f64(H2(c.Q.t[:, b0 * c.S:(b0 + nb) * c.S]))
            parts.append(ref_window_attention(x, P, RH, RW, nb, c.G, WS, c.heads, HD, c.scale))
        c.ref = torch.cat(parts)
    return c.ref


def device_qkv(hip, c, hm, b0=0, nb=None, nan_k_lo=False):
    """images b0 .. b0 + nb of the qkv planes on the device, token-major [nb*S][3][H][hd] or head-major [3][nb][H][S][hd] (rebuilt for the
    slice: the thirds of a head-major buffer are nb images long).  nan_k_lo: the K third of the lo plane filled with NaN."""
    nb = c.B if nb is None else nb
    t = c.Q.t[:, b0 * c.S:(b0 + nb) * c.S].contiguous().cuda()
    if hm:
        t = torch.stack([to_head_major(t[i], nb, c.S, c.heads, HD) for i in range(2)])
    if nan_k_lo:
        k_lo = t[1].view(3, -1)[1] if hm else t[1].view(nb * c.S, 3, c.D)[:, 1]
        k_lo.fill_(float("nan"))
    return hip.H2(t)


def launch(hip, c, split, hm, b0=0, nb=None, nan_k_lo=False):
    """-> the (2, GUARD + M + GUARD, D) buffer whose middle rows are the output: NaN before the launch, 7.0 around them"""
    nb = c.B if nb is None else nb
    M = nb * c.S
    big = torch.full((2, M + 2 * GUARD, c.D), 7.0, dtype=torch.float16, device="cuda")
    big[:, GUARD:GUARD + M] = float("nan")
    out = hip.H2(big[:, GUARD:GUARD + M])                           # a row slice: each plane contiguous, the planes GUARD rows further apart
    dev = lambda h: hip.H2(h.t.cuda())
    hip.attention(device_qkv(hip, c, hm, b0, nb, nan_k_lo), out, nb, c.S, c.heads, HD, mode=2, grid=c.G, window=WS, pad=dev(c.P),
                  rel_h=dev(c.RH), rel_w=dev(c.RW), split_qk=split[0], split_pv=split[1], head_major=hm,
                  scale=1.0 if c.prefold else None)
    torch.cuda.synchronize()
    return big


def check(c, big, split, what):
    """Guards untouched, no NaN left, the error of every pair (max abs over its real tokens / global max |ref|) and of the whole launch
    below SPLIT_TOL[split]; the message names the worst pair."""
    s, M, tol = c.sched, c.B * c.S, SPLIT_TOL[split]
    guards = torch.cat([big[:, :GUARD], big[:, GUARD + M:]], 1)
    assert bool((guards == 7.0).all()), f"{what}: rows outside the output were written"
    out = big[:, GUARD:GUARD + M]
    nans = int(torch.isnan(out).sum())
    got = (out[0].float() + out[1].float()).cpu().double()
    ref = reference(c)
    glob = relerr(got, ref)
    e = (got - ref).abs().view(c.B, c.G, c.G, c.heads, HD).amax(-1)
    gp = s.nwx * WS
    e = F.pad(e, (0, 0, 0, gp - c.G, 0, gp - c.G))                  # pad tokens have no output row: no error
    per_pair = e.view(c.B, s.nwx, WS, s.nwx, WS, c.heads).amax((2, 4)).reshape(-1) / ref.abs().max()   # (image, window, head) = pair order
    assert per_pair.numel() == s.npairs
    worst = int(per_pair.argmax())                                  # a NaN counts as the largest
    bad = (~(per_pair < tol)).nonzero().flatten().tolist()
    print(f"{what}: global {glob:.2e}, worst pair {float(per_pair[worst]):.2e} (tol {tol:.0e}), pairs per workgroup {s.counts()}")
    msg = (f"{what}: {len(bad)} of {s.npairs} pairs at or above {tol:.0e}, {nans} NaN elements; worst {float(per_pair[worst]):.3e} at "
           f"{s.describe(worst)}; positions k of the failing pairs {sorted({s.place(p)[1] for p in bad})}; "
           f"first failing {[s.describe(p) for p in bad[:4]]}")
    assert nans == 0, msg
    assert not bad and glob < tol, msg
    return float(per_pair[worst])


def assert_mixed(s):
    pr = WP.properties(s)
    assert WP.wanted(s), f"{s}: the schedule does not mix pair counts / heads / padded and full windows: {pr}"


# ---------------------------------------------------------------------------------------------
CASES = [(14, False), (15, False), (20, False), (20, True), (27, False), (29, False)]


@pytest.mark.parametrize("hm", [False, True], ids=["token-major", "head-major"])
@pytest.mark.parametrize("split", SPLITS, ids=lambda sp: f"split{sp[0]}{sp[1]}")
@pytest.mark.parametrize("G,prefold", CASES, ids=[f"G{G}{'-scale1' if p else ''}" for G, p in CASES])
def test_multi_pair_launch_vs_fp64(hip, G, prefold, split, hm):
    """Every workgroup runs 3 or 4 pairs (asserted for the CU count found).  Split (1, 2): K's lo plane is NaN, which the kernel must
    not read on any pair of a workgroup's stream."""
    cus = cu_count()
    heads, B = WP.choose(cus, G)
    c = case(cus, G, heads, B, prefold)
    assert_mixed(c.sched)
    nan_k_lo = split == (1, 2)
    if nan_k_lo:
        assert not hip.attention_reads_k_lo(2, G, WS, HD, 1, 2)
    big = launch(hip, c, split, hm, nan_k_lo=nan_k_lo)
    check(c, big, split, f"G={G} heads={heads} B={B} split={split} head-major={hm} scale={'1 (pre-folded)' if prefold else 'hd^-0.5'}")


@pytest.mark.parametrize("hm", [False, True], ids=["token-major", "head-major"])
@pytest.mark.parametrize("split", SPLITS, ids=lambda sp: f"split{sp[0]}{sp[1]}")
@pytest.mark.parametrize("G", [15, 20, 29])
def test_multi_pair_launch_has_the_bits_of_single_pair_launches(hip, G, split, hm):
    """A pair's result depends on that pair's data only and its order of operations does not depend on its place in a workgroup's stream:
    the batch in one launch (3 or 4 pairs per workgroup) and in slices of at most cus // (heads * nwin) images (one pair per workgroup)
    give the same bits."""
    cus = cu_count()
    heads, B = WP.choose(cus, G)
    c = case(cus, G, heads, B, False)
    assert_mixed(c.sched)
    whole = launch(hip, c, split, hm)[:, GUARD:GUARD + B * c.S]
    step = cus // (heads * c.sched.nwin)
    assert step >= 1
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        assert WP.Schedule(cus, G, heads, nb).counts() == [1]
        part = launch(hip, c, split, hm, b0=b0, nb=nb)[:, GUARD:GUARD + nb * c.S]
        rows = whole[:, b0 * c.S:(b0 + nb) * c.S]
        if not torch.equal(rows, part):
            d = (rows != part).view(2, nb, c.G, c.G, heads, HD).any(0).any(-1)            # [image][y][x][head]
            b, y, x, h = d.nonzero()[0].tolist()
            p = ((b0 + b) * c.sched.nwin + (y // WS) * c.sched.nwx + x // WS) * heads + h
            raise AssertionError(f"G={G} split={split} head-major={hm}: {int(d.sum())} (token, head) rows of images {b0}..{b0 + nb - 1} differ "
                                 f"from the single-pair launch; first at token ({y}, {x}) of {c.sched.describe(p)}")


@pytest.mark.parametrize("hm", [False, True], ids=["token-major", "head-major"])
@pytest.mark.parametrize("split", [(3, 3), (1, 2)], ids=lambda sp: f"split{sp[0]}{sp[1]}")
def test_one_extra_pair(hip, split, hm):
    """G = 14, one head, cus + 1 images: workgroup 0 runs two pairs, every other workgroup one -- the smallest launch that crosses a pair
    boundary."""
    cus = cu_count()
    c = case(cus, 14, 1, cus + 1, False)
    s = c.sched
    assert s.wgs == cus and [len(s.items(x)) for x in range(s.wgs)] == [2] + [1] * (cus - 1)
    nan_k_lo = split == (1, 2)
    if nan_k_lo:
        assert not hip.attention_reads_k_lo(2, 14, WS, HD, 1, 2)
    big = launch(hip, c, split, hm, nan_k_lo=nan_k_lo)
    check(c, big, split, f"G=14 heads=1 B={cus + 1} split={split} head-major={hm}")


# ---------------------------------------------------------------------------------------------
ENC_HEADS = 6          # the engine's activations want embed_dim % 32 == 0 (SamEncoder refuses other widths), so with head_dim 80 an even head
                       # count: 6 is the smallest that changes head and window inside a workgroup on 256 and on 304 workgroups (2 and 4 divide
                       # both: a workgroup would keep its head and its window)


@functools.lru_cache(maxsize=1)
def encoder_case(B):
    from camouflaged_vlm_amd import spec, synth
    from oracle import cvlm_oracle as O
    g = spec.SamGeometry(inp_size=320, embed_dim=ENC_HEADS * HD, depth=2, num_heads=ENC_HEADS, global_attn_indexes=(1,))
    sd_np = synth.make_state_dict(spec.sam_encoder_entries(g))
    inp = torch.from_numpy(synth.make_inputs(g, spec.TINY_CLIP, batch=B)[0])
    with torch.no_grad():
        ref = O.sam_encoder(inp, O.to_torch_sd(sd_np), g)
    return g, sd_np, inp, ref


@pytest.mark.parametrize("precision,split", [("exact", (3, 3)), ("mx12", (1, 2))])
def test_encoder_forward_with_several_pairs_per_workgroup(precision, split):
    """SamEncoder.forward as the engine calls the kernel (head-major qkv from the folded projection, scale 1, for (1, 2) a K lo plane that
    the projection never wrote) on 20 x 20 tokens at the batch that gives every workgroup of the window launch three or four pairs which
    mix heads and windows (38 images on 256 CUs), against the CPU oracle.  Depth 2 with one global block: the oracle takes two to three
    seconds at this batch and is shared by the two precisions.
    Geometry: 6 heads of 80 (embed_dim 480), not the 3 heads of 80 first meant for this test: at embed_dim = 240 the engine's GEMMs read
    the 240-wide activation rows at the weights' padded K = 256 -- run once, `exact` was off by 9.1 and `mx12` ended in an illegal
    memory access (30000 rows x 16 halves past the end of a plane).  SamEncoder now refuses such a width
    (test_attention_window_pairs_cpu.test_encoder_refuses_a_width_between_k_steps)."""
    from test_cascade_gpu import TOL
    from camouflaged_vlm_amd.engine import Precision, SamEncoder
    cus = cu_count()
    B = WP.smallest_batch(cus, 20, ENC_HEADS)
    g, sd_np, inp, ref = encoder_case(B)
    s = WP.Schedule(cus, g.grid, g.num_heads, B)
    assert_mixed(s)
    assert s.counts()[0] >= 3
    dev = torch.device("cuda:0")
    enc = SamEncoder({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, dev, Precision.named(precision))
    enc.record = {"attn_splits": set(), "mx_operands": False}
    got = enc.forward(inp.to(dev)).cpu().reshape(B, g.grid, g.grid, g.out_chans).permute(0, 3, 1, 2)
    assert enc.record["attn_splits"] == {split}                      # B * 400 rows: a batch, the precision's own split
    assert enc.ws.gemm_errors() == 0
    d = (got - ref).abs().flatten(1).amax(1)
    err, b = float(d.max()), int(d.argmax())
    print(f"320^2 encoder, {ENC_HEADS} heads, B={B}, {precision}: max abs err vs oracle {err:.2e} (image {b}), pairs per workgroup {s.counts()}")
    assert err < TOL, f"image {b}: {err:.2e}"
