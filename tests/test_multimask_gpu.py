"""Multimask output and predicted mask quality of the edge decoder (Cascade.infer_test_multimask, SAM.infer_test_multimask,
Cascade.infer_classes(quality=True)): the kernel behind it (cvlm_mask_head_multi) against fp64 and against the one-mask kernels'
bits, every mask of every image against the reference's own `predict_masks` call (tests/golden/tiny_multimask.npz,
demo_multimask_digest.npz, demo_multimask_bits.npz; tools/make_multimask_golden.py), the slices and the drop-in surface.
Gate (BASELINE.json north_star): 1e-3 abs on mask / edge logits, IoU >= 0.999; iou_pred within 1e-3 of the fixture's largest
|score| (the scores of synthetic weights are <= 0.08: an absolute 1e-3 would be 1 % of them), and the order of two scores of a
prompt that lie more than twice that apart."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, IOU, IOU_REL = 1e-3, 0.999, 1e-3


def dmax(a, b) -> float:
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def relerr(got, ref) -> float:
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def iou(a, b) -> float:
    a, b = torch.as_tensor(a) > 0, torch.as_tensor(b) > 0
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


# ---- kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,HW", [(1, 1000), (40, 700), (3, 256), (2, 77)])     # 1000, 700, 77: not multiples of the 256-pixel tile
@pytest.mark.parametrize("n_masks", [1, 4])
@pytest.mark.parametrize("mode", ["edge_prob", "no_edge_prob", "no_edge_emb"])
def test_mask_head_multi_against_fp64_and_one_mask_bits(P, HW, n_masks, mode):
    from camouflaged_vlm_amd import hip
    dev = torch.device("cuda:0")
    Cc = 32
    gen = torch.Generator().manual_seed(100 * P + n_masks)
    up = torch.randn(P, HW, Cc, generator=gen)
    emb = torch.randn(P, HW, Cc, generator=gen)
    hyper = torch.randn(P, 5, Cc, generator=gen)
    ud, ed, hd = up.to(dev), emb.to(dev), hyper.to(dev)
    guard = 64                                               # floats behind each output: nothing may be written there
    low = torch.full((P * n_masks * HW + guard,), float("nan"), device=dev)
    edge = torch.full((P * HW + guard,), float("nan"), device=dev)
    hip.mask_head_multi(ud, None if mode == "no_edge_emb" else ed, hd, P, HW, Cc, n_masks, low, edge if mode == "edge_prob" else None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(low[P * n_masks * HW:]).all()) and bool(torch.isnan(edge[P * HW:]).all())
    got = low[:P * n_masks * HW].view(P, n_masks, HW)
    x = torch.einsum("phc,pmc->pmh", up.double(), hyper[:, :n_masks].double())
    s = torch.sigmoid(torch.einsum("phc,pc->ph", emb.double(), hyper[:, 4].double()))
    want = x if mode == "no_edge_emb" else x * s[:, None] + x
    errs = [relerr(got[:, m], want[:, m]) for m in range(n_masks)]
    print(f"mask_head_multi P={P} HW={HW} n={n_masks} {mode}: planes vs fp64 {['%.2e' % e for e in errs]}")
    assert max(errs) < 3e-6                                  # what tests/test_ops_gpu.py holds cvlm_mask_head to
    # plane 0 (and the edge map) hold the bits of the one-mask kernels on the same buffers
    low1, edge1 = torch.empty(P, HW, device=dev), torch.empty(P, HW, device=dev)
    if mode == "no_edge_emb":
        hip.mask_head(ud, None, hd, P, HW, Cc, low1)
    else:
        hip.mask_head_edge(ud, ed, hd, P, HW, Cc, low1, edge1)
    torch.cuda.synchronize()
    assert torch.equal(got[:, 0], low1)
    if mode == "edge_prob":
        assert relerr(edge[:P * HW].view(P, HW), s) < 3e-6 and torch.equal(edge[:P * HW].view(P, HW), edge1)
    else:
        assert bool(torch.isnan(edge).all())                 # not asked for: not written


# ---- tiny geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_multimask.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device("cuda:0")
    return g, c, sd_np, tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


@pytest.fixture(scope="module")
def tiny_cas(tiny, gold):
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c, sd_np, _, dev = tiny
    cas = Cascade({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, c, dev, Precision.named("exact"))
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), torch.from_numpy(gold["bank_test"]), "test")
    return cas


def _check_iou(got, ref, tag):
    """got, ref (B, 4): within IOU_REL of the fixture's largest |score|; two scores of a prompt more than twice that apart keep
    their order (each inside the bar, they cannot swap across that gap)."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
    s = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{tag}: iou_pred {got.tolist()} vs reference {ref.tolist()}: max |diff| {err:.2e} = {err / s:.2e} of the largest |score| {s:.4f} "
          f"(bar {IOU_REL:.0e})")
    assert err <= IOU_REL * s, (tag, err, s)
    for b in range(ref.shape[0]):
        for i in range(ref.shape[1]):
            for j in range(ref.shape[1]):
                if ref[b, i] - ref[b, j] > 2 * IOU_REL * s:
                    assert got[b, i] > got[b, j], (tag, b, i, j)


def test_tiny_all_masks_bits_and_reference(tiny, tiny_cas, gold):
    g, c, _, (inp, ci, cm), dev = tiny
    cas = tiny_cas
    S, L = g.inp_size, 4 * g.grid
    one = cas.infer_test(inp, ci, cm).clone()
    k1 = cas.infer_classes(inp, ci, cm, topk=1)
    k1_edges = k1.edges.clone()
    ms = cas.infer_test_multimask(inp, ci, cm, all_masks=True)
    torch.cuda.synchronize()
    assert ms.masks.shape == (2, 4, S, S) and ms.edges.shape == (2, S, S) and ms.iou.shape == (2, 4)
    assert ms.low_res_masks.shape == (2, 4, L, L)
    assert torch.equal(ms.masks[:, 0], one[:, 0])            # mask 0 is infer_test's, bit for bit
    assert torch.equal(ms.edges, k1_edges[:, 0])             # the edge map is the K = 1 hypothesis's
    ref_m = F.interpolate(torch.from_numpy(gold["low_masks"]), (S, S), mode="bilinear", align_corners=False)
    ref_e = F.interpolate(torch.from_numpy(gold["low_edges"])[:, None], (S, S), mode="bilinear", align_corners=False)[:, 0]
    pos = torch.from_numpy(gold["pos"]).to(dev)
    for b in range(2):
        for m in range(4):
            dl, df = dmax(ms.low_res_masks[b, m], gold["low_masks"][b, m]), dmax(ms.masks[b, m], ref_m[b, m])
            dp = dmax(ms.masks[b, m].reshape(-1)[pos], gold["masks_at_pos"][b, m])
            io = iou(ms.masks[b, m].cpu(), ref_m[b, m])
            print(f"tiny exact image {b} mask {m}: low-res {dl:.2e} full-res {df:.2e} at the reference's positions {dp:.2e} IoU {io:.6f}")
            assert max(dl, df, dp) <= TOL and io >= IOU, (b, m, dl, df, dp, io)
    de = dmax(ms.edges, ref_e)
    print(f"tiny exact edges {de:.2e}")
    assert de <= TOL
    _check_iou(ms.iou, gold["iou"], "tiny exact")


def test_slices_and_quality(tiny, tiny_cas):
    _, _, _, (inp, ci, cm), dev = tiny
    cas = tiny_cas
    full = cas.infer_test_multimask(inp, ci, cm, all_masks=True)
    three = cas.infer_test_multimask(inp, ci, cm)             # multimask_output=True is the default, as a SAM predictor's
    one = cas.infer_test_multimask(inp, ci, cm, multimask_output=False)
    torch.cuda.synchronize()
    assert three.masks.shape[1] == 3 and three.iou.shape == (2, 3) and three.low_res_masks.shape[1] == 3
    assert torch.equal(three.masks, full.masks[:, 1:]) and torch.equal(three.iou, full.iou[:, 1:])
    assert torch.equal(three.low_res_masks, full.low_res_masks[:, 1:]) and torch.equal(three.edges, full.edges)
    assert one.masks.shape[1] == 1 and one.iou.shape == (2, 1)
    assert torch.equal(one.masks, full.masks[:, :1]) and torch.equal(one.iou, full.iou[:, :1])
    assert torch.equal(one.low_res_masks, full.low_res_masks[:, :1]) and torch.equal(one.edges, full.edges)
    # quality=True changes nothing else, and scores hypothesis 0 of K = 1 as infer_test_multimask scores mask 0
    plain = cas.infer_classes(inp, ci, cm, topk=3)
    plain = {f: getattr(plain, f).clone() for f in ("classes", "pass1_logits", "masks", "edges", "logits", "pred")}
    q = cas.infer_classes(inp, ci, cm, topk=3, quality=True)
    torch.cuda.synchronize()
    assert cas.infer_classes(inp, ci, cm, topk=3).iou is None
    assert all(torch.equal(getattr(q, f), plain[f]) for f in plain)
    assert q.iou.shape == (2, 3) and bool(torch.isfinite(q.iou).all())
    q1 = cas.infer_classes(inp, ci, cm, topk=1, quality=True)
    torch.cuda.synchronize()
    assert torch.equal(q1.iou, one.iou)
    assert torch.equal(q.iou[:, 0], q1.iou[:, 0]) or dmax(q.iou[:, 0], q1.iou[:, 0]) <= 6e-5     # K = 3: other GEMM row counts
    # infer_test still gives its bits after multimask calls (grow-only workspace, new buffers of their own)
    a = cas.infer_test(inp, ci, cm).clone()
    cas.infer_test_multimask(inp, ci, cm, all_masks=True)
    b = cas.infer_test(inp, ci, cm)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---- demo geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dgold(golden_dir):
    out = {}
    for name in ("demo_multimask_digest.npz", "demo_multimask_bits.npz"):
        with np.load(os.path.join(golden_dir, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def demo_sd():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    return g, c, {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}


@pytest.mark.parametrize("precision", ["mx", "exact"])
def test_demo_every_mask_matches_reference_digest(demo_sd, dgold, golden_dir, precision):
    from camouflaged_vlm_amd import synth
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c, sd = demo_sd
    dev = torch.device("cuda:0")
    with np.load(os.path.join(golden_dir, "ovcamo_constants.npz")) as z:
        bank = torch.from_numpy(z["bank_test"]).float()
    cas = Cascade(sd, g, c, dev, Precision.named(precision))
    cas.clip.set_text_bank(cas.clip.text_features(dgold["eot_test"].tolist(), "test"), bank, "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))
    assert precision != "mx" or inp.shape[0] * g.grid ** 2 > 4096          # M = 8192 token rows: the mx path
    ms = cas.infer_test_multimask(inp, ci, cm, all_masks=True)
    one = cas.infer_test(inp, ci, cm)
    torch.cuda.synchronize()
    assert torch.equal(ms.masks[:, 0], one[:, 0])
    B = 2
    m, e = ms.masks.reshape(B, 4, -1), ms.edges.reshape(B, -1)
    sample = torch.from_numpy(dgold["sample_idx"]).long().to(dev)
    dense = torch.from_numpy(dgold["dense_idx"]).long().to(dev)
    rows = []
    for b in range(B):
        de = dmax(e[b][sample], dgold["edge_samples"][b])
        for k in range(4):
            mk = m[b, k]
            sets = {"sample": dmax(mk[sample], dgold["mask_samples"][b, k]), "dense": dmax(mk[dense], dgold["dense_samples"][b, k]),
                    "near": dmax(mk[torch.from_numpy(dgold["near_idx"][b, k]).long().to(dev)], dgold["near_samples"][b, k])}
            bits = torch.from_numpy(np.unpackbits(dgold["mask_bits"][b, k])[:mk.numel()].astype(bool))
            ours = (mk > 0).cpu()
            io = float((ours & bits).sum()) / max(float((ours | bits).sum()), 1.0)
            dm = max(sets.values())
            rows.append((b, k, dm, io, de))
            print(f"demo {precision} image {b} mask {k}: mask {dm:.2e} (sample {sets['sample']:.2e} dense {sets['dense']:.2e} near "
                  f"{sets['near']:.2e}), IoU {io:.6f}, edge {de:.2e}, positive {float(ours.float().mean()):.3f}")
    try:
        _check_iou(ms.iou, dgold["iou"], f"demo {precision}")
    finally:                                                 # the mask figures are judged whatever the scores did
        for b, k, dm, io, de in rows:
            assert dm <= TOL and io >= IOU and de <= TOL, (precision, b, k, dm, io, de)


# ---- drop-in ------------------------------------------------------------------------------------------------------------------
def test_dropin_infer_test_multimask_is_the_engine_call(tiny, gold, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    from camouflaged_vlm_amd.engine import MaskSet
    g, c, sd_np, (inp, ci, cm), dev = tiny
    with np.load(os.path.join(golden_dir, "tiny_cascade.npz")) as z:
        eot_train = z["eot_train"].tolist()
    clip = CustomCLIP(geometry=c, eot_train=eot_train, eot_test=gold["eot_test"].tolist())
    enc = dict(name="sam", img_size=g.inp_size, mlp_ratio=4, patch_size=16, qkv_bias=True, use_rel_pos=True,
               window_size=14, out_chans=256, scale_factor=32, input_type="fft", freq_nums=0.25, prompt_type="highpass",
               prompt_embed_dim=256, tuning_stage=1234, handcrafted_tune=True, embedding_tune=True, adaptor="adaptor",
               embed_dim=g.embed_dim, depth=g.depth, num_heads=g.num_heads, global_attn_indexes=list(g.global_attn_indexes))
    model = models.make({"name": "sam_maskdecoder_edge", "args": {"inp_size": g.inp_size, "loss": "iou", "encoder_mode": enc}}).cuda()
    model.train_text_features = model.train_text_features[:c.n_cls_train]
    model.test_text_features = model.test_text_features[:c.n_cls_test]
    model.load_mapleAlphaCLIP(clip)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    model.eval()
    with torch.no_grad():
        got = model.infer_test_multimask(inp, ci, cm)
        want = model.cascade().infer_test_multimask(inp, ci, cm, multimask_output=True)
        torch.cuda.synchronize()
        assert isinstance(got, MaskSet) and got.masks.shape[1] == 3
        assert all(torch.equal(getattr(got, f), getattr(want, f)) for f in ("masks", "iou", "edges", "low_res_masks"))
        q = model.infer_classes(inp, ci, cm, topk=2, quality=True)
        torch.cuda.synchronize()
        assert q.iou.shape == (2, 2)
        with pytest.raises(AssertionError):
            model.infer_test_multimask(inp[:, :, :g.inp_size - 16, :g.inp_size - 16], ci, cm)
