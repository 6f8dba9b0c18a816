"""K class hypotheses per image from one encoder pass (Cascade.infer_classes, SAM.infer_classes): the two kernels behind it
(cvlm_mask_head_edge, cvlm_topk_select), parity against the reference's own K-prompt decoder call (tests/golden/tiny_classes.npz,
demo_classes_digest.npz; tools/make_classes_golden.py), K = 1 against the cascade, independence of the hypotheses, engine state,
chunking and the drop-in surface.  Gate (BASELINE.json north_star): 1e-3 abs on mask / edge / class logits, IoU >= 0.999, equal
predictions."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, IOU = 1e-3, 0.999
BATCH_TOL = 6e-5            # a batch against its single forwards with the GEMM K-splits on (tests/test_cascade_gpu.py)


def dmax(a, b) -> float:
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def iou(a, b) -> float:
    a, b = torch.as_tensor(a) > 0, torch.as_tensor(b) > 0
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def same(x, y) -> bool:
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in ("classes", "pass1_logits", "masks", "edges", "logits", "pred"))


def _topk_host(row: np.ndarray, K: int):
    if np.isnan(row).any():
        return [-1] * K
    return sorted(range(len(row)), key=lambda c: (-row[c], c))[:K]


def _order_matches(classes, gold_classes, gold_p1):
    """topk's classes equal the golden's wherever the golden's adjacent pass-1 logits differ by more than 1e-3."""
    B, K = gold_classes.shape
    for b in range(B):
        gl = gold_p1[b][gold_classes[b]]
        for k in range(K):
            if (k == 0 or gl[k - 1] - gl[k] > 1e-3) and (k == K - 1 or gl[k] - gl[k + 1] > 1e-3):
                assert int(classes[b, k]) == int(gold_classes[b, k]), (b, k)


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def test_mask_head_edge_against_fp64_and_mask_head_bits():
    from camouflaged_vlm_amd import hip
    dev = torch.device("cuda:0")
    P, HW, Cc = 7, 1000, 32                                  # P not a multiple of 8, HW not a multiple of the 256-thread block
    gen = torch.Generator().manual_seed(3)
    up = torch.randn(P, HW, Cc, generator=gen)
    emb = torch.randn(P, HW, Cc, generator=gen)
    hyper = torch.randn(P, 5, Cc, generator=gen) * 0.3
    low, edge, low0 = (torch.full((P, HW), float("nan"), device=dev) for _ in range(3))
    ud, ed, hd = up.to(dev), emb.to(dev), hyper.to(dev)
    hip.mask_head_edge(ud, ed, hd, P, HW, Cc, low, edge)
    hip.mask_head(ud, ed, hd, P, HW, Cc, low0)
    torch.cuda.synchronize()
    m = torch.einsum("phc,pc->ph", up.double(), hyper[:, 0].double())
    s = torch.sigmoid(torch.einsum("phc,pc->ph", emb.double(), hyper[:, 4].double()))
    want = m * s + m
    dm, de = dmax(low, want), dmax(edge, s)
    print(f"mask head with edge output vs fp64: mask {dm:.2e} (|mask| <= {float(want.abs().max()):.1f}), edge {de:.2e}")
    assert dm <= 2e-5 * max(1.0, float(want.abs().max())) and de <= 1e-6
    assert torch.equal(low, low0)                            # the mask output has cvlm_mask_head's bits


def test_topk_select_against_host_sort():
    from camouflaged_vlm_amd import hip
    dev = torch.device("cuda:0")
    B, C, D = 6, 61, 768
    gen = torch.Generator().manual_seed(5)
    img = torch.randn(B, D, generator=gen)
    txt = torch.randn(C, D, generator=gen)
    txt[7] = txt[3]                                          # planted ties: equal rows give bit-equal logits
    txt[40] = txt[3]
    txt[11] = txt[29]
    img[0] = txt[3] * 4.0                                    # image 0's maximum is the tie 3 / 7 / 40
    img[1] = txt[29] * 4.0                                   # image 1's maximum is the tie 11 / 29
    img_d, txt_d = img.to(dev), txt.to(dev)
    img_n, logits = torch.empty(B, D, device=dev), torch.empty(B, C, device=dev)
    pred, tsel = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, D, device=dev)
    hip.clip_head(img_d, txt_d, 100.0, B, C, D, img_n, logits, pred, tsel)
    torch.cuda.synchronize()
    lg = logits.clone()
    top = float(lg[2].max()) + 1.0
    lg[2, 5] = top                                           # a tie at the top planted in the logits themselves
    lg[2, 50] = top
    lg[4, 17] = float("nan")                                 # a NaN row
    lh = lg.cpu().numpy()
    assert _topk_host(lh[0], 3) == [3, 7, 40] and _topk_host(lh[1], 2) == [11, 29] and _topk_host(lh[2], 2) == [5, 50]
    for K in (1, 5, C):
        idx = torch.full((B, K), -7, dtype=torch.int64, device=dev)
        sel = torch.empty(B, K, D, device=dev)
        hip.topk_select(lg, B, C, K, txt_d, D, None, idx, sel)
        torch.cuda.synchronize()
        for b in range(B):
            assert idx[b].tolist() == _topk_host(lh[b], K), (K, b)
        ok = idx >= 0
        assert torch.equal(sel[ok], txt_d[idx[ok]])          # the gather is bit for bit
        assert bool(torch.isnan(sel[4]).all()) and idx[4].tolist() == [-1] * K
        if K == 1:                                           # on finite rows: cvlm_clip_head's strict-`>` first maximum
            finite = [b for b in range(B) if b not in (2, 4)]
            assert idx[finite, 0].tolist() == pred[finite].tolist()
    # gather only (idx_in): repeats and K > C allowed, no ranking, logits unused
    K = 70
    want = torch.randint(0, C, (B, K), generator=gen)
    idx = torch.empty(B, K, dtype=torch.int64, device=dev)
    sel = torch.empty(B, K, D, device=dev)
    hip.topk_select(None, B, C, K, txt_d, D, want.to(dev), idx, sel)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), want) and torch.equal(sel, txt_d[want.to(dev)])


# ---- tiny geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device("cuda:0")
    return g, c, sd_np, tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


def build_tiny(tiny, gold, precision="exact"):
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c, sd_np, _, dev = tiny
    cas = Cascade({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, c, dev, Precision.named(precision))
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), torch.from_numpy(gold["bank_test"]), "test")
    return cas


def test_tiny_hypotheses_match_reference(tiny, gold):
    g, c, _, (inp, ci, cm), dev = tiny
    cas = build_tiny(tiny, gold)
    classes = torch.from_numpy(gold["classes"])
    h = cas.infer_classes(inp, ci, cm, classes=classes.to(dev))
    torch.cuda.synchronize()
    B, K = classes.shape
    S = g.inp_size
    assert h.masks.shape == (B, K, S, S) and h.edges.shape == (B, K, S, S) and h.logits.shape == (B, K, c.n_cls_test)
    assert h.classes.tolist() == classes.tolist()
    ref_m = F.interpolate(torch.from_numpy(gold["low_masks"]), (S, S), mode="bilinear", align_corners=False)
    ref_e = F.interpolate(torch.from_numpy(gold["low_edges"]), (S, S), mode="bilinear", align_corners=False)
    dpos = dmax(h.masks.reshape(B, K, -1)[:, :, torch.from_numpy(gold["pos"]).to(dev)], gold["masks_at_pos"])
    rep = {"masks": dmax(h.masks, ref_m), "masks_at_pos": dpos, "edges": dmax(h.edges, ref_e),
           "pass1_logits": dmax(h.pass1_logits, gold["pass1_logits"]), "stage2_logits": dmax(h.logits, gold["class_logits"]),
           "min_iou": min(iou(h.masks[b, k].cpu(), ref_m[b, k]) for b in range(B) for k in range(K))}
    print("tiny hypotheses vs reference (exact):", {k: f"{v:.2e}" for k, v in rep.items()})
    for b in range(B):
        for k in range(K):
            print(f"  tiny image {b} class {int(classes[b, k])}: mask {dmax(h.masks[b, k], ref_m[b, k]):.2e} edge "
                  f"{dmax(h.edges[b, k], ref_e[b, k]):.2e} stage-2 logits {dmax(h.logits[b, k], gold['class_logits'][b, k]):.2e}")
    for k in ("masks", "masks_at_pos", "edges", "pass1_logits", "stage2_logits"):
        assert rep[k] <= TOL, rep
    assert rep["min_iou"] >= IOU and h.pred.tolist() == gold["pred"].tolist()
    # topk: the engine's own pass-1 order, which is the golden's wherever adjacent golden logits are more than 1e-3 apart
    t = cas.infer_classes(inp, ci, cm, topk=K)
    torch.cuda.synchronize()
    p1 = t.pass1_logits.cpu().numpy()
    for b in range(B):
        assert t.classes[b].tolist() == _topk_host(p1[b], K)
    _order_matches(t.classes, gold["classes"], gold["pass1_logits"])


def _assert_k1_is_cascade(cas, inp, ci, cm):
    m, p, l = (t.clone() for t in cas.cascade(inp, ci, cm))
    h = cas.infer_classes(inp, ci, cm, topk=1)
    torch.cuda.synchronize()
    assert torch.equal(h.masks[:, 0], m[:, 0]) and torch.equal(h.logits[:, 0], l) and torch.equal(h.pred[:, 0], p)
    return h


def test_k1_is_the_cascade_tiny_exact(tiny, gold):
    _, _, _, (inp, ci, cm), _ = tiny
    _assert_k1_is_cascade(build_tiny(tiny, gold), inp, ci, cm)


def test_hypotheses_do_not_talk_to_each_other(tiny, gold, monkeypatch):
    """With the GEMM K-splits off every (b, k) of a K = 5 call is the one-hypothesis call on that image, bit for bit; with the
    default switches within the batch tolerance."""
    _, c, _, (inp, ci, cm), dev = tiny
    K = c.n_cls_test
    classes = torch.tensor([[4, 0, 2, 2, 1], [3, 1, 0, 4, 2]], dtype=torch.int64)
    for ksplit in (False, True):
        if not ksplit:
            monkeypatch.setenv("CVLM_GEMM_TAIL", "0")
            monkeypatch.setenv("CVLM_GEMM_SK", "0")
        else:
            monkeypatch.delenv("CVLM_GEMM_TAIL", raising=False)
            monkeypatch.delenv("CVLM_GEMM_SK", raising=False)
        cas = build_tiny(tiny, gold)
        h = cas.infer_classes(inp, ci, cm, classes=classes)
        hm, he, hl, hp = (t.clone() for t in (h.masks, h.edges, h.logits, h.pred))
        worst = 0.0
        for b in range(2):
            for k in range(K):
                s = cas.infer_classes(inp[b:b + 1], ci[b:b + 1], cm[b:b + 1], classes=classes[b:b + 1, k:k + 1])
                torch.cuda.synchronize()
                if not ksplit:
                    assert torch.equal(s.masks[0, 0], hm[b, k]) and torch.equal(s.edges[0, 0], he[b, k])
                    assert torch.equal(s.logits[0, 0], hl[b, k]) and torch.equal(s.pred[0, 0], hp[b, k])
                else:
                    worst = max(worst, dmax(s.masks[0, 0], hm[b, k]), dmax(s.edges[0, 0], he[b, k]), dmax(s.logits[0, 0], hl[b, k]))
                    assert int(s.pred[0, 0]) == int(hp[b, k])
        if ksplit:
            print(f"hypotheses vs one-hypothesis calls, default switches: {worst:.2e}")
            assert worst <= BATCH_TOL


def test_state_pipelined_flush_workspace_and_refusals(tiny, gold):
    from camouflaged_vlm_amd import hip
    _, c, _, (inp, ci, cm), dev = tiny
    cas = build_tiny(tiny, gold)
    want_m, want_p, want_l = (t.clone() for t in cas.cascade(inp, ci, cm))
    fresh = build_tiny(tiny, gold).infer_classes(inp, ci, cm, topk=3)
    torch.cuda.synchronize()
    # a pipelined batch owes its stage 2: infer_classes flushes it first, and a later flush() has nothing left to do
    masks, pred, logits = cas.cascade(inp, ci, cm, pipelined=True)
    h = cas.infer_classes(inp, ci, cm, topk=3)
    cas.flush()
    torch.cuda.synchronize()
    assert torch.equal(masks, want_m) and torch.equal(pred, want_p) and torch.equal(logits, want_l)
    assert same(h, fresh)
    # grow-only workspace: infer_test / cascade give the same bits after a call with more prompts
    t0 = cas.infer_test(inp, ci, cm).clone()
    c0 = [t.clone() for t in cas.cascade(inp, ci, cm)]
    cas.infer_classes(inp, ci, cm, classes=torch.randint(0, c.n_cls_test, (2, 9), device=dev))
    t1 = cas.infer_test(inp, ci, cm)
    c1 = cas.cascade(inp, ci, cm)
    torch.cuda.synchronize()
    assert torch.equal(t0, t1) and all(torch.equal(a, b) for a, b in zip(c0, c1))
    # bad requests raise ValueError on the host and launch nothing
    calls = []
    saved = {n: getattr(hip, n) for n in ("gemm", "layernorm", "topk_select", "patchify", "split_f32")}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        bad = [dict(), dict(topk=2, classes=torch.zeros(2, 2, dtype=torch.int64)), dict(topk=0), dict(topk=c.n_cls_test + 1),
               dict(topk=1.0), dict(classes=torch.zeros(2, 2, dtype=torch.int32)), dict(classes=torch.zeros(3, 2, dtype=torch.int64)),
               dict(classes=torch.zeros(2, dtype=torch.int64)), dict(classes=torch.zeros(2, 0, dtype=torch.int64)),
               dict(classes=torch.tensor([[0, c.n_cls_test], [0, 0]])), dict(classes=torch.tensor([[0, -1], [1, 1]], device=dev)),
               dict(classes=[[0, 1], [1, 0]])]
        for kw in bad:
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


# ---- demo geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def demo_sd():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    return g, c, {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}


@pytest.fixture(scope="module")
def dgold(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def demo_inputs(demo_sd):
    from camouflaged_vlm_amd import synth
    g, c, _ = demo_sd
    dev = torch.device("cuda:0")
    return tuple(torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))


@pytest.fixture(scope="module")
def demo_engines(demo_sd, dgold, golden_dir):
    """One demo-geometry engine per precision for the whole module."""
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c, sd = demo_sd
    with np.load(os.path.join(golden_dir, "ovcamo_constants.npz")) as z:
        bank = torch.from_numpy(z["bank_test"]).float()
    out = {}
    for p in ("mx", "exact"):
        cas = Cascade(sd, g, c, torch.device("cuda:0"), Precision.named(p))
        cas.clip.set_text_bank(cas.clip.text_features(dgold["eot_test"].tolist(), "test"), bank, "test")
        out[p] = cas
    return out


def _check_digest(h, dgold, tag):
    B, K = dgold["classes"].shape
    m = h.masks.reshape(B, K, -1)
    e = h.edges.reshape(B, K, -1)
    dev = m.device
    sample = torch.from_numpy(dgold["sample_idx"]).long().to(dev)
    dense = torch.from_numpy(dgold["dense_idx"]).long().to(dev)
    rows = []
    for b in range(B):
        for k in range(K):
            mk = m[b, k]
            sets = {"sample": dmax(mk[sample], dgold["mask_samples"][b, k]), "dense": dmax(mk[dense], dgold["dense_samples"][b, k]),
                    "near": dmax(mk[torch.from_numpy(dgold["near_idx"][b, k]).long().to(dev)], dgold["near_samples"][b, k])}
            bits = torch.from_numpy(np.unpackbits(dgold["mask_bits"][b, k])[:mk.numel()].astype(bool))
            ours = (mk > 0).cpu()
            io = float((ours & bits).sum()) / max(float((ours | bits).sum()), 1.0)
            de = dmax(e[b, k][sample], dgold["edge_samples"][b, k])
            dl = dmax(h.logits[b, k], dgold["class_logits"][b, k])
            dm = max(sets.values())
            rows.append((b, k, dm, io, de, dl))
            print(f"demo {tag} image {b} class {int(dgold['classes'][b, k])}: mask {dm:.2e} (sample {sets['sample']:.2e} dense "
                  f"{sets['dense']:.2e} near {sets['near']:.2e}), IoU {io:.6f}, edge {de:.2e}, stage-2 logits {dl:.2e}, "
                  f"pred {int(h.pred[b, k])} / {int(dgold['pred'][b, k])}")
    for b, k, dm, io, de, dl in rows:
        assert dm <= TOL and io >= IOU and de <= TOL and dl <= TOL, (tag, b, k, dm, io, de, dl)
    assert h.pred.tolist() == dgold["pred"].tolist()
    assert dmax(h.pass1_logits, dgold["pass1_logits"]) <= TOL


@pytest.mark.parametrize("precision", ["mx", "exact"])
def test_demo_hypotheses_match_reference_digest(demo_engines, dgold, demo_inputs, precision):
    cas = demo_engines[precision]
    inp, ci, cm = demo_inputs
    h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(dgold["classes"]))
    torch.cuda.synchronize()
    _check_digest(h, dgold, precision)
    t = cas.infer_classes(inp, ci, cm, topk=dgold["classes"].shape[1])
    torch.cuda.synchronize()
    _order_matches(t.classes, dgold["classes"], dgold["pass1_logits"])


def test_demo_k1_is_the_cascade_mx(demo_engines, demo_inputs):
    inp, ci, cm = demo_inputs
    cas = demo_engines["mx"]
    assert inp.shape[0] * cas.g.grid ** 2 > 4096                # M = 8192 token rows: the mx path
    _assert_k1_is_cascade(cas, inp, ci, cm)


def test_demo_chunked_prompts(demo_engines, dgold, demo_inputs):
    """B = 2, K = 61: 122 prompts in more than one decoder pass; the golden's three classes come out as in the K = 3 call."""
    inp, ci, cm = demo_inputs
    cas = demo_engines["exact"]
    n_cls = cas.clip.txt["test"].shape[0]
    assert 2 * n_cls > cas.class_chunk()
    three = torch.from_numpy(dgold["classes"])
    h3 = cas.infer_classes(inp, ci, cm, classes=three)
    h3 = {f: getattr(h3, f).clone() for f in ("masks", "edges", "logits", "pred")}
    hall = cas.infer_classes(inp, ci, cm, topk=n_cls)
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(2):
        order = hall.classes[b].tolist()
        for k, cl in enumerate(three[b].tolist()):
            j = order.index(cl)
            worst = max(worst, dmax(hall.masks[b, j], h3["masks"][b, k]), dmax(hall.edges[b, j], h3["edges"][b, k]),
                        dmax(hall.logits[b, j], h3["logits"][b, k]))
            assert int(hall.pred[b, j]) == int(h3["pred"][b, k])
    print(f"122 prompts in chunks of {cas.class_chunk()} vs the K = 3 call (exact): {worst:.2e}")
    assert worst <= BATCH_TOL


# ---- drop-in ------------------------------------------------------------------------------------------------------------------
def test_dropin_infer_classes_is_the_engine_call(tiny, gold, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    from camouflaged_vlm_amd.engine import ClassHypotheses
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
        got = model.infer_classes(inp, ci, cm, topk=3)
        want = model.cascade().infer_classes(inp, ci, cm, topk=3)
        torch.cuda.synchronize()
        assert isinstance(got, ClassHypotheses) and same(got, want)
        with pytest.raises(AssertionError):
            model.infer_classes(inp[:, :, :g.inp_size - 16, :g.inp_size - 16], ci, cm, topk=1)
