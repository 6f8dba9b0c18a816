"""Encode images once, decode class prompts many times (Cascade.encode / Cascade.decode, SAM.encode_images / SAM.decode_classes;
DESIGN.md §11): the kernel behind the per-prompt expansion (cvlm_expand_blocks), `decode(encode(x))` against `infer_classes(x)` and
the cascade, parity against the reference's own K-prompt decoder call (tests/golden/tiny_classes.npz), survival of the encoded
state across other calls, image subsets, caller-supplied text rows against the CPU oracle (tests/session_oracle.py), the switches
and the refusals.  Gate (BASELINE.json north_star): 1e-3 abs on mask / edge / class logits, IoU >= 0.999, equal predictions."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_classes_gpu import BATCH_TOL, IOU, TOL, _order_matches, _topk_host, build_tiny, dmax, iou, same

pytestmark = pytest.mark.gpu

C5 = [[4, 0, 2, 2, 1], [3, 1, 0, 4, 2]]
FIELDS = ("masks", "edges", "logits", "pred")


def rows_equal(h, full, rows, fields=FIELDS + ("pass1_logits",)) -> bool:
    return all(torch.equal(getattr(h, f), getattr(full, f)[rows]) for f in fields)


# ---- kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("block_elems", [1, 5, 4099, 8200, 32004])
def test_expand_blocks_is_index_select(block_elems, shift):
    """P = 7 blocks out of B = 3 with repeats and one unused image; f32 only, h2 only, both; bases shifted by one element (no
    16-byte access possible); 4099 and 5 take the element path, 32 004 the vector path for f32 alone, 8200 for the planes too;
    more than one chunk of 4096 elements from 4099 on.  Bit-equal to torch.index_select, sentinels around every destination."""
    from camouflaged_vlm_amd import hip
    from camouflaged_vlm_amd.hip import H2
    dev = torch.device("cuda:0")
    P, B, n, PAD = 7, 3, block_elems, 64
    of = [2, 0, 2, 2, 0, 0, 2]                                # image 1 is never read
    image_of = torch.tensor(of, dtype=torch.int32, device=dev)
    idx = torch.tensor(of, dtype=torch.int64, device=dev)
    gen = torch.Generator().manual_seed(11 + block_elems)
    # bit patterns, not values: NaN payloads and subnormals must come through as they are
    src_f = torch.randint(-2 ** 31, 2 ** 31 - 1, (shift + B * n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).to(dev)
    src_h = torch.randint(-2 ** 15, 2 ** 15 - 1, (2, shift + B * n), generator=gen, dtype=torch.int64).to(torch.int16).view(torch.float16).to(dev)
    sf, sh = src_f[shift:], H2(src_h[:, shift:])
    want_f = sf.view(torch.int32).view(B, n).index_select(0, idx)
    want_h = sh.t.view(torch.int16).view(2, B, n).index_select(1, idx)
    SF, SH = -7.25, -3.5
    for mode in ("f32", "h2", "both"):
        dst_f = torch.full((shift + P * n + PAD,), SF, device=dev)
        dst_h = torch.full((2, shift + P * n + PAD), SH, dtype=torch.float16, device=dev)
        df, dh = dst_f[shift:], H2(dst_h[:, shift:])
        kw = {}
        if mode in ("f32", "both"):
            kw.update(src_f32=sf, dst_f32=df)
        if mode in ("h2", "both"):
            kw.update(src_h2=sh, dst_h2=dh)
        hip.expand_blocks(image_of, P, B, n, **kw)
        torch.cuda.synchronize()
        if mode == "h2":
            assert bool((dst_f == SF).all())
        else:
            assert torch.equal(df[:P * n].view(torch.int32).view(P, n), want_f), (mode, n, shift)
            assert bool((dst_f[:shift] == SF).all()) and bool((df[P * n:] == SF).all())
        if mode == "f32":
            assert bool((dst_h == SH).all())
        else:
            assert torch.equal(dh.t[:, :P * n].view(torch.int16).view(2, P, n), want_h), (mode, n, shift)
            assert bool((dst_h[:, :shift] == SH).all()) and bool((dh.t[:, P * n:] == SH).all())


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


@pytest.fixture(scope="module")
def cas(tiny, gold):
    """One tiny `exact` engine for the module.  (The K-split switches are read per launch in test processes, tests/conftest.py.)"""
    return build_tiny(tiny, gold)


@pytest.fixture
def nosplit(monkeypatch):
    """GEMM K-splits off: the summation order of a GEMM no longer depends on its row count."""
    monkeypatch.setenv("CVLM_GEMM_TAIL", "0")
    monkeypatch.setenv("CVLM_GEMM_SK", "0")


def test_decode_of_encode_has_the_bits_of_infer_classes_without_ksplits(tiny, cas, nosplit):
    _, _, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    want = cas.infer_classes(inp, ci, cm, classes=classes)
    got = cas.decode(cas.encode(inp, ci, cm), classes=classes)
    torch.cuda.synchronize()
    assert same(got, want)


def test_decode_of_encode_within_batch_tolerance_and_k1_is_the_cascade(tiny, cas):
    _, _, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    want = cas.infer_classes(inp, ci, cm, classes=classes)
    enc = cas.encode(inp, ci, cm)
    got = cas.decode(enc, classes=classes)
    torch.cuda.synchronize()
    worst = max(dmax(got.masks, want.masks), dmax(got.edges, want.edges), dmax(got.logits, want.logits),
                dmax(got.pass1_logits, want.pass1_logits))
    print(f"decode(encode(x)) vs infer_classes(x), default switches: {worst:.2e}")
    assert worst <= BATCH_TOL
    assert torch.equal(got.pred, want.pred) and torch.equal(got.classes, want.classes)
    # one prompt per image: every GEMM has the cascade's row count, so the bits are the cascade's
    m, p, l = (t.clone() for t in cas.cascade(inp, ci, cm, pipelined=False))
    h = cas.decode(enc, topk=1)
    torch.cuda.synchronize()
    assert torch.equal(h.masks[:, 0], m[:, 0]) and torch.equal(h.logits[:, 0], l) and torch.equal(h.pred[:, 0], p)
    assert torch.equal(h.classes[:, 0], enc.pass1_pred)


def test_tiny_session_matches_reference(tiny, cas, gold):
    g, c, _, (inp, ci, cm), dev = tiny
    classes = torch.from_numpy(gold["classes"])
    enc = cas.encode(inp, ci, cm)
    h = cas.decode(enc, classes=classes.to(dev))
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
    print("tiny session vs reference (exact):", {k: f"{v:.2e}" for k, v in rep.items()})
    for b in range(B):
        for k in range(K):
            print(f"  tiny image {b} class {int(classes[b, k])}: mask {dmax(h.masks[b, k], ref_m[b, k]):.2e} edge "
                  f"{dmax(h.edges[b, k], ref_e[b, k]):.2e} stage-2 logits {dmax(h.logits[b, k], gold['class_logits'][b, k]):.2e}")
    for k in ("masks", "masks_at_pos", "edges", "pass1_logits", "stage2_logits"):
        assert rep[k] <= TOL, rep
    assert rep["min_iou"] >= IOU and h.pred.tolist() == gold["pred"].tolist()
    # topk: the engine's own pass-1 order, which is the golden's wherever adjacent golden logits are more than 1e-3 apart
    t = cas.decode(enc, topk=K)
    torch.cuda.synchronize()
    p1 = t.pass1_logits.cpu().numpy()
    for b in range(B):
        assert t.classes[b].tolist() == _topk_host(p1[b], K)
    _order_matches(t.classes, gold["classes"], gold["pass1_logits"])


def test_encoded_images_survive_other_calls(tiny, cas):
    """Workspace growth, a pipelined batch that owes its stage 2 and `infer_test`, all on other inputs, leave the session as it was;
    `decode` pays the pipelined batch's debt first."""
    _, c, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    inp2, ci2, cm2 = inp.flip(0).contiguous(), ci.flip(0).contiguous(), cm.flip(0).contiguous()
    want_m, want_p, want_l = (t.clone() for t in cas.cascade(inp2, ci2, cm2, pipelined=False))
    enc = cas.encode(inp, ci, cm)
    first = cas.decode(enc, classes=classes)
    first = {f: getattr(first, f).clone() for f in FIELDS + ("classes", "pass1_logits")}
    cas.infer_classes(inp2, ci2, cm2, classes=torch.randint(0, c.n_cls_test, (2, 9), device=dev))   # 18 prompts: the workspace grows
    masks, pred, logits = cas.cascade(inp2, ci2, cm2, pipelined=True)                                # stage 2 owed
    cas.infer_test(inp2, ci2, cm2)                                                                   # (flushes; nothing owed afterwards)
    masks, pred, logits = cas.cascade(inp2, ci2, cm2, pipelined=True)                                # owed again, when decode comes
    again = cas.decode(enc, classes=classes)
    torch.cuda.synchronize()
    for f, t in first.items():
        assert torch.equal(getattr(again, f), t), f
    assert torch.equal(masks, want_m) and torch.equal(pred, want_p) and torch.equal(logits, want_l)
    cas.flush()                                                                                      # nothing left to do
    torch.cuda.synchronize()
    assert torch.equal(pred, want_p) and torch.equal(logits, want_l)


def test_image_subsets_have_the_rows_of_the_full_decode(tiny, cas, nosplit):
    _, _, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    enc = cas.encode(inp, ci, cm)
    full = cas.decode(enc, classes=classes)
    full_t = cas.decode(enc, topk=3)
    for images in ([1], [1, 1, 0]):
        h = cas.decode(enc, classes=classes[images], images=images)
        t = cas.decode(enc, topk=3, images=images)
        torch.cuda.synchronize()
        assert h.masks.shape[0] == len(images) and h.classes.tolist() == classes[images].tolist()
        assert rows_equal(h, full, images), images
        assert rows_equal(t, full_t, images, FIELDS + ("pass1_logits", "classes")), images


def test_text_rows(tiny, cas, gold):
    from oracle import cvlm_oracle as O
    import session_oracle as SO
    g, c, sd_np, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    enc = cas.encode(inp, ci, cm)
    bank_rows = cas.clip.txt["test"]
    want = cas.decode(enc, classes=classes)
    got = cas.decode(enc, text=bank_rows[classes.to(dev)])
    torch.cuda.synchronize()
    assert got.classes is None and all(torch.equal(getattr(got, f), getattr(want, f)) for f in FIELDS)
    # rows no class of the bank has: the mean of two bank rows, 2 images x K = 2, against the CPU oracle on the same rows
    rows = bank_rows.cpu()
    text = torch.stack([torch.stack([(rows[0] + rows[3]) / 2, (rows[1] + rows[4]) / 2]),
                        torch.stack([(rows[2] + rows[0]) / 2, (rows[4] + rows[3]) / 2])])
    h = cas.decode(enc, text=text)
    torch.cuda.synchronize()
    sd = O.to_torch_sd(sd_np)
    with torch.no_grad():
        tf = O.clip_text_features(sd, c, gold["eot_test"].tolist())
        r = SO.decode_text(inp.cpu(), ci.cpu(), cm.cpu(), sd, g, c, tf, torch.from_numpy(gold["bank_test"]), text)
    rep = {"masks": dmax(h.masks, r["masks"]), "edges": dmax(h.edges, r["edges"]), "stage2_logits": dmax(h.logits, r["logits"]),
           "pass1_logits": dmax(h.pass1_logits, r["pass1_logits"]),
           "min_iou": min(iou(h.masks[b, k].cpu(), r["masks"][b, k]) for b in range(2) for k in range(2))}
    print("tiny session, mean-of-two text rows vs CPU oracle (exact):", {k: f"{v:.2e}" for k, v in rep.items()})
    for k in ("masks", "edges", "stage2_logits", "pass1_logits"):
        assert rep[k] <= TOL, rep
    assert rep["min_iou"] >= IOU and h.pred.tolist() == r["pred"].tolist() and h.classes is None


def test_stage2_off_launches_no_encoder_and_no_clip(tiny, cas, monkeypatch):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    enc = cas.encode(inp, ci, cm)
    want = cas.decode(enc, classes=classes)
    torch.cuda.synchronize()
    calls = {"attention": 0, "patchify": 0}
    for name in calls:
        real = getattr(hip, name)

        def counted(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(hip, name, counted)
    got = cas.decode(enc, classes=classes, stage2=False)
    torch.cuda.synchronize()
    assert calls == {"attention": 0, "patchify": 0}            # both the SAM encoder and the CLIP tower start with cvlm_patchify
    assert got.logits is None and got.pred is None
    assert torch.equal(got.masks, want.masks) and torch.equal(got.edges, want.edges) and torch.equal(got.classes, want.classes)
    cas.decode(enc, classes=classes)                           # the counters do count: stage 2 is a CLIP forward
    assert calls["attention"] > 0 and calls["patchify"] > 0


def test_quality_is_infer_classes_quality(tiny, cas, nosplit):
    _, _, _, (inp, ci, cm), dev = tiny
    classes = torch.tensor(C5, dtype=torch.int64)
    want = cas.infer_classes(inp, ci, cm, classes=classes, quality=True)
    got = cas.decode(cas.encode(inp, ci, cm), classes=classes, quality=True)
    torch.cuda.synchronize()
    assert got.iou.shape == (2, 5) and torch.equal(got.iou, want.iou) and same(got, want)
    assert cas.decode(cas.encode(inp, ci, cm), classes=classes).iou is None


def test_bad_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, c, _, (inp, ci, cm), dev = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    D = cas.clip.txt["test"].shape[1]
    n_cls = c.n_cls_test
    ok = torch.zeros(2, 2, dtype=torch.int64)
    bad = [dict(), dict(topk=2, classes=ok), dict(topk=2, text=torch.zeros(2, 2, D)), dict(classes=ok, text=torch.zeros(2, 2, D)),
           dict(topk=0), dict(topk=n_cls + 1), dict(topk=1.0),
           dict(classes=ok.int()), dict(classes=torch.zeros(3, 2, dtype=torch.int64)), dict(classes=torch.zeros(2, dtype=torch.int64)),
           dict(classes=torch.zeros(2, 0, dtype=torch.int64)), dict(classes=torch.tensor([[0, n_cls], [0, 0]])),
           dict(classes=torch.tensor([[0, -1], [1, 1]], device=dev)), dict(classes=[[0, 1], [1, 0]]),
           dict(text=torch.zeros(2, 2, D, dtype=torch.float64)), dict(text=torch.zeros(2, 2, D + 4)), dict(text=torch.zeros(3, 2, D)),
           dict(text=torch.zeros(2, D)), dict(text=torch.zeros(2, 0, D, device=dev)),
           dict(topk=1, images=[]), dict(topk=1, images=[2]), dict(topk=1, images=[-1]), dict(topk=1, images=torch.tensor([0], device=dev)),
           dict(classes=ok, images=[0]), dict(text=torch.zeros(2, 2, D), images=[0, 1, 0])]
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "add_rows", "small_attention", "bilinear",
             "attention")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in bad:
            with pytest.raises(ValueError):
                cas.decode(enc, **kw)
        with pytest.raises(ValueError):                        # images another engine encoded
            cas.decode(dataclasses.replace(enc, engine=object()), topk=1)
        with pytest.raises(ValueError):
            cas.decode((inp, ci, cm), topk=1)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []
    h = cas.decode(enc, topk=1)                                # the session is still good
    torch.cuda.synchronize()
    assert torch.equal(h.classes[:, 0], enc.pass1_pred)


# ---- drop-in ------------------------------------------------------------------------------------------------------------------
def test_dropin_session_is_the_engine_call(tiny, gold, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    from camouflaged_vlm_amd.engine import ClassHypotheses, EncodedImages
    g, c, sd_np, (inp, ci, cm), dev = tiny
    with np.load(os.path.join(golden_dir, "tiny_cascade.npz")) as z:
        eot_train = z["eot_train"].tolist()
    clip = CustomCLIP(geometry=c, eot_train=eot_train, eot_test=gold["eot_test"].tolist())
    enc_cfg = dict(name="sam", img_size=g.inp_size, mlp_ratio=4, patch_size=16, qkv_bias=True, use_rel_pos=True,
                   window_size=14, out_chans=256, scale_factor=32, input_type="fft", freq_nums=0.25, prompt_type="highpass",
                   prompt_embed_dim=256, tuning_stage=1234, handcrafted_tune=True, embedding_tune=True, adaptor="adaptor",
                   embed_dim=g.embed_dim, depth=g.depth, num_heads=g.num_heads, global_attn_indexes=list(g.global_attn_indexes))
    model = models.make({"name": "sam_maskdecoder_edge", "args": {"inp_size": g.inp_size, "loss": "iou", "encoder_mode": enc_cfg}}).cuda()
    model.train_text_features = model.train_text_features[:c.n_cls_train]
    model.test_text_features = model.test_text_features[:c.n_cls_test]
    model.load_mapleAlphaCLIP(clip)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    model.eval()
    with torch.no_grad():
        enc = model.encode_images(inp, ci, cm)
        got = model.decode_classes(enc, topk=3)
        want = model.cascade().decode(model.cascade().encode(inp, ci, cm), topk=3)
        sub = model.decode_classes(enc, topk=2, images=[1], stage2=False)
        torch.cuda.synchronize()
        assert isinstance(enc, EncodedImages) and enc.engine is model.cascade() and enc.B == 2
        assert isinstance(got, ClassHypotheses) and same(got, want)
        assert sub.logits is None and sub.masks.shape[:2] == (1, 2) and torch.equal(sub.classes[0], got.classes[1, :2])
        assert dmax(sub.masks[0], got.masks[1, :2]) <= BATCH_TOL     # two prompts against six: other GEMM row counts
        with pytest.raises(AssertionError):
            model.encode_images(inp[:, :, :g.inp_size - 16, :g.inp_size - 16], ci, cm)
