"""Class vocabularies at run time: the three kernels behind them (cvlm_text_assemble, cvlm_clip_head_wide,
cvlm_topk_select_wide) against torch / fp64 / the entries they extend, ClipModel.make_vocabulary's bits, the 1100-class vocabulary
against the reference's own run (tests/golden/tiny_vocab.npz, tools/make_vocab_golden.py), sessions, `use_vocabulary` and the
drop-in surface.  Gates as tests/test_classes_gpu.py: 1e-3 abs on mask / edge / class logits, IoU >= 0.999, equal predictions."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, IOU = 1e-3, 0.999
BATCH_TOL = 6e-5            # a batch against its single forwards with the GEMM K-splits on (tests/test_cascade_gpu.py)
DEV = "cuda:0"


def dmax(a, b) -> float:
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def relerr(got, ref) -> float:
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def iou(a, b) -> float:
    a, b = torch.as_tensor(a) > 0, torch.as_tensor(b) > 0
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def same(x, y) -> bool:
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in ("classes", "pass1_logits", "masks", "edges", "logits", "pred"))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def scan(row) -> int:
    """cvlm_clip_head's prediction: the sequential strict-`>` scan from class 0."""
    best = 0
    for c in range(1, len(row)):
        if row[c] > row[best]:
            best = c
    return best


def head(fn_name, img, txt, **kw):
    from camouflaged_vlm_amd import hip
    P, D = img.shape
    C = txt.shape[0]
    img_n, logits = torch.full((P, D), -7.0, device=DEV), torch.full((P, C), -7.0, device=DEV)
    pred, sel = torch.full((P,), -7, dtype=torch.int64, device=DEV), torch.full((P, D), -7.0, device=DEV)
    if fn_name == "wide":
        ws = torch.empty(hip.clip_head_wide_workspace_bytes(P, C), dtype=torch.uint8, device=DEV)
        hip.clip_head_wide(img.to(DEV), txt.to(DEV), 100.0, P, C, D, img_n, logits, pred, sel, ws)
    else:
        hip.clip_head(img.to(DEV), txt.to(DEV), 100.0, P, C, D, img_n, logits, pred, sel)
    torch.cuda.synchronize()
    return img_n, logits, pred, sel


def head_inputs(P, C, D=768):
    """Seeded so that the fp64 top-2 gap of every image exceeds 1e-3 (checked on the CPU when this test was written: the smallest
    is 0.65, at P = 17, C = 1025; the text rows are not normalised, |logits| reach 500)."""
    return rnd(P, D, seed=1000 + 7 * P + C), rnd(C, D, seed=2000 + 7 * P + C)


# ---- kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [9, 77])
def test_text_assemble_is_the_torch_expression(L):
    from camouflaged_vlm_amd import hip
    n, CL, W, V, n_ctx = 3, 77, 64, 11, 4
    table, ctx, pos = rnd(V, W, seed=1).to(DEV), rnd(n_ctx, W, seed=2).to(DEV), rnd(CL, W, seed=3).to(DEV)
    ids = torch.randint(0, V, (n, CL), generator=torch.Generator().manual_seed(4), dtype=torch.int32).to(DEV)
    emb = table[ids.long()].contiguous()
    full = torch.cat([emb[:, :1], ctx.unsqueeze(0).expand(n, -1, -1), emb[:, 1 + n_ctx:]], 1)[:, :L].contiguous()
    want = full + pos[:L]
    via_add_rows = torch.empty(n, L, W, device=DEV)                # what ClipModel.text_features launches
    hip.add_rows(full, pos[:L].contiguous(), L, n * L, W, out_f32=via_add_rows)
    # form 2 ignores positions 1..n_ctx of the embeddings
    emb2 = emb.clone()
    emb2[:, 1:1 + n_ctx] = float("nan")
    got1, got2 = torch.full((n, L, W), -7.0, device=DEV), torch.full((n, L, W), -7.0, device=DEV)
    hip.text_assemble(ids, table, None, ctx, pos[:L].contiguous(), n, CL, L, W, got1)
    hip.text_assemble(None, None, emb2, ctx, pos[:L].contiguous(), n, CL, L, W, got2)
    torch.cuda.synchronize()
    assert torch.equal(want, via_add_rows)
    assert torch.equal(got1, want) and torch.equal(got2, want)


@pytest.mark.parametrize("P,C,D", [(3, 61, 768), (17, 1024, 768), (1, 5, 8)])
def test_wide_head_has_the_bits_of_clip_head(P, C, D):
    img, txt = rnd(P, D, seed=11 + C), rnd(C, D, seed=12 + C)
    a, b = head("wide", img, txt), head("head", img, txt)
    for name, x, y in zip(("img_n", "logits", "pred", "txt_sel"), a, b):
        print(f"wide head vs cvlm_clip_head ({P}, {C}, {D}) {name}: max |diff| {dmax(x, y):.2e}")
    for name, x, y in zip(("img_n", "logits", "pred", "txt_sel"), a, b):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("C", [1025, 2500])
@pytest.mark.parametrize("P", [1, 17])
def test_wide_head_against_fp64(P, C):
    img, txt = head_inputs(P, C)
    img_n, logits, pred, sel = head("wide", img, txt)
    n = img.double() / img.double().norm(dim=-1, keepdim=True)
    rl = 100.0 * n @ txt.double().t()
    top2 = rl.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    e_n, e_l = relerr(img_n, n), relerr(logits, rl)
    print(f"wide head vs fp64 (P = {P}, C = {C}): img_n {e_n:.2e}, logits {e_l:.2e}, smallest fp64 top-2 gap {gap:.2e}")
    assert gap > 1e-3
    assert e_n < 1e-6 and e_l < 3e-6                               # the bounds of tests/test_ops_gpu.py's clip-head case
    assert pred.cpu().tolist() == rl.argmax(1).tolist() and torch.equal(sel.cpu(), txt[rl.argmax(1)])


@pytest.mark.parametrize("C", [1025, 2500])
def test_wide_head_ties_and_nans(C):
    """Class tiles are 4 classes wide at C = 1025 and 8 at C = 2500: class 8 opens a tile in both, 13 and 900 lie in different tiles."""
    P, D = 5, 768
    img, txt = head_inputs(P, C)
    txt[900] = txt[13]                                             # equal rows: bit-equal logits
    img[0] = txt[13] * 4.0                                         # image 0's maximum is the tie 13 / 900
    clean = head("wide", img, txt)
    lg = clean[1].cpu().numpy()
    assert lg[0, 13] == lg[0, 900] == lg[0].max()
    print(f"ties (C = {C}): pred {clean[2].tolist()}, host scan {[scan(r) for r in lg]}")
    assert clean[2].tolist() == [scan(r) for r in lg] and clean[2][0].item() == 13
    assert torch.equal(clean[3].cpu(), txt[clean[2].cpu()])
    # NaN at class 0: nothing compares greater than a NaN -> 0 for every image
    t0 = txt.clone()
    t0[0, 5] = float("nan")
    _, l0, p0, s0 = head("wide", img, t0)
    assert bool(torch.isnan(l0[:, 0]).all()) and p0.tolist() == [0] * P
    assert torch.equal(torch.nan_to_num(s0.cpu(), nan=-1.0), torch.nan_to_num(t0[0].expand(P, D), nan=-1.0))
    # NaN at the first class of a later tile -- the tile of image 1's maximum, moved there -- and a finite maximum elsewhere
    t8 = txt.clone()
    t8[8, 5] = float("nan")
    t8[9] = img[1] * 4.0                                           # image 1's maximum sits in the tile the NaN opens
    _, l8, p8, s8 = head("wide", img, t8)
    l8h = l8.cpu().numpy()
    want = [int(np.nanargmax(r)) for r in l8h]
    print(f"NaN at class 8 (C = {C}): pred {p8.tolist()}, first maximum of the rest {want}")
    assert bool(torch.isnan(l8[:, 8]).all()) and p8.tolist() == want == [scan(r) for r in l8h] and want[1] == 9 and want[0] == 13
    assert torch.equal(s8.cpu(), t8[p8.cpu()])
    # an all-NaN row (a NaN in the image) gives 0 and leaves the other images alone
    im = img.clone()
    im[2, 100] = float("nan")
    n2, l2, p2, s2 = head("wide", im, txt)
    assert bool(torch.isnan(l2[2]).all()) and p2[2].item() == 0 and torch.equal(s2[2].cpu(), txt[0])
    keep = [0, 1, 3, 4]
    for x, y in zip((n2, l2, p2, s2), clean):
        assert torch.equal(x[keep], y[keep])


@pytest.mark.parametrize("C", [1025, 2500])
def test_topk_select_wide_against_stable_sort(C):
    from camouflaged_vlm_amd import hip
    B, D = 6, 768
    img, txt = head_inputs(B, C)
    _, logits, pred, _ = head("wide", img, txt)
    txt_d = txt.to(DEV)
    lg = logits.clone()
    top = float(lg[2].max()) + 1.0
    lg[2, 1024] = top                                              # exact ties at the top, across tiles and 256-class strides
    lg[2, 5] = top
    lg[2, 261] = top
    lg[3, 700:720] = lg[3, 40]                                     # a run of equal values in the middle of the order
    lg[5, C - 1] = float("-inf")
    lg[5, 0] = float("inf")
    lg[4, 1024] = float("nan")                                     # a NaN row
    for K in (1, 5, 64):
        idx = torch.full((B, K), -7, dtype=torch.int64, device=DEV)
        sel = torch.full((B, K, D), -7.0, device=DEV)
        hip.topk_select_wide(lg, B, C, K, txt_d, D, None, idx, sel)
        torch.cuda.synchronize()
        want = torch.sort(lg.cpu(), dim=1, descending=True, stable=True).indices[:, :K]
        ok = [b for b in range(B) if b != 4]
        print(f"topk wide C = {C} K = {K}: row 2 {idx[2, :min(K, 5)].tolist()} (stable sort {want[2, :min(K, 5)].tolist()})")
        assert torch.equal(idx.cpu()[ok], want[ok])
        assert torch.equal(sel[ok], txt_d[idx[ok]])               # the gather is bit for bit
        assert idx[4].tolist() == [-1] * K and bool(torch.isnan(sel[4]).all())
        if K >= 3:
            assert idx[2, :3].tolist() == [5, 261, 1024]
    # slot 0 is the wide head's prediction on finite rows
    idx = torch.empty(B, 1, dtype=torch.int64, device=DEV)
    sel = torch.empty(B, 1, D, device=DEV)
    hip.topk_select_wide(logits, B, C, 1, txt_d, D, None, idx, sel)
    torch.cuda.synchronize()
    assert idx[:, 0].tolist() == pred.tolist()


# ---- tiny geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def vgold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_vocab.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device(DEV)
    return g, c, sd_np, tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


def build_tiny(tiny, gold):
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c, sd_np, _, dev = tiny
    cas = Cascade({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, c, dev, Precision.named("exact"))
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), torch.from_numpy(gold["bank_test"]), "test")
    return cas


@pytest.fixture(scope="module")
def cas(tiny, gold):
    """One tiny `exact` engine for the module.  (The K-split switches are read per launch in test processes, tests/conftest.py.)"""
    return build_tiny(tiny, gold)


@pytest.fixture(scope="module")
def big_inputs(tiny, vgold):
    """(tokens (N, 77) int32, the token-embedding table on the device, bank (N, D)) of tiny_vocab.npz's 1100 classes."""
    from camouflaged_vlm_amd import synth
    _, c, _, _, dev = tiny
    N = int(vgold["n_cls"])
    tokens = np.zeros((N, c.context_length), np.int32)
    tokens[:, :vgold["tokens"].shape[1]] = vgold["tokens"]
    table = torch.from_numpy(synth.make_tensor("openai.token_embedding.weight", (49408, c.text_width), "embed", 0)).to(dev)
    return tokens, table, torch.from_numpy(synth.make_text_bank(N, c.embed_dim, "test"))


@pytest.fixture(scope="module")
def big(cas, big_inputs):
    """The 1100-class vocabulary on the module's engine."""
    tokens, table, bank = big_inputs
    return cas.make_vocabulary(tokens=tokens, table=table, bank=bank, name="ovcamo pairs")


@pytest.fixture
def nosplit(monkeypatch):
    """GEMM K-splits off: the summation order of a GEMM no longer depends on its row count."""
    monkeypatch.setenv("CVLM_GEMM_TAIL", "0")
    monkeypatch.setenv("CVLM_GEMM_SK", "0")


def own_vocabulary(cas, tiny, gold):
    """The constructor's own test prompts as a vocabulary: embeddings = [prefix | anything | suffix], same eot, same bank."""
    _, c, _, _, dev = tiny
    pre, suf = cas.clip.prefix["test"], cas.clip.suffix["test"]
    emb = torch.cat([pre, torch.full((pre.shape[0], c.n_ctx, c.text_width), float("nan"), device=dev), suf], 1)
    return cas.make_vocabulary(embeddings=emb, eot=gold["eot_test"].tolist(), bank=torch.from_numpy(gold["bank_test"]))


def test_vocabulary_of_the_constructors_prompts_is_the_constructors_bank(tiny, cas, gold):
    from camouflaged_vlm_amd.engine import Vocabulary
    _, c, _, (inp, ci, cm), dev = tiny
    v = own_vocabulary(cas, tiny, gold)
    torch.cuda.synchronize()
    assert isinstance(v, Vocabulary) and (v.n, v.D) == (c.n_cls_test, c.embed_dim) and v.eot == gold["eot_test"].tolist()
    assert v.engine is cas.clip
    print(f"rows of the constructor's prompts as a vocabulary vs txt['test']: max |diff| {dmax(v.rows, cas.clip.txt['test']):.2e}")
    assert torch.equal(v.rows, cas.clip.txt["test"])
    want = cas.infer_classes(inp, ci, cm, topk=3)
    got = cas.infer_classes(inp, ci, cm, topk=3, vocab=v)
    torch.cuda.synchronize()
    assert same(got, want)
    assert torch.equal(cas.infer_test(inp, ci, cm, vocab=v), cas.infer_test(inp, ci, cm))
    a, b = cas.infer_test_multimask(inp, ci, cm, vocab=v), cas.infer_test_multimask(inp, ci, cm)
    assert torch.equal(a.masks, b.masks) and torch.equal(a.iou, b.iou)


def test_rows_do_not_depend_on_chunk_or_input_form(tiny, cas, big_inputs):
    tokens, table, bank = big_inputs
    tok, bk = tokens[:40], bank[:40].contiguous()
    a = cas.make_vocabulary(tokens=tok, table=table, bank=bk, chunk=16)
    b = cas.make_vocabulary(tokens=tok, table=table, bank=bk, chunk=64)
    e = cas.make_vocabulary(embeddings=table[torch.from_numpy(tok).long().to(table.device)], eot=tok.argmax(-1), bank=bk, chunk=7)
    h = cas.make_vocabulary(tokens=tok, table=table.cpu(), chunk=64)          # a host table is uploaded; no bank: no add
    torch.cuda.synchronize()
    print(f"40 prompts: chunk 16 vs 64 {dmax(a.rows, b.rows):.2e}, tokens vs embeddings {dmax(a.rows, e.rows):.2e}")
    assert torch.equal(a.rows, b.rows) and torch.equal(a.text_features, b.text_features)
    assert torch.equal(a.rows, e.rows) and torch.equal(a.text_features, e.text_features)
    assert torch.equal(h.text_features, b.text_features)
    from camouflaged_vlm_amd import hip
    plain = torch.empty_like(h.rows)
    hip.normalize_add(b.text_features, None, 40, b.D, plain)
    torch.cuda.synchronize()
    assert torch.equal(h.rows, plain)
    assert a.eot == tok.argmax(-1).tolist()


def test_1100_class_vocabulary_matches_reference(tiny, cas, big, vgold):
    g, c, _, (inp, ci, cm), dev = tiny
    N = int(vgold["n_cls"])
    assert big.n == N and big.rows.shape == (N, c.embed_dim)
    d_rows = dmax(big.rows[torch.from_numpy(vgold["row_idx"]).to(dev)], vgold["rows"])
    print(f"1100-class vocabulary: sampled text rows vs reference {d_rows:.2e}")
    assert d_rows <= 1e-4                                          # test_engine_matches_reference_golden's bound on tap_clip_text
    classes = torch.from_numpy(vgold["classes"])
    h = cas.infer_classes(inp, ci, cm, classes=classes.to(dev), vocab=big)
    torch.cuda.synchronize()
    B, K = classes.shape
    S = g.inp_size
    assert h.masks.shape == (B, K, S, S) and h.pass1_logits.shape == (B, N) and h.logits.shape == (B, K, N)
    ref_m = F.interpolate(torch.from_numpy(vgold["low_masks"]), (S, S), mode="bilinear", align_corners=False)
    ref_e = F.interpolate(torch.from_numpy(vgold["low_edges"]), (S, S), mode="bilinear", align_corners=False)
    dpos = dmax(h.masks.reshape(B, K, -1)[:, :, torch.from_numpy(vgold["pos"]).to(dev)], vgold["masks_at_pos"])
    rep = {"masks": dmax(h.masks, ref_m), "masks_at_pos": dpos, "edges": dmax(h.edges, ref_e),
           "pass1_logits": dmax(h.pass1_logits, vgold["pass1_logits"]), "stage2_logits": dmax(h.logits, vgold["class_logits"]),
           "min_iou": min(iou(h.masks[b, k].cpu(), ref_m[b, k]) for b in range(B) for k in range(K))}
    print("1100-class vocabulary vs reference (exact):", {k: f"{v:.2e}" for k, v in rep.items()})
    for k in ("masks", "masks_at_pos", "edges", "pass1_logits", "stage2_logits"):
        assert rep[k] <= TOL, rep
    assert rep["min_iou"] >= IOU and h.pred.tolist() == vgold["pred"].tolist()
    # topk through both wide kernels: the fixture's eight leading classes, all of them (its top nine are >= 1e-3 apart)
    t = cas.infer_classes(inp, ci, cm, topk=8, vocab=big)
    torch.cuda.synchronize()
    print("topk=8:", t.classes.tolist(), "fixture:", vgold["top8"].tolist())
    assert t.classes.tolist() == vgold["top8"].tolist()
    assert torch.equal(t.pass1_logits, h.pass1_logits) and torch.equal(t.classes[:, 0], t.pass1_logits.argmax(1))
    with pytest.raises(ValueError):
        cas.infer_classes(inp, ci, cm, topk=65, vocab=big)


def test_sessions_with_a_vocabulary(tiny, cas, big, nosplit):
    _, _, _, (inp, ci, cm), dev = tiny
    want = cas.infer_classes(inp, ci, cm, topk=2, vocab=big)
    enc = cas.encode(inp, ci, cm, vocab=big)
    got = cas.decode(enc, topk=2)
    torch.cuda.synchronize()
    assert enc.vocab is big and enc.pass1_features.shape == (2, big.D)
    assert same(got, want)
    # images encoded on the constructor's bank, decoded against the vocabulary: pass 1 re-scored from the kept features
    enc0 = cas.encode(inp, ci, cm)
    assert enc0.vocab is None and enc0.pass1_logits.shape == (2, cas.clip.txt["test"].shape[0])
    got0 = cas.decode(enc0, topk=2, vocab=big)
    torch.cuda.synchronize()
    print(f"decode(enc0, vocab=v) vs decode(encode(vocab=v)): masks {dmax(got0.masks, got.masks):.2e}, logits {dmax(got0.logits, got.logits):.2e}")
    assert torch.equal(got0.pass1_logits, enc.pass1_logits)
    assert same(got0, got)
    # and back: the vocabulary's session against the constructor's bank needs an explicit vocabulary; the default is enc.vocab
    d0 = cas.decode(enc0, topk=2)
    assert d0.pass1_logits.shape == enc0.pass1_logits.shape and torch.equal(d0.pass1_logits, enc0.pass1_logits)


def test_use_vocabulary(tiny, cas, big, gold):
    _, _, _, (inp, ci, cm), dev = tiny
    before = [t.clone() for t in cas.cascade(inp, ci, cm)]
    want = [t.clone() for t in cas.cascade(inp, ci, cm, pipelined=False, vocab=big)]
    try:
        cas.use_vocabulary(big)
        masks, pred, logits = cas.cascade(inp, ci, cm, pipelined=True)
        cas.flush()
        torch.cuda.synchronize()
        print(f"use_vocabulary: pipelined vs cascade(vocab=): masks {dmax(masks, want[0]):.2e}, logits {dmax(logits, want[2]):.2e}")
        assert logits.shape == (2, big.n)
        assert dmax(masks, want[0]) < BATCH_TOL and dmax(logits, want[2]) < BATCH_TOL and torch.equal(pred, want[1])
        dflt = cas.infer_classes(inp, ci, cm, topk=1)              # every entry point takes the default
        assert dflt.pass1_logits.shape == (2, big.n)
        with pytest.raises(ValueError):
            cas.cascade(inp, ci, cm, pipelined=True, vocab=big)
    finally:
        cas.use_vocabulary(None)
    after = cas.cascade(inp, ci, cm)
    torch.cuda.synchronize()
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    # a vocabulary of another engine is refused everywhere
    other = build_tiny(tiny, gold)
    foreign = own_vocabulary(other, tiny, gold)
    enc = cas.encode(inp, ci, cm)
    for call in (lambda: cas.use_vocabulary(foreign), lambda: cas.infer_test(inp, ci, cm, vocab=foreign),
                 lambda: cas.infer_test_multimask(inp, ci, cm, vocab=foreign), lambda: cas.infer_classes(inp, ci, cm, topk=1, vocab=foreign),
                 lambda: cas.encode(inp, ci, cm, vocab=foreign), lambda: cas.decode(enc, topk=1, vocab=foreign),
                 lambda: cas.cascade(inp, ci, cm, vocab=foreign), lambda: cas.stage2(before[0], ci, vocab=foreign),
                 lambda: cas.clip.forward(ci, cm, vocab=foreign)):
        with pytest.raises(ValueError):
            call()


# ---- drop-in ------------------------------------------------------------------------------------------------------------------
def test_dropin_vocabulary_is_the_engine_call(tiny, gold, vgold, big_inputs, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    from camouflaged_vlm_amd.engine import ClassHypotheses
    g, c, sd_np, (inp, ci, cm), dev = tiny
    tokens, table, bank = big_inputs
    tok, bk = tokens[:1030], bank[:1030].contiguous()
    with np.load(os.path.join(golden_dir, "tiny_cascade.npz")) as z:
        eot_train = z["eot_train"].tolist()
    clip = CustomCLIP(geometry=c, eot_train=eot_train, eot_test=gold["eot_test"].tolist())
    n_keys = len(clip.state_dict())
    clip.set_token_embedding(table.cpu())
    assert len(clip.state_dict()) == n_keys                        # a plain attribute: the state_dict keys stay the reference's
    enc = dict(name="sam", img_size=g.inp_size, mlp_ratio=4, patch_size=16, qkv_bias=True, use_rel_pos=True,
               window_size=14, out_chans=256, scale_factor=32, input_type="fft", freq_nums=0.25, prompt_type="highpass",
               prompt_embed_dim=256, tuning_stage=1234, handcrafted_tune=True, embedding_tune=True, adaptor="adaptor",
               embed_dim=g.embed_dim, depth=g.depth, num_heads=g.num_heads, global_attn_indexes=list(g.global_attn_indexes))
    model = models.make({"name": "sam_maskdecoder_edge", "args": {"inp_size": g.inp_size, "loss": "iou", "encoder_mode": enc}}).cuda()
    model.train_text_features = model.train_text_features[:c.n_cls_train]
    model.test_text_features = model.test_text_features[:c.n_cls_test]
    model.load_mapleAlphaCLIP(clip)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    with torch.no_grad():
        v = model.make_vocabulary(tokens=tok, bank=bk, name="pairs")   # the kept table
        got = model.infer_classes(inp, ci, cm, topk=2, vocab=v)
        want = model.cascade().infer_classes(inp, ci, cm, topk=2, vocab=v)
        torch.cuda.synchronize()
        assert isinstance(got, ClassHypotheses) and same(got, want) and got.pass1_logits.shape == (2, 1030)
        _, _, p, lg = model.clip_model(ci, cm, train=False, vocab=v)
        assert torch.equal(lg, got.pass1_logits) and torch.equal(p, got.classes[:, 0])
        e = model.encode_images(inp, ci, cm, vocab=v)
        dd = model.decode_classes(e, topk=2)
        assert torch.equal(dd.classes, got.classes)
        model.use_vocabulary(v)
        assert model.infer_classes(inp, ci, cm, topk=1).pass1_logits.shape == (2, 1030)
        model.use_vocabulary(None)
        assert model.infer_classes(inp, ci, cm, topk=1).pass1_logits.shape == (2, c.n_cls_test)
        with pytest.raises(AssertionError):
            model.infer_classes(inp[:, :, :g.inp_size - 16, :g.inp_size - 16], ci, cm, topk=1, vocab=v)
        # a weight load drops the engines: the vocabulary made before it is refused
        model.load_state_dict(sd, strict=True)
        for call in (lambda: model.infer_classes(inp, ci, cm, topk=1, vocab=v), lambda: model.infer_test(inp, ci, cm, vocab=v),
                     lambda: model.use_vocabulary(v), lambda: model.encode_images(inp, ci, cm, vocab=v),
                     lambda: model.clip_model(ci, cm, train=False, vocab=v)):
            with pytest.raises(RuntimeError):
                call()
