"""Instances on the device: cvlm_mask_regions_sized == its host twin == the oracle (tests/regions_oracle.py) on every
hand-made plane as ONE ragged call, every output pre-filled with garbage, again with exactly the minimum workspace so that rounds run,
and with set pad bits; cvlm_region_alpha against the fp64 oracle at R = 56 and R = 336; the tiny engine through pack_masks_sized ->
mask_regions_sized -> compact -> classify_regions against single CLIP forwards.  Bits, tables and counts are exact."""
import os

import numpy as np
import pytest
import torch

pytest.importorskip("scipy.ndimage")
import regions_oracle as GO  # noqa: E402
import rowops_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH_TOL = 6e-5            # a batch against its single forwards with the GEMM K-splits on (tests/test_cascade_gpu.py)
ALL = [p for _, p in GO.planes()]
DEV = "cuda:0"


def dmax(a, b) -> float:
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


# ---- cvlm_mask_regions_sized -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity,M,min_area", [(8, 5, 0), (4, 5, 4), (4, 64, 1), (8, 1, 0)])
def test_device_equals_host_entry_equals_oracle(connectivity, M, min_area):
    from camouflaged_vlm_amd import hip
    want = GO.expected(connectivity, M, min_area)
    GO.same(GO.run(hip.mask_regions_sized_host, ALL, connectivity, M, min_area), want)
    _, off, max_words = GO.tables([p.shape for p in ALL])
    everything = hip.mask_regions_workspace_bytes(int(off[-1]), len(ALL), max_words)
    least = hip.mask_regions_workspace_bytes(4 * max_words, 1, max_words)
    assert least == GO.WS_PER_WORD * max_words < everything
    got = GO.run(hip.mask_regions_sized, ALL, connectivity, M, min_area, dev=DEV, ws_bytes=everything)
    GO.same(got, want)
    rounds = GO.run(hip.mask_regions_sized, ALL, connectivity, M, min_area, dev=DEV, ws_bytes=least)      # one plane per round
    GO.same(rounds, want)
    assert np.array_equal(rounds["out_bits"], got["out_bits"])
    some = GO.run(hip.mask_regions_sized, ALL, connectivity, M, min_area, dev=DEV, ws_bytes=3 * least + 100, dirty=True)
    GO.same(some, want)                                               # three planes per round, every pad bit of the input set


def test_a_refused_plane_on_the_device():
    from camouflaged_vlm_amd import hip
    planes = [ALL[0], np.ones((5, 33), bool), ALL[1]]
    dims, off, max_words = GO.tables([p.shape for p in planes])
    dims = dims.copy()
    dims[1] = (6, 33)
    M = 3
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    run = {}
    for dev in ("cpu", DEV):
        bits = torch.from_numpy(np.concatenate([GO.pack_rows(p) for p in planes])).to(dev)
        n, table, status = (t.to(dev) for t in (i32(3), i32(3, M, 6), i32(1)))
        out = torch.full((M * bits.numel(),), 0xA5, dtype=torch.uint8, device=dev)
        args = (bits, torch.from_numpy(off).to(dev), torch.from_numpy(dims).to(dev), max_words, 8, 0)
        if dev == "cpu":
            hip.mask_regions_sized_host(*args, n, table, out, status)
        else:
            ws = torch.empty(hip.mask_regions_workspace_bytes(bits.numel(), 3, max_words), dtype=torch.uint8, device=dev)
            hip.mask_regions_sized(*args, ws, n, table, out, status)
        run[dev] = [t.cpu() for t in (n, table, out, status)]
    for a, b in zip(run["cpu"], run[DEV]):
        assert torch.equal(a, b)
    assert int(run[DEV][3]) == 1 and int(run[DEV][0][1]) == 0 and not run[DEV][2][M * int(off[1]):M * int(off[2])].any()


# ---- cvlm_region_alpha ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [56, 336])
def test_region_alpha_against_the_oracle(R):
    from camouflaged_vlm_amd import hip, spec
    assert spec.TINY_CLIP.image_resolution == 56
    rng = np.random.default_rng(R)
    planes = [np.ones((1, 1), bool), rng.random((5, 33)) < 0.5, rng.random((20, 30)) < 0.5, rng.random((R, R)) < 0.5, np.ones((R, R), bool),
              rng.random((1024, 1024)) < 0.5]
    alpha = torch.from_numpy(rng.random((3, R, R)).astype(np.float32))
    src = [0, 1, 2, 0, 1, 2]
    out, status = GO.run_alpha(hip.region_alpha, planes, alpha, src, dev=DEV)
    assert status == 0
    err = RO.rowerr(out, GO.region_alpha(planes, alpha, src), row_dims=2)
    print(f"cvlm_region_alpha R = {R}: rowerr {err:.3g}")
    assert err <= 1e-6
    assert RO.same_bits(out[3], alpha[0] * torch.from_numpy(planes[3].astype(np.float32)))       # (R, R): out == alpha * bit exactly
    assert RO.same_bits(out[4], alpha[1])                                                        # a full (R, R) plane: alpha bit for bit
    host, _ = GO.run_alpha(hip.region_alpha_host, planes, alpha, src)
    assert RO.same_bits(out, host)                                                               # the blend is not contracted on either side
    out, status = GO.run_alpha(hip.region_alpha, planes[:2], alpha, [3, 0], dev=DEV)
    assert status == 1 and not out[0].any()                                                      # a src outside [0, N)


# ---- the tiny engine -------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def scene(tiny, gold):
    """The engine, K = 2 hypotheses per image as P = 4 planes of mask logits, their sized planes at two ragged sizes with a hand-made
    two-blob pattern ORed in wherever the synthetic mask has fewer than two regions, the split and the compacted regions."""
    g, c, _, (inp, ci, cm), dev = tiny
    cas = build_tiny(tiny, gold)
    h = cas.infer_classes(inp, ci, cm, topk=2)
    logits = h.masks.reshape(-1, 1, g.inp_size, g.inp_size).clone()
    image_of = [0, 0, 1, 1]
    sizes = [(37, 45), (37, 45), (50, 33), (50, 33)]
    sized = cas.pack_masks_sized(logits, sizes)
    first = cas.mask_regions_sized(sized, regions=4)
    n = first.n_regions.cpu().numpy()
    for p, (hh, ww) in enumerate(sizes):
        if n[p] < 2:                                                  # two blobs well apart, in the plane's own rows
            blobs = np.zeros((hh, ww), bool)
            blobs[1:4, 1:5] = blobs[hh - 5:hh - 1, ww - 7:ww - 2] = True
            lo, hi = sized.byte_range(p)
            sized.bits[lo:hi] |= torch.from_numpy(GO.pack_rows(blobs)).to(dev)
    regs = cas.mask_regions_sized(sized, regions=4)
    regions, plane_of, rank = regs.compact()
    return dict(cas=cas, logits=logits, ci=ci, image_of=image_of, sizes=sizes, sized=sized, regs=regs, regions=regions, plane_of=plane_of, rank=rank)


def test_the_split_of_the_engine_planes_is_the_oracle(scene):
    import components_oracle as CO
    regs, sized = scene["regs"], scene["sized"]
    n, table = regs.n_regions.cpu().numpy(), regs.table.cpu().numpy()
    for p in range(4):
        plane = sized.to_numpy(p)
        lab, rows = CO.regions(plane, 8)
        c, t, planes = GO.split(plane, lab, rows, 4, 0)
        assert n[p] == c and np.array_equal(table[p], t)
        for m in range(4):
            assert np.array_equal(regs.masks.to_numpy(p * 4 + m), planes[m])
    Q, P = len(scene["regions"].sizes), 4
    print(f"regions per plane {n.tolist()}: Q = {Q}, P = {P}")
    assert Q > P and Q == int(np.minimum(n, 4).sum())
    assert torch.equal(regs.masks.area, regs.table[..., 0].reshape(-1)) and regs.masks.level == sized.level


def test_classify_regions_against_single_forwards(scene):
    from camouflaged_vlm_amd import hip, maskpost
    cas, regions, plane_of, ci = scene["cas"], scene["regions"], scene["plane_of"], scene["ci"]
    Q, R, dev = len(regions.sizes), cas.c.image_resolution, ci.device
    out = cas.classify_regions(regions, plane_of, scene["logits"], ci, image_of=scene["image_of"])
    out.check()
    logits, pred = out.logits.clone(), out.pred.clone()
    assert logits.shape == (Q, cas.c.n_cls_test) and torch.equal(pred, logits.argmax(-1))
    # each region singly, its alpha read back from the device's own cvlm_region_alpha
    alpha = cas._alpha(scene["logits"], "alpha2").clone()
    a = torch.empty(Q, 1, R, R, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.region_alpha(regions.bits, regions.offsets, torch.from_numpy(maskpost.sized_tables(regions.sizes)[0]).to(dev), alpha,
                     torch.from_numpy(plane_of.astype(np.int32)).to(dev), a, status)
    assert int(status) == 0
    worst = 0.0
    for q in range(Q):
        i = scene["image_of"][int(plane_of[q])]
        _, _, pr, lg = cas.clip.forward(ci[i:i + 1], a[q:q + 1])
        worst = max(worst, dmax(lg[0], logits[q]))
    print(f"classify_regions against {Q} single forwards: {worst:.2e}")
    assert worst <= BATCH_TOL
    # the regions differ from the whole mask: the gate does something
    assert float((a.reshape(Q, -1).sum(1) < alpha[torch.from_numpy(plane_of).to(dev)].reshape(Q, -1).sum(1)).float().mean()) > 0


def test_a_full_plane_per_image_reproduces_stage2(scene, tiny):
    from camouflaged_vlm_amd import maskpost
    cas, ci = scene["cas"], scene["ci"]
    g, c, _, (inp, _, cm), dev = tiny
    R = c.image_resolution
    masks = cas.infer_test(inp, ci, cm).clone()
    _, _, want_pred, want_logits = (t.clone() for t in cas.stage2(masks, ci))
    sizes = [(R, R)] * 2
    _, off, _ = maskpost.sized_tables(sizes)
    full = maskpost.SizedMasks(bits=torch.full((int(off[-1]),), 0xFF, dtype=torch.uint8, device=dev), offsets=torch.from_numpy(off).to(dev),
                               area=None, box=None, status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=sizes)
    out =cas.classify_regions(full, [0, 1], masks, ci)
    d = dmax(out.logits, want_logits)
    print(f"full planes against stage2: {d:.2e}, bit-equal: {torch.equal(out.logits, want_logits)}")
    assert d <= BATCH_TOL and torch.equal(out.pred, want_pred)


def test_chunks_vocabularies_empty_calls_and_refusals(scene, tiny, gold, monkeypatch):
    from camouflaged_vlm_amd import hip, maskpost
    assert maskpost.REGIONS_MAXM == hip.REGIONS_MAXM == 64
    cas, regions, plane_of, ci, image_of = scene["cas"], scene["regions"], scene["plane_of"], scene["ci"], scene["image_of"]
    _, c, _, _, dev = tiny
    whole = cas.classify_regions(regions, plane_of, scene["logits"], ci, image_of=image_of).logits.clone()
    monkeypatch.setattr(type(cas), "class_chunk", lambda self: 3)
    small = cas.classify_regions(regions, plane_of, scene["logits"], ci, image_of=image_of)
    assert small.status.numel() == -(-len(regions.sizes) // 3)
    d = dmax(small.logits, whole)
    print(f"chunks of 3 against one chunk: {d:.2e}")
    assert d <= BATCH_TOL
    monkeypatch.undo()
    # vocab=: three of the constructor's prompts
    pre, suf = cas.clip.prefix["test"], cas.clip.suffix["test"]
    emb = torch.cat([pre, torch.full((pre.shape[0], c.n_ctx, c.text_width), float("nan"), device=dev), suf], 1)[:3]
    vocab = cas.make_vocabulary(embeddings=emb, eot=gold["eot_test"].tolist()[:3], bank=torch.from_numpy(gold["bank_test"][:3]))
    v = cas.classify_regions(regions, plane_of, scene["logits"], ci, image_of=image_of, vocab=vocab)
    assert v.logits.shape == (len(regions.sizes), 3) and dmax(v.logits, whole[:, :3]) <= BATCH_TOL
    # Q = 0 launches nothing
    calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))
    none = maskpost.SizedMasks(bits=regions.bits[:0], offsets=regions.offsets[:1], area=regions.area[:0], box=regions.box[:0],
                               status=regions.status, sizes=[])
    e = cas.classify_regions(none, [], scene["logits"], ci, image_of=image_of)
    assert e.logits.shape == (0, c.n_cls_test) and e.pred.shape == (0,) and e.pred.dtype == torch.int64 and calls == []
    # malformed arguments: ValueError before anything is queued
    for args, kw in (((regions, plane_of[:-1], scene["logits"], ci), dict(image_of=image_of)),
                     ((regions, plane_of + 4, scene["logits"], ci), dict(image_of=image_of)),
                     ((regions, plane_of, scene["logits"], ci), {}),                                 # P = 4 planes, B = 2 images
                     ((regions, plane_of, scene["logits"], ci), dict(image_of=[0, 0, 1, 2])),
                     ((regions, plane_of.astype(np.float32), scene["logits"], ci), dict(image_of=image_of)),
                     ((regions, plane_of, scene["logits"].cpu(), ci), dict(image_of=image_of)),
                     ((regions, plane_of, scene["logits"][:, :, :-1], ci), dict(image_of=image_of)),
                     ((regions, plane_of, scene["logits"], ci[:, :2]), dict(image_of=image_of)),
                     ((regions.bits, plane_of, scene["logits"], ci), dict(image_of=image_of)),
                     ((regions, plane_of, scene["logits"], ci), dict(image_of=image_of, vocab="ovcamo"))):
        with pytest.raises(ValueError):
            cas.classify_regions(*args, **kw)
    assert calls == []
    for kw in (dict(regions=0), dict(regions=65), dict(min_area=-1), dict(connectivity=6)):
        with pytest.raises(ValueError):
            cas.mask_regions_sized(scene["sized"], **kw)
    with pytest.raises(ValueError):
        cas.mask_regions_sized(scene["sized"].bits)
    assert calls == []


def test_the_chain_to_coco_results(scene):
    from camouflaged_vlm_amd import maskpost
    cas, regions, plane_of = scene["cas"], scene["regions"], scene["plane_of"]
    out = cas.classify_regions(regions, plane_of, scene["logits"], scene["ci"], image_of=scene["image_of"])
    scores = out.logits.softmax(-1).amax(-1)
    image_ids = [scene["image_of"][int(p)] for p in plane_of]
    res = maskpost.instances_to_coco(cas.mask_rle_sized(regions), image_ids, out.pred, scores, boxes=regions.box)
    assert len(res) == len(regions.sizes)
    area = regions.area.cpu().tolist()
    for q, d in enumerate(res):
        assert d["segmentation"]["size"] == list(regions.sizes[q]) and sum(d["segmentation"]["counts"][1::2]) == area[q]
        assert d["image_id"] == image_ids[q] and d["category_id"] == int(out.pred[q]) and 0 < d["score"] <= 1
    m = cas.coco_match(regions, regions, scores=scores, det_image=image_ids, gt_image=image_ids, det_category=out.pred.cpu().tolist(),
                       gt_category=out.pred.cpu().tolist())
    m.check()
