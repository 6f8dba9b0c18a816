"""Run-length encoding of packed masks: cvlm_mask_rle_count / cvlm_mask_rle_emit against the oracle (tests/rle_oracle.py:
the definition in numpy) and against cvlm_debug_mask_rle_host, exactly -- every output is an integer -- and into sentinel-filled outputs
with guard bands inside the same tensor: the operator cases, shapes around the kernel's tile, planes in rounds, the reference's own planes
(tests/golden/demo_classes_digest.npz), a base off 16 bytes, gaps, an undersized slot, offsets past 2^31 in bits and in counts; then rle=
of Cascade.infer_classes / decode / the drop-in against the oracle on the call's own bits and against the call without it, and the
utility Cascade.mask_rle."""
import os
import sys

import numpy as np
import pytest
import torch

import rle_oracle as RO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE_ROWS, TILE_WORDS = 128, 16                                                   # the transpose's tile (csrc/rle.hip: RL_TH, RL_TW)
GUARD = 5                                                                         # sentinel elements before, between and behind the slices
FILL = -9


def device_rle(bits, H: int, W: int, ws_planes=None, spare: int = 0, short: int = 0, host: bool = True):
    """hip.mask_rle_count then hip.mask_rle_emit on device bits (P, H * W / 8) into ONE sentinel-filled counts tensor, so a wrong store
    cannot leave the allocation.  GUARD sentinels lie before the first slice; the slice of every plane but the last holds its
    n_runs[p] + spare counts and then GUARD elements more, which the plane has no counts for: the sentinels between the planes; the
    last plane's slice ends with its n_runs + spare - short elements (short > 0: an undersized slot) and GUARD sentinels follow it
    outside every slice, where only the kernel's own check keeps a store away.  Asserts every element outside the planes' counts
    untouched -> (n_runs, each plane's counts as far as its slice goes, status).  With `host` the same through
    cvlm_debug_mask_rle_host must agree element for element."""
    from camouflaged_vlm_amd import hip
    b = (torch.from_numpy(np.ascontiguousarray(bits)) if isinstance(bits, np.ndarray) else bits).to(DEV)
    P = b.shape[0]
    n = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hip.mask_rle_count(b, H, W, n)
    runs = n.cpu().numpy().astype(np.int64)
    room = runs + spare + GUARD
    room[P - 1] = runs[P - 1] + spare - short
    off = np.zeros(P + 1, dtype=np.int64)
    off[1:] = np.cumsum(room)
    off += GUARD
    total = int(off[P]) + GUARD
    ws = torch.empty(hip.mask_rle_workspace_bytes(P if ws_planes is None else ws_planes, H, W), dtype=torch.uint8, device=DEV)

    def run(emit, dev):
        counts = torch.full((total,), FILL, dtype=torch.int32, device=dev)
        status = torch.full((1,), -3, dtype=torch.int32, device=dev)
        emit(torch.from_numpy(off).to(dev), counts, status)
        if dev != "cpu":
            torch.cuda.synchronize()
        return counts.cpu().numpy(), int(status.cpu().item())

    got, status = run(lambda o, c, s: hip.mask_rle_emit(b, H, W, o, c, s, ws), DEV)
    if host:
        cpu, hn = b.cpu(), torch.full((P,), -7, dtype=torch.int32)
        ref, hstatus = run(lambda o, c, s: hip.mask_rle_host(cpu, H, W, hn, o, c, s), "cpu")
        assert np.array_equal(runs, hn.numpy()) and status == hstatus and np.array_equal(got, ref), "the host entry"
    keep = np.ones(total, dtype=bool)
    out = []
    for p in range(P):
        end = off[p] + min(runs[p], room[p])
        keep[off[p]:end] = False
        out.append(got[off[p]:end])
    assert (got[keep] == FILL).all(), "an element outside the planes' counts was overwritten"
    return runs, out, status


def check(planes: np.ndarray, H: int, W: int, **kw):
    bits = RO.pack(planes)
    want = RO.encode(bits, H, W)
    runs, got, status = device_rle(bits, H, W, **kw)
    assert status == 0 and runs.tolist() == [len(w) for w in want]
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and np.array_equal(g, w), p
    return runs


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 64), (8, 64), (31, 64), (32, 64), (33, 64), (65, 96)])
def test_operator_cases_equal_the_oracle(H, W):
    """Every case of the shape as one batch: each plane has neighbours it must not join; with and without spare room."""
    planes = np.stack(list(RO.cases(H, W).values()))
    check(planes, H, W)
    check(planes, H, W, spare=3)


def test_two_planes_do_not_join():
    H, W = 4, 32
    planes = np.zeros((2, H, W), dtype=bool)
    planes[0, H - 1, W - 1] = True
    planes[1, 1, 0] = True
    _, got, _ = device_rle(RO.pack(planes), H, W)
    assert got[0].tolist() == [H * W - 1, 1] and got[1].tolist() == [1, 1, H * W - 2]


@pytest.mark.parametrize("H,wpr", [(TILE_ROWS - 1, TILE_WORDS - 1), (TILE_ROWS + 1, TILE_WORDS + 1), (2 * TILE_ROWS + 1, 2 * TILE_WORDS - 1),
                                   (2 * TILE_ROWS, 2 * TILE_WORDS), (TILE_ROWS - 32, TILE_WORDS)])
def test_shapes_around_the_tile(H, wpr):
    """One below and one above the tile in rows and word columns, several tiles each way; H % 32 == 0 takes the whole-word stores,
    the others the ORs into the zeroed stream."""
    rng = np.random.default_rng(H * 100 + wpr)
    W = 32 * wpr
    planes = np.stack([rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.03, RO.cases(H, W)["stripes"]])
    check(planes, H, W)


def test_planes_in_rounds():
    """130 planes of 33 x 64 through a workspace of exactly seven planes: 19 rounds, the last of four planes."""
    rng = np.random.default_rng(130)
    P, H, W = 130, 33, 64
    planes = rng.random((P, H, W)) < rng.random((P, 1, 1))
    check(planes, H, W, ws_planes=7)


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


def test_reference_planes_equal_the_oracle_and_repeat(ref_bits):
    """The six 1024 x 1024 planes of the reference: twice, and plane by plane, with bit-identical outputs."""
    S = 1024
    want = RO.encode(ref_bits, S, S)
    first = device_rle(ref_bits, S, S)
    again = device_rle(ref_bits, S, S, host=False)
    assert first[2] == 0 and first[0].tolist() == [len(w) for w in want] and (first[0] >= 100000).all()
    for p in range(6):
        assert np.array_equal(first[1][p], want[p]) and np.array_equal(again[1][p], want[p]), p
        alone = device_rle(ref_bits[p:p + 1], S, S, host=False)
        assert alone[0].tolist() == [len(want[p])] and np.array_equal(alone[1][0], want[p]), p


def test_bits_off_a_sixteen_byte_boundary():
    """The same planes from a 16-byte aligned base and 4 bytes further on (the kernels load whole words one by one: both are the
    one path they have)."""
    rng = np.random.default_rng(4)
    P, H, W = 2, 150, 1024
    planes = rng.random((P, H, W)) < 0.2
    bits = RO.pack(planes)
    want = RO.encode(bits, H, W)
    buf = torch.zeros(bits.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    for at in (0, 4):
        b = buf[at:at + bits.size].view(P, -1)
        b.copy_(torch.from_numpy(bits))
        assert b.data_ptr() % 16 == at
        _, got, status = device_rle(b, H, W, host=False)
        assert status == 0 and all(np.array_equal(g, w) for g, w in zip(got, want)), at


def test_undersized_slot_sets_status_and_stays_inside():
    """The last plane's slice one element short, its guard band right behind the slice inside the same tensor: status 1, the band
    untouched (device_rle asserts every sentinel), the slice holds what fits and the other planes are whole."""
    H, W = 33, 64
    planes = np.stack([RO.cases(H, W)[k] for k in ("random_0.5", "random_0.01", "checker")])
    bits = RO.pack(planes)
    want = RO.encode(bits, H, W)
    runs, got, status = device_rle(bits, H, W, short=1)
    assert status == 1 and runs.tolist() == [len(w) for w in want]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2][:-1])
    _, got, status = device_rle(bits, H, W, short=40)          # transitions dropped too, not only the tail run
    assert status == 1 and np.array_equal(got[2], want[2][:-40]) and np.array_equal(got[0], want[0])


def test_slices_outside_counts_are_dropped():
    """offsets that leave counts[0, total) on either side: nothing is stored for those planes, status 1, the others whole."""
    from camouflaged_vlm_amd import hip
    H, W = 8, 64
    planes = np.stack([RO.cases(H, W)[k] for k in ("random_0.5", "checker", "random_0.5")])
    bits = torch.from_numpy(RO.pack(planes)).to(DEV)
    want = RO.encode(bits.cpu().numpy(), H, W)
    n = len(want[0])
    ws = torch.empty(hip.mask_rle_workspace_bytes(3, H, W), dtype=torch.uint8, device=DEV)
    for off, whole in (([-4, n + 8, 2 * n + 600, 3 * n + 700], (1, 2)), ([8, n + 8, 2 * n + 600, 10 ** 12], (0, 1)),
                       ([8, n + 58, n + 28, 2 * n + 38], (0, 2))):     # plane 1's slice runs backwards: empty
        counts = torch.full((3 * n + 700,), FILL, dtype=torch.int32, device=DEV)
        status = torch.full((1,), -3, dtype=torch.int32, device=DEV)
        hip.mask_rle_emit(bits, H, W, torch.tensor(off, device=DEV), counts, status, ws)
        torch.cuda.synchronize()
        c = counts.cpu().numpy()
        keep = np.ones(c.size, dtype=bool)
        for p in whole:
            assert np.array_equal(c[off[p]:off[p] + len(want[p])], want[p]), (off, p)
            keep[off[p]:off[p] + len(want[p])] = False
        assert status.item() == 1 and (c[keep] == FILL).all(), off


def test_bits_past_two_to_the_31():
    """16 400 planes of 1024 x 1024, all zero but the last: the last plane starts 2^31 + 2 MiB into the bits.  The emit walks them in
    rounds of 256 planes."""
    from camouflaged_vlm_amd import hip
    P, S = 16400, 1024
    try:
        bits = torch.zeros(P, S * S // 8, dtype=torch.uint8, device=DEV)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("2.1 GiB of device memory for the 16 400 planes could not be allocated")
    last = RO.pack((np.random.default_rng(31).random((1, S, S)) < 0.001))
    bits[P - 1].copy_(torch.from_numpy(last[0]))
    want = RO.encode(last, S, S)[0]
    n = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hip.mask_rle_count(bits, S, S, n)
    assert int(n[P - 1]) == len(want) > 1000 and bool((n[:P - 1] == 1).all())
    off = torch.zeros(P + 1, dtype=torch.int64, device=DEV)
    off[1:] = torch.cumsum(n, 0)
    counts = torch.full((int(off[P]) + GUARD,), FILL, dtype=torch.int32, device=DEV)
    status = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    ws = torch.empty(hip.mask_rle_workspace_bytes(256, S, S), dtype=torch.uint8, device=DEV)
    hip.mask_rle_emit(bits, S, S, off, counts, status, ws)
    torch.cuda.synchronize()
    assert status.item() == 0 and bool((counts[:P - 1] == S * S).all()) and bool((counts[-GUARD:] == FILL).all())
    assert np.array_equal(counts[P - 1:-GUARD].cpu().numpy(), want)


def test_counts_past_two_to_the_31():
    """A plane whose slice starts beyond element 2^29 of counts -- byte 2^31 --, in an uninitialised tensor of a little over 2 GiB:
    only the slices and their neighbours are looked at."""
    from camouflaged_vlm_amd import hip
    H, W = 33, 64
    planes = np.stack([RO.cases(H, W)[k] for k in ("random_0.5", "checker")])
    bits = torch.from_numpy(RO.pack(planes)).to(DEV)
    want = RO.encode(bits.cpu().numpy(), H, W)
    far = (1 << 29) + 4099
    total = far + len(want[1]) + GUARD
    try:
        counts = torch.empty(total, dtype=torch.int32, device=DEV)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("2 GiB of device memory for the counts could not be allocated")
    off = [GUARD, GUARD + len(want[0]), far, far + len(want[1])]
    for lo, hi in ((0, off[1] + GUARD), (far - GUARD, total)):
        counts[lo:hi] = FILL
    status = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    ws = torch.empty(hip.mask_rle_workspace_bytes(1, H, W), dtype=torch.uint8, device=DEV)
    for p in range(2):                                               # one plane per call: each slice has its own end
        hip.mask_rle_emit(bits[p:p + 1], H, W, torch.tensor(off[2 * p:2 * p + 2], device=DEV), counts, status, ws)
        torch.cuda.synchronize()
        assert status.item() == 0
    assert np.array_equal(counts[off[0]:off[1]].cpu().numpy(), want[0]) and np.array_equal(counts[off[2]:off[3]].cpu().numpy(), want[1])
    for lo, hi in ((0, GUARD), (off[1], off[1] + GUARD), (far - GUARD, far), (off[3], total)):
        assert bool((counts[lo:hi] == FILL).all()), (lo, hi)


# ---- tiny geometry, exact ------------------------------------------------------------------------------------------------------------------
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
    dev = torch.device(DEV)
    return g, c, sd_np, tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


@pytest.fixture(scope="module")
def cas(tiny, gold):
    return build_tiny(tiny, gold)


OTHER = ("classes", "pass1_logits", "masks", "edges", "logits", "pred", "iou", "mask_bits", "area", "box", "inter", "n_comp", "comps", "n_kept",
         "kept_bits", "kept_area", "kept_box", "n_holes", "holes", "n_filled", "filled_bits", "filled_area", "band_bits", "band_area",
         "band_inter", "edge_bits", "edge_area", "edge_band", "edge_inter")
SOURCE = {"mask": "mask_bits", "kept": "kept_bits", "filled": "filled_bits"}
CLASSES = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]                                      # 10 prompts in passes of 4, 4 and 2
POST = dict(masks="bits", min_area=16, fill_holes=16)


def assert_rle_is_oracle(r, planes_bits: torch.Tensor, S: int):
    """A MaskRle = the oracle on the given planes (any leading shape): n_runs, offsets without gaps, counts; to_coco decodes back."""
    from camouflaged_vlm_amd import rle
    flat = planes_bits.cpu().numpy().reshape(-1, planes_bits.shape[-1])
    want = RO.encode(flat, S, S)
    N = len(want)
    assert r.size == (S, S) and r.n_runs.dtype == torch.int32 and r.offsets.dtype == torch.int64 and r.counts.dtype == torch.int32
    assert all(t.is_cuda for t in (r.counts, r.offsets, r.n_runs))
    assert r.n_runs.cpu().tolist() == [len(w) for w in want]
    assert r.offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert tuple(r.counts.shape) == (sum(len(w) for w in want),) and np.array_equal(r.counts.cpu().numpy(), np.concatenate(want))
    planes = RO.unpack(flat, S, S)
    for compressed in (False, True):
        coco = r.to_coco(compressed=compressed)
        assert len(coco) == N
        for p, d in enumerate(coco):
            c = rle.string_to_counts(d["counts"]) if compressed else d["counts"]
            assert d["size"] == [S, S] and isinstance(d["counts"], bytes if compressed else list)
            assert np.array_equal(rle.decode(c, S, S), planes[p]), p
    return want


def check_call(call, S: int, name: str):
    """`call(**kw)` runs one entry point: with rle=name the new field is the oracle's on the call's own planes and every other field
    keeps the bits of the call without it."""
    plain = call()
    assert plain.rle is None
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    h = call(rle=name)
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in plain), f
    for f, t in plain.items():                                                    # bit for bit, floats included
        assert torch.equal(getattr(h, f).contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    want = assert_rle_is_oracle(h.rle, getattr(h, SOURCE[name]), S)
    print(name, "n_runs", [len(w) for w in want])
    assert max(len(w) for w in want) > 2                                          # not only empty and full planes
    return h


@pytest.mark.parametrize("name", ["mask", "kept", "filled"])
def test_infer_classes_rle(tiny, cas, monkeypatch, name):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **POST, **kw), g.inp_size, name)


@pytest.mark.parametrize("name", ["mask", "kept", "filled"])
def test_decode_rle(tiny, cas, monkeypatch, name):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    h = check_call(lambda **kw: cas.decode(enc, topk=5, images=[1, 0, 1], **POST, **kw), g.inp_size, name)
    K = 5
    o = h.rle.offsets.cpu().numpy()
    c = h.rle.counts.cpu().numpy()
    assert np.array_equal(c[o[0]:o[K]], c[o[2 * K]:o[3 * K]])                     # images 1, 0, 1: rows 0 and 2 are the same hypotheses


def test_mask_rle_utility(tiny, cas):
    g, _, _, (inp, ci, cm), _ = tiny
    S = g.inp_size
    bits, _, _ = cas.pack_masks(cas.infer_test(inp, ci, cm).clone())
    assert_rle_is_oracle(cas.mask_rle(bits, S, S), bits, S)
    odd = torch.zeros(bits.numel() + 2, dtype=torch.uint8, device=DEV)[2:].view_as(bits)           # off a 4-byte boundary: cloned
    odd.copy_(bits)
    assert_rle_is_oracle(cas.mask_rle(odd, S, S), bits, S)
    empty = cas.mask_rle(torch.zeros(2, S * S // 8, dtype=torch.uint8, device=DEV), S, S)          # what a hypothesis of class -1 packs to
    assert empty.counts.cpu().tolist() == [S * S, S * S] and empty.n_runs.cpu().tolist() == [1, 1]
    rows = cas.mask_rle(bits.view(-1, 2 * S // 8), 2, S)                                            # any H, not the model's
    assert_rows = RO.encode(bits.cpu().numpy().reshape(-1, 2 * S // 8), 2, S)
    assert np.array_equal(rows.counts.cpu().numpy(), np.concatenate(assert_rows))
    for bad in (dict(bits=bits.cpu()), dict(bits=bits.int()), dict(bits=bits[0]), dict(W=S + 32), dict(W=S // 2 + 1), dict(H=0), dict(H=True)):
        kw = dict(dict(bits=bits, H=S, W=S), **bad)
        with pytest.raises(ValueError):
            cas.mask_rle(kw["bits"], kw["H"], kw["W"])


def test_bad_rle_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_rle_count",
             "mask_rle_emit", "mask_overlap")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(rle="mask"), dict(masks="logits", rle="mask"), dict(masks="bits", rle="bits"), dict(masks="bits", rle=True),
                   dict(masks="bits", rle="kept"), dict(masks="both", rle="filled"), dict(masks="bits", rle="kept", fill_holes=4),
                   dict(masks="bits", rle="filled", min_area=4)):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_rle_memory_is_the_results_and_the_workspace(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, rle="kept" peaks above the same call without it by no more than
    the new result tensors, the status word and cumsum's temporaries -- the workspace "cls_rle" is already there and is no larger
    than RLE_WS_CAP."""
    from camouflaged_vlm_amd import engine, hip
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    modes = {"plain": dict(masks="bits", min_area=16), "rle": dict(masks="bits", min_area=16, rle="kept")}
    for kw in modes.values():
        cas.infer_classes(inp, ci, cm, topk=5, **kw)
    torch.cuda.synchronize()
    ws = cas.ws._flat[("u8", "cls_rle")]
    assert hip.mask_rle_workspace_bytes(10, g.inp_size, g.inp_size) <= ws.numel() <= engine.RLE_WS_CAP      # grow-only: an earlier call may have had more planes
    peak = {}
    for name, kw in modes.items():
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        h = cas.infer_classes(inp, ci, cm, topk=5, **kw)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - start
        if name == "rle":
            new = [h.rle.counts, h.rle.offsets, h.rle.n_runs, h.rle.status]
            results = sum(-(-t.numel() * t.element_size() // 512) * 512 for t in new)                 # the allocator's 512-byte blocks
        del h
    print(f"peak over the starting level: plain {peak['plain']} B, with rle {peak['rle']} B; new results {results} B")
    assert 0 < peak["rle"] - peak["plain"] <= results + 4 * 512


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_rle_through(tiny, gold, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
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
    S = g.inp_size
    with torch.no_grad():
        plain = model.infer_classes(inp, ci, cm, topk=3, **POST)
        got = model.infer_classes(inp, ci, cm, topk=3, rle="filled", **POST)
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, rle="kept", **POST)
        torch.cuda.synchronize()
        assert plain.rle is None
        assert_rle_is_oracle(got.rle, got.filled_bits, S)
        assert_rle_is_oracle(dec.rle, dec.kept_bits, S)
        for f in ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box", "kept_bits", "filled_bits"):
            assert torch.equal(getattr(got, f), getattr(plain, f)), f
        bits, _, _ = model.pack_masks(model.infer_test(inp, ci, cm))
        assert_rle_is_oracle(model.mask_rle(bits, S, S), bits, S)
