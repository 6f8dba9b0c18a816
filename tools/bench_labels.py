"""Label maps of a full class sweep on the device: demo geometry, B = 8, every class of the bank on one encoded batch --
`decode(enc, classes=all, masks="bits", sizes=...)` (a) as it is and (b) with label_maps=True and label_weights = the softmax of pass 1
at each class, one process.  The sizes are tools/bench_sized.py's.  First the maps are held against numpy on the call's own sized bits
(the published loop on the device's winner map) and the other fields against the call without label_maps; then, after a warm-up, the
two calls alternate, each timed with device events around it and a synchronise after it.  Reported: the added device time (b) - (a),
medians and ranges, and the peak memory of both.  Then the host alternative: the same sweep with masks="both", a device-to-host copy
of the (B, K, S, S) logits, and per image sigmoid, bilinear resize, weighted argmax and the published per-query loop in torch / numpy
on at most 16 threads -- its time and the memory the logits take.  Gated: the parity, and the added device time below the host
alternative.
--kernels: instead, cvlm_label_init / accumulate / finish / lookup on 61 planes of 1024^2 per image for the same 8 sizes and
cvlm_label_iou_hist on the resulting map, `--repeat` calls each back to back (for `rocprofv3 --kernel-trace --stats -- python
tools/bench_labels.py --kernels`), with the event-timed means.
Usage: python tools/bench_labels.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision, label_tables  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]


def sweep_sizes(B: int) -> list:
    sizes = [PHOTO_SIZES[i] for i in np.random.default_rng(19).integers(0, len(PHOTO_SIZES), B)]
    if B >= 2:
        sizes[0], sizes[1] = PHOTO_SIZES[0], PHOTO_SIZES[6]
    return sizes


def published_loop(winner: np.ndarray, bits: np.ndarray, overlap_threshold: float):
    """Mask2Former's per-query loop on an argmax map (h, w) and binary masks (K, h, w) -> (segment map, segment ids)."""
    K = bits.shape[0]
    segment = np.full(winner.shape, -1, np.int16)
    ids = np.zeros(K, np.int32)
    current = 0
    for k in range(K):
        mine = winner == k
        mask_area, original_area = int(mine.sum()), int(bits[k].sum())
        mask = mine & bits[k]
        if mask_area > 0 and original_area > 0 and mask.sum() > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            current += 1
            ids[k] = current
            segment[mask] = k
    return segment, ids


def timed(fn, repeat: int) -> float:
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeat):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeat


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, K, B = spec.DEMO_SAM.inp_size, 61, args.batch
    sizes = sweep_sizes(B)
    dims, off, max_pixels = label_tables(sizes)
    n_pix = int(off[-1])
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    planes = torch.stack([6 * torch.sin(yy / (40.0 + 3 * k) + k) * torch.cos(xx / (55.0 + 2 * k) - k) for k in range(K)]).float().contiguous()
    d, o = torch.from_numpy(dims).to(dev), torch.from_numpy(off).to(dev)
    score = torch.empty(n_pix, device=dev)
    winner, segment = (torch.empty(n_pix, dtype=torch.int16, device=dev) for _ in range(2))
    areas = torch.empty(3, B * K, dtype=torch.int32, device=dev)
    ids, nseg = torch.empty(B * K, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wts = (0.2 + 0.8 * torch.rand(B * K, device=dev)).contiguous()
    ms_init = timed(lambda: hip.label_init(score, winner, segment, areas, ids, nseg, status, B, K), args.repeat)

    def accumulate():                                                # one call per image: the same 61 planes stand for each image's chunk
        for b in range(B):
            hip.label_accumulate(planes, b * K, B, K, d, o, wts, 128, score, winner, segment, max_pixels, areas, status)
    ms_acc = timed(accumulate, args.repeat)
    hip.label_init(score, winner, segment, areas, ids, nseg, status, B, K)
    accumulate()
    ms_fin = timed(lambda: hip.label_finish(B, K, d, o, 0.8, winner, segment, max_pixels, areas, ids, nseg, status), args.repeat)
    table = torch.arange(B * K, dtype=torch.int32, device=dev) % K
    sem = torch.empty(n_pix, dtype=torch.int32, device=dev)
    ms_look = timed(lambda: hip.label_lookup(winner, B, K, d, o, max_pixels, table, 255, sem, status), args.repeat)
    gt8 = (sem % 61).to(torch.uint8)
    totals = torch.zeros(3, K, dtype=torch.int64, device=dev)
    ms_lds = timed(lambda: hip.label_iou_hist(sem, gt8, K, 255, False, True, totals), args.repeat)
    wide = torch.zeros(3, 5000, dtype=torch.int64, device=dev)
    ms_glob = timed(lambda: hip.label_iou_hist(sem, gt8, 5000, 255, False, True, wide), args.repeat)
    ok = int(status) == 0 and int(totals[0].sum()) == n_pix and torch.equal(wide[:, :K], totals)
    print(f"{B} images of {n_pix} pixels in all, {K} planes of {S}^2 each, {args.repeat} calls back to back:\n"
          f"cvlm_label_init {ms_init * 1e3:.0f} us; cvlm_label_accumulate x {B} {ms_acc * 1e3:.0f} us ({ms_acc * 1e9 / (n_pix * K):.1f} ps per pixel "
          f"and plane); cvlm_label_finish {ms_fin * 1e3:.0f} us; cvlm_label_lookup {ms_look * 1e3:.0f} us;\ncvlm_label_iou_hist C = {K} (LDS) "
          f"{ms_lds * 1e3:.0f} us, C = 5000 (global atomics) {ms_glob * 1e3:.0f} us ({n_pix * 5 / ms_lds / 1e6:.0f} / {n_pix * 5 / ms_glob / 1e6:.0f} GB/s); "
          f"the totals {'agree' if ok else 'DISAGREE'}", flush=True)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    B, K = args.batch, c.n_cls_test
    sizes = sweep_sizes(B)
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    weights = torch.softmax(enc.pass1_logits.float(), dim=1).gather(1, classes.to(dev)).contiguous()
    base_kw = dict(masks="bits", sizes=sizes)
    maps_kw = dict(base_kw, label_maps=True, label_weights=weights)
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    print(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, sizes {sizes}; {args.rounds} alternating rounds "
          f"after {args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    # parity before any timing
    plain = cas.decode(enc, classes=classes, **base_kw)
    full = cas.decode(enc, classes=classes, **maps_kw)
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box")) and \
        torch.equal(plain.sized.bits, full.sized.bits) and torch.equal(plain.sized.area, full.sized.area)
    m = full.label_maps
    m.check()
    got = m.to_host()
    agree = np.array_equal(got["orig_area"].reshape(-1), full.sized.area.cpu().numpy())
    for b in range(B):
        bits = np.stack([full.sized.to_numpy(b * K + k) for k in range(K)])
        seg, ids = published_loop(got["winner"][b], bits, 0.8)
        agree = agree and np.array_equal(seg, got["segment"][b]) and np.array_equal(ids, got["segment_id"][b])
    state = sum(t.numel() * t.element_size() for t in (m.score, m.winner, m.segment))
    print(f"label maps of {m.winner.numel()} pixels: {state / 2**20:.1f} MiB of maps ({state / m.winner.numel():.0f} bytes per pixel), segments per image "
          f"{got['n_segments'].tolist()}, winners per image {[len(np.unique(w)) for w in got['winner']]}; the other fields "
          f"{'equal' if same else 'DIFFERENT'} to the call without label_maps; areas, ids and segment maps {'equal' if agree else 'DIFFERENT'} to the "
          f"published loop on the call's own winner map and sized bits", flush=True)
    device_winner = got["winner"]
    del plain, full, m
    modes = [("(a) masks=\"bits\", sizes=", base_kw), ("(b) ... label_maps=True", maps_kw)]
    for _ in range(args.warmup):
        for _, kw in modes:
            cas.decode(enc, classes=classes, **kw)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    peaks = {name: 0 for name, _ in modes}
    for _ in range(args.rounds):
        for name, kw in modes:
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h = cas.decode(enc, classes=classes, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - start)
            del h
    print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'peak MiB':>9s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {peaks[name] / 2**20:9.1f}", flush=True)
    base, with_maps = (statistics.median(times[name]) for name, _ in modes)
    diffs = [b - a for a, b in zip(times[modes[0][0]], times[modes[1][0]])]
    added = with_maps - base
    print(f"label_maps=True adds (b) - (a) = {added:+.2f} ms to the sweep (per round {min(diffs):+.2f} .. {max(diffs):+.2f}); peak (b) - (a) = "
          f"{(peaks[modes[1][0]] - peaks[modes[0][0]]) / 2**20:+.1f} MiB", flush=True)
    # the host alternative: masks="both", then everything on the host
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h = cas.decode(enc, classes=classes, masks="both", sizes=sizes)
    e1.record()
    torch.cuda.synchronize()
    ms_both = e0.elapsed_time(e1)
    peak_both = torch.cuda.max_memory_allocated() - start
    w_host = weights.cpu()
    t0 = time.perf_counter()
    logits = h.masks.cpu()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    differing = 0
    for b, (hh, ww) in enumerate(sizes):
        v = torch.nn.functional.interpolate(torch.sigmoid(logits[b])[None], size=(hh, ww), mode="bilinear", align_corners=False)[0]
        win = (w_host[b][:, None, None] * v).argmax(0).numpy().astype(np.int16)
        published_loop(win, (v >= 0.5).numpy(), 0.8)
        differing += int((win != device_winner[b]).sum())
    t_host = time.perf_counter() - t0
    alt = (t_copy + t_host) * 1e3
    n_pix = sum(a * b for a, b in sizes)
    print(f"host alternative: masks=\"both\" {ms_both:.0f} ms on the device ({ms_both - base:+.0f} ms against (a)), peak {peak_both / 2**20:.0f} MiB "
          f"({h.masks.numel() * 4 / 2**20:.0f} MiB of logits, as many of edge maps); copy {t_copy * 1e3:.0f} ms + sigmoid, resize, argmax and the published "
          f"loop {t_host * 1e3:.0f} ms on {threads} threads = {alt:.0f} ms; its winner (torch's resize, level 127.5) differs from the device's at "
          f"{differing} of {n_pix} pixels; the device adds {added:+.2f} ms: {'below' if added < alt else 'NOT BELOW'} the host alternative", flush=True)
    return 0 if same and agree and added < alt else 1


if __name__ == "__main__":
    sys.exit(main())
