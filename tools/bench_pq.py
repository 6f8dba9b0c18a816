"""Panoptic quality of a full class sweep on the device: demo geometry, B = 8, every class of the bank on one encoded
batch -- `decode(enc, classes=all, masks="bits", sizes=..., label_maps=True)`, whose panoptic map `LabelMaps.pq_inputs` hands to
`Cascade.panoptic_quality`.  The sizes are tools/bench_sized.py's.  Ground truth is synthesised from the call's own panoptic map: every
image's map shifted by a few pixels, its slots relabelled by a permutation and cut along a 5 x 4 grid of tiles (about 20 segments per
image), written as raw ids and brought back by `Cascade.panoptic_remap`; one slot per image gets another category, one becomes crowd.  First the totals and the per-image results are
held against the oracle (tests/pq_oracle.py) on the same maps, bit by bit; then each entry is timed with device events, `--repeat` calls
back to back, and `pq_inputs` + `panoptic_quality` end to end (device events and wall clock).  Then the host alternative: both maps
copied to the host, per image the published np.unique over gt * 2^24 + pred and the matching loop, images spread over at most 16
threads.  Gated: the parity, and the added device time below the host alternative.
--kernels: instead, cvlm_pan_pair_hist alone on synthetic piecewise-constant maps of the same 8 sizes, at slot tables on both sides of
the LDS bound (for `rocprofv3 --kernel-trace --stats -- python tools/bench_pq.py --kernels`), with the event-timed means.
Usage: python tools/bench_pq.py [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
import argparse
import concurrent.futures
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from camouflaged_vlm_amd import hip, host, segeval, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision, label_tables  # noqa: E402
import pq_oracle as PO  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]


def sweep_sizes(B: int) -> list:
    sizes = [PHOTO_SIZES[i] for i in np.random.default_rng(19).integers(0, len(PHOTO_SIZES), B)]
    if B >= 2:
        sizes[0], sizes[1] = PHOTO_SIZES[0], PHOTO_SIZES[6]
    return sizes


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


def images_of(flat: np.ndarray, sizes) -> list:
    out, at = [], 0
    for h, w in sizes:
        out.append(flat[at:at + h * w].reshape(h, w))
        at += h * w
    return out


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    B = args.batch
    sizes = sweep_sizes(B)
    dims, off, max_pixels = label_tables(sizes)
    n_pix = int(off[-1])
    d, o = torch.from_numpy(dims).to(dev), torch.from_numpy(off).to(dev)
    pred_img = [PO.piecewise(h, w, 62, 5 + b, (max(2, h // 6), max(2, w // 6))) for b, (h, w) in enumerate(sizes)]
    gt_img = [(np.roll(p, (5, 7), (0, 1)) * 7 + 3) % 21 for p in pred_img]
    pred, gt = torch.from_numpy(PO.flat(pred_img)).to(dev), torch.from_numpy(PO.flat(gt_img)).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L = hip.pan_lds_cells()
    print(f"{B} images of {n_pix} pixels in all, about 60 x 20 segments per image, {args.repeat} calls back to back, zero_first each; LDS up to {L} cells", flush=True)
    want = np.stack([PO.pair_counts(g, p, 21, 62)[0] for g, p in zip(gt_img, pred_img)])
    ok = True
    above = L + 1
    while PO.factor(above)[0] < 21:                                   # the first table above the bound that holds the maps' 21 x 62 slots
        above += 1
    for G, S in sorted({(21, 62), (64, 64), (64, 128), (128, 128), (113, 145), (128, 256), (99, 331), PO.factor(L), PO.factor(above), (256, 256)},
                       key=lambda gs: gs[0] * gs[1]):
        inter = torch.empty(B, G, S, dtype=torch.int32, device=dev)
        ms = timed(lambda: hip.pan_pair_hist(pred, gt, B, G, S, d, o, max_pixels, True, inter, status), args.repeat)
        ok = ok and np.array_equal(inter[:, :21, :62].cpu().numpy(), want) and int(inter.sum()) == n_pix
        print(f"cvlm_pan_pair_hist G x S = {G} x {S} = {G * S} cells ({'LDS' if G * S <= L else 'global atomics'}, {4 * B * G * S / 2**10:.0f} KiB of "
              f"table): {ms * 1e3:.0f} us ({n_pix * 8 / ms / 1e6:.0f} GB/s of maps)", flush=True)
    print(f"status {int(status)}; the tables {'agree' if ok else 'DISAGREE'} with the oracle", flush=True)
    return 0 if ok and int(status) == 0 else 1


def main() -> int:
    ap = argparse.ArgumentParser()
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cas.decode(enc, classes=classes, masks="bits", sizes=sizes, label_maps=True, label_weights=weights)
    e0.record()
    h = cas.decode(enc, classes=classes, masks="bits", sizes=sizes, label_maps=True, label_weights=weights)
    e1.record()
    torch.cuda.synchronize()
    ms_sweep = e0.elapsed_time(e1)
    m = h.label_maps
    m.check()
    pred, pred_cat = m.pq_inputs(classes)
    S = K + 1
    # ground truth from the call's own map: shifted and relabelled, then every slot cut along a 5 x 4 grid of tiles (the synthetic
    # weights leave an image one or two segments; the grid brings the ground truth to about 20), as raw ids listed in id order
    pred_img = images_of(pred.cpu().numpy(), sizes)
    slot_img, slot_cat, slot_crowd = PO.shifted_gt(pred_img, pred_cat.cpu().numpy(), K, 24, shift=(4, 6))
    raw_img, segments = [], []
    for b, (hh, ww) in enumerate(sizes):
        tile = (np.arange(hh)[:, None] * 5 // hh) * 4 + np.arange(ww)[None, :] * 4 // ww
        ids = np.where(slot_img[b] > 0, 1000 + 7 * (slot_img[b].astype(np.int64) * 20 + tile), 0).astype(np.int32)
        raw_img.append(ids)
        segments.append([(int(i), int(slot_cat[b, (i - 1000) // 7 // 20]), int(slot_crowd[b, (i - 1000) // 7 // 20] and (i - 1000) // 7 % 20 == 0))
                         for i in np.unique(ids[ids > 0])])
    gt_img = [np.searchsorted(np.asarray([0] + [s[0] for s in segs]), ids).astype(np.int32) for ids, segs in zip(raw_img, segments)]
    raw = torch.from_numpy(PO.flat(raw_img)).to(dev)
    gt = cas.panoptic_remap(raw, sizes, segments)
    gt.check()
    gt_cat, gt_crowd, G = gt.gt_cat, gt.gt_crowd, gt.gt_cat.shape[1]
    n_pix = pred.numel()
    print(f"demo geometry, B = {B}, all {K} classes, precision {args.precision}, sizes {sizes}: {n_pix} pixels; the sweep with label_maps=True "
          f"takes {ms_sweep:.0f} ms; segments per image {m.n_segments.tolist()}, ground-truth segments per image "
          f"{[len(s) for s in segments]}; G x S = {G} x {S}, inter {4 * B * G * S / 2**10:.0f} KiB", flush=True)
    # parity before any timing
    t = cas.panoptic_quality(pred, pred_cat, gt.gt, gt.gt_cat, gt.gt_crowd, sizes, num_classes=K)
    got = t.to_host()
    want = PO.pq_compute(pred_img, pred_cat.cpu().numpy(), gt_img, gt_cat, gt_crowd, K)
    agree = int(gt.unknown.sum()) == 0 and np.array_equal(gt.gt.cpu().numpy(), PO.flat(gt_img))
    try:
        PO.compare(got, want)
    except AssertionError as e:
        agree = False
        print(f"DIFFERENT from the oracle: {e}", flush=True)
    avg = segeval.pq_average(t.counts, t.iou_sum)["All"]
    print(f"totals {'equal' if agree else 'DIFFERENT'} to the oracle on the same maps, f64 sums bit by bit: tp {int(got['counts'][0].sum())}, fp "
          f"{int(got['counts'][1].sum())}, fn {int(got['counts'][2].sum())}, PQ {avg['pq']:.4f} SQ {avg['sq']:.4f} RQ {avg['rq']:.4f} over {avg['n']} classes",
          flush=True)
    # the entries one by one
    dims, off, max_pixels = label_tables(sizes)
    d, o = torch.from_numpy(dims).to(dev), torch.from_numpy(off).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    from camouflaged_vlm_amd.engine import pq_segments_request
    keys, vals, tab, _, _ = pq_segments_request(segments, B)
    keys, vals, tab, gc, gw = up(keys), up(vals), up(tab), up(gt.gt_cat), up(gt.gt_crowd)
    out, unknown, status = torch.empty_like(gt.gt), torch.empty_like(gt.unknown), torch.zeros(1, dtype=torch.int32, device=dev)
    rgb = torch.stack([raw % 256, raw // 256 % 256, raw // 65536], dim=1).to(torch.uint8).contiguous()
    r = args.repeat
    ms = {"pq_inputs (cvlm_label_lookup)": timed(lambda: m.pq_inputs(classes), r),
          "cvlm_pan_remap int32": timed(lambda: hip.pan_remap(raw, B, d, o, max_pixels, keys, vals, tab, out, unknown, status), r),
          "cvlm_pan_remap RGB": timed(lambda: hip.pan_remap(rgb, B, d, o, max_pixels, keys, vals, tab, out, unknown, status), r),
          "cvlm_pan_pair_hist": timed(lambda: hip.pan_pair_hist(pred, gt.gt, B, G, S, d, o, max_pixels, True, t.inter, status), r),
          "cvlm_pan_match": timed(lambda: hip.pan_match(t.inter, pred_cat, gc, gw, K, t.pred_match, t.pred_iou, t.gt_match, t.pred_area, t.gt_area), r),
          "cvlm_pan_accumulate": timed(lambda: hip.pan_accumulate(pred_cat, gc, t.pred_match, t.pred_iou, t.gt_match, K, True, t.counts, t.iou_sum), r)}
    quality = lambda: cas.panoptic_quality(*m.pq_inputs(classes), gt.gt, gt.gt_cat, gt.gt_crowd, sizes, num_classes=K)
    ms["pq_inputs + panoptic_quality, end to end"] = timed(quality, r)
    t0 = time.perf_counter()
    for _ in range(r):
        quality()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / r
    for name, v in ms.items():
        print(f"{name:44s} {v * 1e3:9.0f} us", flush=True)
    added = ms["pq_inputs + panoptic_quality, end to end"]
    print(f"end to end by the wall clock {wall:.2f} ms per call; the device adds {added:.2f} ms to the sweep's {ms_sweep:.0f} ms", flush=True)
    # the host alternative
    threads = min(16, os.cpu_count() or 1, B)
    t0 = time.perf_counter()
    hp, hg = pred.cpu().numpy(), gt.gt.cpu().numpy()
    t_copy = time.perf_counter() - t0
    pcat = pred_cat.cpu().numpy()
    t0 = time.perf_counter()
    hp_img, hg_img = images_of(hp, sizes), images_of(hg, sizes)
    one = lambda b: PO.match(PO.pair_counts_unique(hg_img[b], hp_img[b], G, S), pcat[b], gt.gt_cat[b], gt.gt_crowd[b], K)
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        matches = list(pool.map(one, range(B)))
    totals = PO.accumulate(PO.new_totals(K), matches, pcat, gt.gt_cat, K)
    t_host = time.perf_counter() - t0
    alt = (t_copy + t_host) * 1e3
    same = np.array_equal(totals["counts"], got["counts"]) and PO.same_bits(totals["iou_sum"], got["iou_sum"])
    print(f"host alternative: copy of both maps {t_copy * 1e3:.0f} ms + np.unique over gt * 2^24 + pred, matching and sums {t_host * 1e3:.0f} ms on "
          f"{threads} threads = {alt:.0f} ms, totals {'equal' if same else 'DIFFERENT'}; the device adds {added:.2f} ms: "
          f"{'below' if added < alt else 'NOT BELOW'} the host alternative ({alt / added:.0f} x)", flush=True)
    return 0 if agree and same and added < alt else 1


if __name__ == "__main__":
    sys.exit(main())
