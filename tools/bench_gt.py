"""COCO annotations held against a full class sweep on the device: demo geometry, B = 8, every class of the bank on one
encoded batch -- `decode(enc, classes=all, masks="bits", sizes=...)` (a) as it is and (b) with ground_truth=(gt, gt_image), gt =
`rle_decode` of n annotations per image (discs at the image's own size, as COCO run counts), for n = 1 and n = 10, one process.  The
sizes are tools/bench_sized.py's.  First the intersections are held against numpy on the call's own sized bits and the other fields
against the call without ground_truth=; then, after a warm-up, the two calls and the `rle_decode` of the annotations alternate, each
timed with device events around it and a synchronise after it.  Reported: the added device time (b) - (a) + rle_decode, medians and
ranges, and the peak memory of both.  Then the host alternative for the same pairs: a device-to-host copy of the sized bits,
numpy.unpackbits per plane, `rle.decode` per annotation, `&` and sum per pair on at most 16 threads.  Gated: the parity, and the added
device time below the host alternative.
--kernels: instead, cvlm_mask_rle_decode and cvlm_mask_inter_sized on 64 planes of 1024^2, `--repeat` calls each back to back (for
`rocprofv3 --kernel-trace --stats -- python tools/bench_gt.py --kernels`), with the event-timed means and the bytes moved.
Usage: python tools/bench_gt.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from camouflaged_vlm_amd import hip, host, rle, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision, sized_tables  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]


def host_counts(mask: np.ndarray) -> np.ndarray:
    """bool (h, w) -> the plane's run counts by the definition: transpose, the positions that differ from their predecessor."""
    f = np.ascontiguousarray(mask.T).reshape(-1).view(np.int8)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0)


def disc(h: int, w: int, cy: float, cx: float, r: float) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def annotations(sizes, per_image: int, seed: int = 20):
    """per_image discs per image at the image's own size -> (COCO dicts with plain counts, the image id of each)."""
    rng = np.random.default_rng(seed)
    coco, ids = [], []
    for b, (h, w) in enumerate(sizes):
        for _ in range(per_image):
            m = disc(h, w, h * rng.uniform(0.2, 0.8), w * rng.uniform(0.2, 0.8), min(h, w) * rng.uniform(0.05, 0.4))
            coco.append({"size": [h, w], "counts": host_counts(m).tolist()})
            ids.append(b)
    return coco, ids


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
    S, P = spec.DEMO_SAM.inp_size, 64
    rng = np.random.default_rng(20)
    blob = disc(S, S, S * 0.45, S * 0.55, S * 0.3) ^ (rng.random((S, S)) < 0.002)          # a disc with speckle: a few thousand runs
    c = host_counts(blob).astype(np.int32)
    counts = torch.from_numpy(np.tile(c, P)).to(dev)
    ro = torch.from_numpy(np.arange(P + 1, dtype=np.int64) * c.size).to(dev)
    dims, off, max_words = sized_tables([(S, S)] * P)
    d, o = torch.from_numpy(dims).to(dev), torch.from_numpy(off).to(dev)
    bits = torch.empty(int(off[P]), dtype=torch.uint8, device=dev)
    area, box = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, 4, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(hip.mask_rle_decode_workspace_bytes(P, S * S), dtype=torch.uint8, device=dev)
    ms_dec = timed(lambda: hip.mask_rle_decode(counts, ro, d, o, S * S, bits, area, box, status, ws), args.repeat)
    ok = int(status) == 0 and int(area[0]) == int(blob.sum()) and np.array_equal(
        np.unpackbits(bits[:S * S // 8].cpu().numpy()).reshape(S, S).astype(bool), blob)
    moved = counts.numel() * 4 + 3 * ws.numel() + bits.numel()                              # the stream: zeroed, scanned in place, read
    print(f"cvlm_mask_rle_decode, {P} planes of {S}^2, {c.size} counts each, {args.repeat} calls back to back: {ms_dec * 1e3:.0f} us per call, "
          f"{ms_dec * 1e3 / P:.1f} us per plane, about {moved / 2**20:.0f} MiB moved ({moved / ms_dec / 1e6:.0f} GB/s); plane 0 "
          f"{'equal' if ok else 'DIFFERENT'} to the source", flush=True)
    other = torch.roll(bits.view(P, -1), 1, 0).contiguous().view(-1)
    pairs = torch.stack([torch.arange(P, dtype=torch.int32), torch.arange(P, dtype=torch.int32)], 1).to(dev)
    inter = torch.empty(P, dtype=torch.int32, device=dev)
    ms_int = timed(lambda: hip.mask_inter_sized(bits, o, d, other, o, d, pairs, max_words, inter, status), args.repeat)
    same = int(status) == 0 and inter.cpu().tolist() == [int(blob.sum())] * P
    moved = 2 * bits.numel()
    print(f"cvlm_mask_inter_sized, {P} pairs of planes of {S}^2: {ms_int * 1e3:.0f} us per call, {ms_int * 1e3 / P:.2f} us per pair, "
          f"{moved / 2**20:.0f} MiB read ({moved / ms_int / 1e6:.0f} GB/s); the sums {'equal' if same else 'DIFFERENT'} to the area", flush=True)
    return 0 if ok and same else 1


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
    P = B * K
    sizes = [PHOTO_SIZES[i] for i in np.random.default_rng(19).integers(0, len(PHOTO_SIZES), B)]
    if B >= 2:
        sizes[0], sizes[1] = PHOTO_SIZES[0], PHOTO_SIZES[6]
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    base_kw = dict(masks="bits", sizes=sizes)
    threads = min(16, os.cpu_count() or 1)
    print(f"demo geometry, B = {B}, all {K} classes ({P} prompts), precision {args.precision}, sizes {sizes}; {args.rounds} alternating rounds "
          f"after {args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    ok = True
    for per_image in (1, 10):
        coco, ids = annotations(sizes, per_image)
        gt = cas.rle_decode(coco)
        gt.check()
        # parity before any timing
        plain = cas.decode(enc, classes=classes, **base_kw)
        full = cas.decode(enc, classes=classes, ground_truth=(gt, ids), **base_kw)
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box")) and \
            torch.equal(plain.sized.bits, full.sized.bits) and torch.equal(plain.sized.area, full.sized.area)
        o = full.gt_overlaps
        o.check()
        pairs, inter = o.pairs.cpu().numpy(), o.inter.cpu().numpy()
        truth = [rle.decode(d["counts"], *d["size"]) for d in coco]
        some = list(range(0, len(pairs), max(1, len(pairs) // 16)))
        agree = all(int(inter[i]) == int((full.sized.to_numpy(int(pairs[i, 0])) & truth[int(pairs[i, 1])]).sum()) for i in some)
        agree = agree and len(pairs) == P * per_image and all(np.array_equal(gt.to_numpy(q), truth[q]) for q in range(0, len(truth), max(1, len(truth) // 8)))
        iou = o.iou()
        print(f"{per_image} annotation(s) per image: {len(coco)} planes, {sum(len(d['counts']) for d in coco)} counts, {gt.bits.numel() / 2**20:.1f} MiB of bits; "
              f"{len(pairs)} pairs; the other fields {'equal' if same else 'DIFFERENT'} to the call without ground_truth=; intersections and decoded "
              f"planes {'equal' if agree else 'DIFFERENT'} to numpy on every {max(1, len(pairs) // 16)}th pair; IoU {iou.min():.3f} .. {iou.max():.3f}",
              flush=True)
        del plain, full, o
        modes = [("(a) masks=\"bits\", sizes=", base_kw), ("(b) ... ground_truth=", dict(base_kw, ground_truth=(gt, ids)))]
        for _ in range(args.warmup):
            for _, kw in modes:
                cas.decode(enc, classes=classes, **kw)
            cas.rle_decode(coco)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in modes}
        peaks = {name: 0 for name, _ in modes}
        dec_dev, dec_wall = [], []
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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            again = cas.rle_decode(coco)
            e1.record()
            torch.cuda.synchronize()
            dec_wall.append((time.perf_counter() - t0) * 1e3)
            dec_dev.append(e0.elapsed_time(e1))
            del again
        print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'peak MiB':>9s}")
        for name, _ in modes:
            t = times[name]
            print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {peaks[name] / 2**20:9.1f}", flush=True)
        print(f"{'rle_decode(annotations): events':42s} {statistics.median(dec_dev):10.2f} {min(dec_dev):9.2f} {max(dec_dev):9.2f}; host checks and "
              f"uploads included, wall {statistics.median(dec_wall):.2f} ms", flush=True)
        base, with_gt = (statistics.median(times[name]) for name, _ in modes)
        diffs = [b - a for a, b in zip(times[modes[0][0]], times[modes[1][0]])]
        added = with_gt - base + statistics.median(dec_dev)
        print(f"ground_truth= adds (b) - (a) = {with_gt - base:+.2f} ms (per round {min(diffs):+.2f} .. {max(diffs):+.2f}) + rle_decode "
              f"{statistics.median(dec_dev):.2f} ms = {added:+.2f} ms to the sweep; workspace \"cls_rle\" "
              f"{cas.ws._flat[('u8', 'cls_rle')].numel() / 2**20:.1f} MiB; peak (b) - (a) = {(peaks[modes[1][0]] - peaks[modes[0][0]]) / 2**10:+.1f} KiB", flush=True)
        # the host alternative for the same pairs
        h = cas.decode(enc, classes=classes, **base_kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        raw = h.sized.bits.cpu().numpy()
        t_copy = time.perf_counter() - t0
        _, off, _ = sized_tables(h.sized.sizes)

        def unpack(p):
            hh, ww = h.sized.sizes[p]
            return np.unpackbits(raw[off[p]:off[p + 1]].reshape(hh, -1), axis=1)[:, :ww].astype(bool)

        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            planes = list(pool.map(unpack, range(P)))
            t_unpack = time.perf_counter() - t0
            t0 = time.perf_counter()
            host_truth = list(pool.map(lambda d: rle.decode(d["counts"], *d["size"]), coco))
            t_dec = time.perf_counter() - t0
            t0 = time.perf_counter()
            host_inter = list(pool.map(lambda pq: int((planes[pq[0]] & host_truth[pq[1]]).sum()), pairs.tolist()))
            t_and = time.perf_counter() - t0
        alt = (t_copy + t_unpack + t_dec + t_and) * 1e3
        equal = host_inter == inter.tolist()
        print(f"host alternative for the same {len(pairs)} pairs: copy of {raw.nbytes / 2**20:.1f} MiB {t_copy * 1e3:.0f} ms + unpackbits {t_unpack * 1e3:.0f} ms "
              f"+ rle.decode {t_dec * 1e3:.0f} ms + & and sum {t_and * 1e3:.0f} ms on {threads} threads = {alt:.0f} ms, its sums "
              f"{'equal' if equal else 'DIFFERENT'} to the device's; the device adds {added:+.2f} ms: "
              f"{'below' if added < alt else 'NOT BELOW'} the host alternative", flush=True)
        ok = ok and same and agree and equal and added < alt
        del h, planes, host_truth, gt
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
