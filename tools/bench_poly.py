"""COCO polygon annotations on the device, timed.  Two parts, one process; every line goes to stdout and to --log
(default profiles/poly_bench.log).
Per launch: 64 planes of 1024^2, each the outline of a disc in 200 vertices, (a) one polygon per plane and (b) four overlapping ones,
through cvlm_mask_poly_decode; in the same run cvlm_mask_rle_decode of the same 64 planes from their run counts (the ratio is
reported, not gated) and the HOST ALTERNATIVE: cvlm_debug_mask_poly_decode_host -- the sequential algorithm of pycocotools' C, which is
not installed here, so this is a stand-in for it -- plus the upload of its planes.  The three alternate for --rounds rounds; medians
and ranges.  Gated: the device's planes equal the host entry's, and the device time lies below the host alternative's.
The sweep: demo geometry, B = 8, every class of the bank on one encoded batch -- `decode(enc, classes=all, masks="bits", sizes=...)` as
it is and with ground_truth=(polygons_decode(annotations), ids), n = 1 and n = 10 polygon annotations per image, alternating; the added
device time (b) - (a) + polygons_decode against the host alternative for the same annotations, and the peak memory of both calls.
Usage: python tools/bench_poly.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--skip-sweep] [--log PATH]"""
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
from camouflaged_vlm_amd.engine import Cascade, Precision, polygons_request, sized_tables  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]
LOG = None


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def outline(n: int, cx: float, cy: float, r: float) -> list:
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).reshape(-1).tolist()


def host_counts(mask: np.ndarray) -> np.ndarray:
    f = np.ascontiguousarray(mask.T).reshape(-1).view(np.int8)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0)


def host_decode(anns):
    """The host alternative: every check, cvlm_debug_mask_poly_decode_host, its planes -> (bits, area, box on the host, seconds)."""
    t0 = time.perf_counter()
    xy, po, pp, sizes = polygons_request(anns)
    P = len(sizes)
    dims, off, _ = sized_tables(sizes)
    t = torch.from_numpy
    bits = torch.empty(int(off[P]), dtype=torch.uint8)
    area, box, status = torch.empty(P, dtype=torch.int32), torch.empty(P, 4, dtype=torch.int32), torch.empty(1, dtype=torch.int32)
    hip.mask_poly_decode_host(t(xy), t(po), t(pp), t(dims), t(off), max(h * w for h, w in sizes), bits, area, box, status)
    assert int(status) == 0
    return bits, area, box, time.perf_counter() - t0


def med(v) -> str:
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def per_launch(args, dev) -> bool:
    S, P = 1024, 64
    rng = np.random.default_rng(21)
    ok = True
    for polys in (1, 4):
        anns = []
        for _ in range(P):
            cx, cy, r = S * rng.uniform(0.35, 0.65), S * rng.uniform(0.35, 0.65), S * rng.uniform(0.1, 0.3)
            anns.append({"size": [S, S], "polygons": [outline(200, cx + 40 * k, cy - 30 * k, r) for k in range(polys)]})
        xy, po, pp, sizes = polygons_request(anns)
        dims, off, _ = sized_tables(sizes)
        t = lambda a: torch.from_numpy(a).to(dev)
        d_xy, d_po, d_pp, d_dims, d_off = t(xy), t(po), t(pp), t(dims), t(off)
        bits = torch.empty(int(off[P]), dtype=torch.uint8, device=dev)
        area, box, status = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((P,), (P, 4), (1,)))
        ws = torch.empty(hip.mask_poly_decode_workspace_bytes(P, S * S), dtype=torch.uint8, device=dev)
        poly = lambda: hip.mask_poly_decode(d_xy, d_po, d_pp, d_dims, d_off, S * S, bits, area, box, status, ws)
        poly()
        h_bits, h_area, h_box, _ = host_decode(anns)
        same = int(status) == 0 and torch.equal(bits.cpu(), h_bits) and torch.equal(area.cpu(), h_area) and torch.equal(box.cpu(), h_box)
        # the same planes as run counts, for cvlm_mask_rle_decode in the same run
        planes = np.unpackbits(h_bits.numpy().reshape(P, S, S // 8), axis=2).astype(bool)
        counts = [host_counts(m).astype(np.int32) for m in planes]
        d_counts = t(np.concatenate(counts))
        d_ro = t(np.concatenate([[0], np.cumsum([c.size for c in counts])]).astype(np.int64))
        r_bits = torch.empty_like(bits)
        r_ws = torch.empty(hip.mask_rle_decode_workspace_bytes(P, S * S), dtype=torch.uint8, device=dev)
        runs = lambda: hip.mask_rle_decode(d_counts, d_ro, d_dims, d_off, S * S, r_bits, area, box, status, r_ws)
        runs()
        same = same and torch.equal(r_bits, bits)
        for _ in range(args.warmup):
            poly()
            runs()
        torch.cuda.synchronize()
        t_poly, t_runs, t_host = [], [], []
        for _ in range(args.rounds):
            t_poly.append(event_ms(poly))
            t_runs.append(event_ms(runs))
            hb, _, _, sec = host_decode(anns)
            t0 = time.perf_counter()
            hb.to(dev)
            torch.cuda.synchronize()
            t_host.append((sec + time.perf_counter() - t0) * 1e3)
        points = int(sum((np.abs(np.roll(v, -1, 0) - v).max(1) + 1).sum() for v in
                         ((5.0 * xy[po[q]:po[q + 1]] + 0.5).astype(np.int64).reshape(-1, 2) for q in range(len(po) - 1))))
        m_poly, m_runs, m_host = (statistics.median(v) for v in (t_poly, t_runs, t_host))
        say(f"{P} planes of {S}^2, {polys} polygon(s) of 200 vertices per plane, {points} walk points in all; planes "
            f"{'equal' if same else 'DIFFERENT'} to the host entry's and to cvlm_mask_rle_decode's; {args.rounds} alternating rounds, ms per call, median (range):")
        say(f"  cvlm_mask_poly_decode            {med(t_poly)}  = {m_poly * 1e3 / P:.1f} us per plane")
        say(f"  cvlm_mask_rle_decode, same planes {med(t_runs)}  = {m_runs * 1e3 / P:.1f} us per plane; polygons / run counts = {m_poly / m_runs:.2f}")
        say(f"  host alternative (stand-in for pycocotools' C: cvlm_debug_mask_poly_decode_host + upload of {h_bits.numel() / 2**20:.0f} MiB) {med(t_host)}: "
            f"the device is {'below' if m_poly < m_host else 'NOT BELOW'} it, {m_host / m_poly:.0f} x")
        ok = ok and same and m_poly < m_host
    return ok


def annotations(sizes, per_image: int, seed: int = 21):
    rng = np.random.default_rng(seed)
    anns, ids = [], []
    for b, (h, w) in enumerate(sizes):
        for _ in range(per_image):
            cx, cy, r = w * rng.uniform(0.2, 0.8), h * rng.uniform(0.2, 0.8), min(h, w) * rng.uniform(0.05, 0.4)
            anns.append({"size": [h, w], "polygons": [outline(int(rng.integers(20, 200)), cx, cy, r)]})
            ids.append(b)
    return anns, ids


def sweep(args, dev) -> bool:
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    B, K = args.batch, c.n_cls_test
    sizes = [PHOTO_SIZES[i] for i in np.random.default_rng(19).integers(0, len(PHOTO_SIZES), B)]
    if B >= 2:
        sizes[0], sizes[1] = PHOTO_SIZES[0], PHOTO_SIZES[6]
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    base_kw = dict(masks="bits", sizes=sizes)
    say(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, sizes {sizes}; {args.rounds} alternating rounds "
        f"after {args.warmup} warm-up")
    ok = True
    for per_image in (1, 10):
        anns, ids = annotations(sizes, per_image)
        gt = cas.polygons_decode(anns)
        gt.check()
        h_bits, h_area, _, _ = host_decode(anns)
        same = torch.equal(gt.bits.cpu(), h_bits) and torch.equal(gt.area.cpu(), h_area)
        plain = cas.decode(enc, classes=classes, **base_kw)
        full = cas.decode(enc, classes=classes, ground_truth=(gt, ids), **base_kw)
        torch.cuda.synchronize()
        full.gt_overlaps.check()
        same = same and torch.equal(plain.sized.bits, full.sized.bits) and torch.equal(plain.pred, full.pred)
        pairs, inter = full.gt_overlaps.pairs.cpu().numpy(), full.gt_overlaps.inter.cpu().numpy()
        some = range(0, len(pairs), max(1, len(pairs) // 16))
        agree = all(int(inter[i]) == int((full.sized.to_numpy(int(pairs[i, 0])) & gt.to_numpy(int(pairs[i, 1]))).sum()) for i in some)
        del plain, full
        modes = [("(a) masks=\"bits\", sizes=", base_kw), ("(b) ... ground_truth=", dict(base_kw, ground_truth=(gt, ids)))]
        for _ in range(args.warmup):
            for _, kw in modes:
                cas.decode(enc, classes=classes, **kw)
            cas.polygons_decode(anns)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in modes}
        peaks = {name: 0 for name, _ in modes}
        dec_dev, dec_wall, t_host = [], [], []
        for _ in range(args.rounds):
            for name, kw in modes:
                torch.cuda.reset_peak_memory_stats()
                start = torch.cuda.memory_allocated()
                times[name].append(event_ms(lambda: cas.decode(enc, classes=classes, **kw)))
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - start)
            t0 = time.perf_counter()
            dec_dev.append(event_ms(lambda: cas.polygons_decode(anns)))
            dec_wall.append((time.perf_counter() - t0) * 1e3)
            hb, _, _, sec = host_decode(anns)
            t0 = time.perf_counter()
            hb.to(dev)
            torch.cuda.synchronize()
            t_host.append((sec + time.perf_counter() - t0) * 1e3)
        base, with_gt = (statistics.median(times[name]) for name, _ in modes)
        added = with_gt - base + statistics.median(dec_dev)
        alt = statistics.median(t_host)
        say(f"{per_image} polygon annotation(s) per image: {len(anns)} planes, {gt.bits.numel() / 2**20:.1f} MiB of bits, {len(pairs)} pairs; planes "
            f"{'equal' if same else 'DIFFERENT'} to the host entry's and the other fields to the call without ground_truth=; intersections "
            f"{'equal' if agree else 'DIFFERENT'} to numpy on every {max(1, len(pairs) // 16)}th pair")
        for name, _ in modes:
            say(f"  {name:40s} {med(times[name])} ms / call, peak {peaks[name] / 2**20:.1f} MiB")
        say(f"  polygons_decode(annotations): events     {med(dec_dev)} ms; host checks and uploads included, wall {statistics.median(dec_wall):.2f} ms")
        say(f"  ground_truth= of polygons adds (b) - (a) = {with_gt - base:+.2f} ms + polygons_decode {statistics.median(dec_dev):.2f} ms = {added:+.2f} ms; "
            f"peak (b) - (a) = {(peaks[modes[1][0]] - peaks[modes[0][0]]) / 2**10:+.1f} KiB; workspace \"cls_rle\" "
            f"{cas.ws._flat[('u8', 'cls_rle')].numel() / 2**20:.1f} MiB")
        say(f"  host alternative (stand-in for pycocotools' C: the checks, cvlm_debug_mask_poly_decode_host, upload) {med(t_host)} ms: polygons_decode "
            f"is {'below' if statistics.median(dec_dev) < alt else 'NOT BELOW'} it")
        ok = ok and same and agree and statistics.median(dec_dev) < alt
        del gt
    return ok


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "poly_bench.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    LOG = open(args.log, "w")
    say("# tools/bench_poly.py (" + torch.cuda.get_device_name(0) + ")")
    dev = torch.device("cuda:0")
    ok = per_launch(args, dev)
    if not args.skip_sweep:
        ok = sweep(args, dev) and ok
    say("all gates hold" if ok else "A GATE FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
