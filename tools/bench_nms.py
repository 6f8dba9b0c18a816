"""Mask NMS on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/nms_bench.log).  Workloads, instances, tables and outputs resident on the device:
  sweep 8 x 40     the sweep's instances at K = 5 hypotheses and M = 8 slots per plane: 8 images (480 x 640 and 427 x 640 in turn) of 40
                   instances each -- three objects that every hypothesis finds, a few pixels apart, and five small regions of its own;
  64 x 40 x 1024^2 64 images of 1024 x 1024 with 40 instances each of the same kind.
Per workload, after --warmup untimed calls, --rounds calls: medians with min and max of
  (a) cvlm_mask_nms_inter, by device events;
  (b) cvlm_mask_inter_sized on the same triangles through its pair table (pairs=), by device events;
  (c) cvlm_mask_inter_sized on every pair of an image, both directions and the diagonal (a_image = b_image), by device events;
  (d) Cascade.mask_nms_sized, request and upload included, wall clock to the synchronisation;
  (e) the host alternative: (b) through Cascade.mask_inter_sized, the intersections and areas read back, then the greedy loop in numpy
      per image on 16 processes that were started before this process opened the device, wall clock.
Gated: the intersections of (a), (b) and the triangle of (c) are equal, and keep of (d) equals (e)'s.
`--inter-only` times (a) alone and names the library: for a probe library of the same ABI in CVLM_PROBE_LIB, e.g. csrc/nms.hip built with
-DCVLM_NMS_PAIR_THREADS=256 (a workgroup per pair instead of a wave per pair).
Usage: python tools/bench_nms.py [--rounds N] [--warmup W] [--inter-only] [--log PATH]"""
import argparse
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_boundary import Engine, event_ms, med  # noqa: E402
from camouflaged_vlm_amd import hip, maskpost  # noqa: E402
from camouflaged_vlm_amd.engine import SizedMasks, sized_tables  # noqa: E402

LOG = None
K, M = 5, 8


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def disc(h: int, w: int, cy: int, cx: int, r: int):
    """(packed rows, area, box) of a disc clipped to the plane, drawn inside its own window only."""
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r, h - 1), max(cx - r, 0), min(cx + r, w - 1)
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    win = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    full = np.zeros((h, 32 * ((w + 31) // 32)), dtype=np.uint8)
    full[y0:y1 + 1, x0:x1 + 1] = win
    ys, xs = np.nonzero(win)
    return np.packbits(full, axis=1).reshape(-1), int(win.sum()), (x0 + int(xs.min()), y0 + int(ys.min()), x0 + int(xs.max()), y0 + int(ys.max()))


def instances(sizes, rng, dev):
    """K * M instances per image -> (SizedMasks with true areas and boxes, image ids, scores)."""
    rows, area, box, image, plane_sizes = [], [], [], [], []
    for b, (h, w) in enumerate(sizes):
        objects = [(int(rng.uniform(0.2, 0.8) * h), int(rng.uniform(0.2, 0.8) * w), int(rng.uniform(0.08, 0.2) * min(h, w))) for _ in range(3)]
        for _ in range(K):
            found = [(cy + int(rng.integers(-3, 4)), cx + int(rng.integers(-3, 4)), r + int(rng.integers(-2, 3))) for cy, cx, r in objects]
            found += [(int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(2, max(3, min(h, w) // 40)))) for _ in range(M - 3)]
            for cy, cx, r in found:
                bits, a, bx = disc(h, w, cy, cx, r)
                rows.append(bits), area.append(a), box.append(bx), image.append(b), plane_sizes.append((h, w))
    _, offsets, _ = sized_tables(plane_sizes)
    sized = SizedMasks(bits=torch.from_numpy(np.concatenate(rows)).to(dev), offsets=torch.from_numpy(offsets).to(dev),
                       area=torch.tensor(area, dtype=torch.int32, device=dev), box=torch.tensor(box, dtype=torch.int32, device=dev),
                       status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=plane_sizes, level=0)
    return sized, image, torch.from_numpy(rng.random(len(image)).astype(np.float32)).to(dev)


def host_greedy(job):
    """The textbook loop on one image: inter (D, D) symmetric, areas, scores -> keep."""
    inter, area, score, thr = job
    order = np.argsort(-score, kind="mergesort")
    gone, keep = np.zeros(len(area), bool), np.zeros(len(area), np.uint8)
    for r, i in enumerate(order):
        if gone[i] or area[i] < 1:
            continue
        keep[i] = 1
        later = order[r + 1:]
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.where(inter[i, later] > 0, inter[i, later] / (area[i] + area[later] - inter[i, later]).astype(np.float64), 0.0)
        gone[later[iou > thr]] = True
    return keep


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inter-only", action="store_true")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "nms_bench.log"))
    args = ap.parse_args()
    hip.load()
    pool = None if args.inter_only else multiprocessing.get_context("spawn").Pool(16)    # the workers start before the device is opened
    dev = torch.device("cuda:0")
    eng = Engine(dev)
    LOG = open(args.log, "w")
    say(f"# tools/bench_nms.py --rounds {args.rounds} --warmup {args.warmup}{' --inter-only' if args.inter_only else ''}   "
        f"{torch.cuda.get_device_name(0)}   library {os.path.relpath(os.environ.get('CVLM_PROBE_LIB') or hip.LIB_PATH, REPO)}")
    say(f"{'workload':18s} {'what':84s} median ms (min .. max)")
    rng = np.random.default_rng(30)
    ok = True
    for name, sizes in (("sweep 8 x 40", [((480, 640), (427, 640))[i % 2] for i in range(8)]), ("64 x 40 x 1024^2", [(1024, 1024)] * 64)):
        sized, image, scores = instances(sizes, rng, dev)
        Q = len(image)
        req = maskpost.nms_request(sized.sizes, image=image)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        dims_np, _, max_words = sized_tables(sized.sizes)
        dims, goff, member, poff = up(dims_np), up(req.group_offsets), up(req.member), up(req.pair_offsets)
        N = req.n_pairs
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        inter, status = i32(N), i32(1)
        tri = np.concatenate([[(req.member[m0 + i], req.member[m0 + j]) for i in range(m1 - m0) for j in range(i + 1, m1 - m0)]
                              for m0, m1 in zip(req.group_offsets[:-1], req.group_offsets[1:])]).astype(np.int32)
        sq = maskpost.pairs_request(sized.sizes, sized.sizes, a_image=image, b_image=image)
        tri_d, sq_d = up(tri), up(sq)
        inter_b, inter_c = i32(len(tri)), i32(len(sq))
        calls = {"a": lambda: hip.mask_nms_inter(sized.bits, sized.offsets, dims, sized.area, sized.box, goff, member, poff, inter, status),
                 "b": lambda: hip.mask_inter_sized(sized.bits, sized.offsets, dims, sized.bits, sized.offsets, dims, tri_d, max_words, inter_b, status),
                 "c": lambda: hip.mask_inter_sized(sized.bits, sized.offsets, dims, sized.bits, sized.offsets, dims, sq_d, max_words, inter_c, status)}
        t = {}
        for k, fn in list(calls.items())[:1 if args.inter_only else 3]:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t[k] = [event_ms(fn) for _ in range(args.rounds)]
        if args.inter_only:
            say(f"{name:18s} {'(a) cvlm_mask_nms_inter, device events':84s} {med(t['a'])}   sum of the intersections {int(inter.clamp(min=0).sum())}")
            continue
        a, b, c = inter.cpu().numpy(), inter_b.cpu().numpy(), inter_c.cpu().numpy()
        lookup = {(int(p), int(q)): int(v) for (p, q), v in zip(sq, c)}
        same_inter = np.array_equal(a, b) and all(lookup[(int(p), int(q))] == int(v) for (p, q), v in zip(tri, a))
        bx = sized.box.cpu().numpy()
        apart = sum(1 for p, q in tri if max(bx[p, 0], bx[q, 0]) > min(bx[p, 2], bx[q, 2]) or max(bx[p, 1], bx[q, 1]) > min(bx[p, 3], bx[q, 3]))

        def device_path():
            return eng.mask_nms_sized(sized, scores=scores, image=image)

        def host_path():
            ov = eng.mask_inter_sized(sized, sized, pairs=tri)
            got, area, sc = ov.inter.cpu().numpy(), sized.area.cpu().numpy(), scores.cpu().numpy()
            jobs, at = [], 0
            for m0, m1 in zip(req.group_offsets[:-1], req.group_offsets[1:]):
                D = int(m1 - m0)
                full = np.zeros((D, D), np.int64)
                full[np.triu_indices(D, 1)] = got[at:at + D * (D - 1) // 2]
                at += D * (D - 1) // 2
                rows = req.member[m0:m1]
                jobs.append((full + full.T, area[rows].astype(np.int64), sc[rows], 0.5))
            keep = np.zeros(Q, np.uint8)
            for (m0, m1), k in zip(zip(req.group_offsets[:-1], req.group_offsets[1:]), pool.map(host_greedy, jobs)):
                keep[req.member[m0:m1]] = k
            return keep

        t_dev, t_host, keep_dev, keep_host = [], [], None, None
        for i in range(args.warmup + args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = device_path()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            keep_host = host_path()
            t2 = time.perf_counter()
            keep_dev = out.keep.cpu().numpy()
            if i >= args.warmup:
                t_dev.append((t1 - t0) * 1e3), t_host.append((t2 - t1) * 1e3)
        same_keep = np.array_equal(keep_dev, keep_host) and out.status.cpu().tolist() == [0, 0]
        ok &= bool(same_inter and same_keep)
        mb = sum(4 * h * ((w + 31) // 32) for h, w in sized.sizes) / 2 ** 20
        say(f"{name:18s} {Q} instances in {len(sizes)} images, {mb:.0f} MiB of planes; {N} pairs in the triangles, {apart} of them ({100 * apart / N:.1f} %) "
            f"with boxes apart, {int((a == 0).sum())} without a shared pixel; {len(sq)} pairs for a_image = b_image; {int(keep_dev.sum())} instances kept")
        say(f"{name:18s} {'(a) cvlm_mask_nms_inter, device events':84s} {med(t['a'])}   sum of the intersections {int(inter.clamp(min=0).sum())}")
        say(f"{name:18s} {'(b) cvlm_mask_inter_sized on the triangles (pairs=), device events':84s} {med(t['b'])}")
        say(f"{name:18s} {'(c) cvlm_mask_inter_sized on a_image = b_image, device events':84s} {med(t['c'])}")
        say(f"{name:18s} {'(d) mask_nms_sized: request, upload, both entries; wall clock to the synchronisation':84s} {med(t_dev)}")
        say(f"{name:18s} {'(e) mask_inter_sized(pairs=), read back, greedy loop in numpy on 16 processes; wall clock':84s} {med(t_host)}")
        say(f"{name:18s} intersections of (a), (b) and (c) equal: {same_inter}; keep of (d) and (e) equal: {same_keep};  (b) / (a) = "
            f"{statistics.median(t['b']) / statistics.median(t['a']):.1f}x, (c) / (a) = {statistics.median(t['c']) / statistics.median(t['a']):.1f}x, "
            f"(e) / (d) = {statistics.median(t_host) / statistics.median(t_dev):.1f}x")
    if pool is not None:
        pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
