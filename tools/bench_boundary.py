"""Boundary IoU on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/boundary_bench.log).  Workloads:
  sweep    the 61-class sweep's sized planes: B = 8 images of §19's eight photo sizes x 61 hypotheses, each at the published radius of
           its own size (0.02 of the diagonal);
  1024 d29 64 planes of 1024 x 1024 at d = 29, the published radius of that size;
  1024 d463 the same planes at the probe radius 463 (what 16384 x 16384 would take): the entry's time must not grow with the radius
           beyond what the warm-up rows of the column pass explain.
Per workload, after a warm-up, --rounds rounds, medians and ranges:
  (a) cvlm_mask_boundary_sized per call -- init, row pass, column pass -- by device events;
  (b) the host alternative: the planes copied to the host, numpy.unpackbits, scipy.ndimage.binary_erosion(iterations = d, border_value
      = 0) and X & ~ero, one plane per task on 16 processes.
And on the sweep's geometry at 480 x 640 (8 images x 61 hypotheses against 10 annotations each): Cascade.coco_match(boundary=0.02)
end to end against Cascade.coco_match(), wall clock to the synchronisation and device events.
Gated: the device's areas equal the host alternative's on every plane, and the device time `boundary=` adds to coco_match lies
below the host alternative's time for the same boundaries.
`--kernels` runs the entry of the three workloads alone -- `--only TEXT`: of those whose name holds TEXT --, for a `rocprofv3
--kernel-trace --stats -- python tools/bench_boundary.py --kernels --only "d = 463"` run of its own, which splits (a) into the two passes.
Usage: python tools/bench_boundary.py [--rounds N] [--warmup W] [--kernels [--only TEXT]] [--log PATH]"""
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
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.engine import MaskUtilities, SizedMasks, Workspace, boundary_radius, sized_tables  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]
LOG = None


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def med(v) -> str:
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class Engine(MaskUtilities):
    """The two attributes the packed-mask utilities use of an engine."""

    def __init__(self, dev):
        self.device, self.ws = dev, Workspace(dev)


def blobs(h: int, w: int, n: int, rng) -> np.ndarray:
    """n planes (n, h, w) bool: a disc with a wavy rim each, the kind of region a segmentation model returns."""
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    out = np.empty((n, h, w), dtype=bool)
    for i in range(n):
        cy, cx, r = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w, rng.uniform(0.15, 0.4) * min(h, w)
        ang = np.arctan2(yy - cy, xx - cx)
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= (r * (1 + 0.15 * np.sin(rng.integers(3, 9) * ang))) ** 2
    return out


def sized_from(planes, dev) -> SizedMasks:
    """Bool planes -> SizedMasks on the device, with areas and boxes of no meaning (the boundary entry reads neither)."""
    sizes = [tuple(p.shape) for p in planes]
    _, offsets, _ = sized_tables(sizes)
    rows = []
    for p in planes:
        h, w = p.shape
        full = np.zeros((h, 32 * ((w + 31) // 32)), dtype=np.uint8)
        full[:, :w] = p
        rows.append(np.packbits(full, axis=1).reshape(-1))
    P = len(planes)
    return SizedMasks(bits=torch.from_numpy(np.concatenate(rows)).to(dev), offsets=torch.from_numpy(offsets).to(dev),
                      area=torch.tensor([int(p.sum()) for p in planes], dtype=torch.int32, device=dev),
                      box=torch.zeros(P, 4, dtype=torch.int32, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=sizes, level=0)


class Entry:
    """cvlm_mask_boundary_sized on planes, tables and outputs resident on the device."""

    def __init__(self, sized: SizedMasks, radii, dev):
        dims, _, self.max_words = sized_tables(sized.sizes)
        self.sized, self.dims = sized, torch.from_numpy(dims).to(dev)
        self.radius = torch.tensor(radii, dtype=torch.int32, device=dev)
        self.ws, self.out = torch.empty_like(sized.bits), torch.empty_like(sized.bits)
        self.area = torch.empty(len(sized.sizes), dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)

    def launch(self):
        hip.mask_boundary_sized(self.sized.bits, self.sized.offsets, self.dims, self.radius, self.max_words, self.ws, self.out, self.area,
                                self.status)


def host_task(job):
    """The host alternative for one plane: unpack, scipy's iterated 3 x 3 erosion, the boundary's popcount."""
    from scipy import ndimage
    rows, w, d = job
    x = np.unpackbits(rows, axis=1)[:, :w].astype(bool)
    b = x & ~ndimage.binary_erosion(x, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
    return int(b.sum())


def host_alternative(pool, sized: SizedMasks, radii):
    """-> (seconds, the areas): the copy, then one task per plane."""
    t0 = time.perf_counter()
    raw = sized.bits.cpu().numpy()
    _, off, _ = sized_tables(sized.sizes)
    jobs = [(raw[off[p]:off[p + 1]].reshape(h, -1), w, int(radii[p])) for p, (h, w) in enumerate(sized.sizes)]
    res = pool.map(host_task, jobs, chunksize=max(1, len(jobs) // 64))
    return time.perf_counter() - t0, res


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "boundary_bench.log"))
    args = ap.parse_args()
    # the host alternative's workers start before this process opens the device
    pool = None if args.kernels else multiprocessing.get_context("spawn").Pool(16)
    dev = torch.device("cuda:0")
    if not args.kernels:
        LOG = open(args.log, "w")
    say(f"# tools/bench_boundary.py --rounds {args.rounds} --warmup {args.warmup}{' --kernels' if args.kernels else ''}   {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(25)
    sweep_planes = [p for s in PHOTO_SIZES for p in blobs(*s, 61, rng)]
    sweep = sized_from(sweep_planes, dev)
    big = sized_from(list(blobs(1024, 1024, 64, rng)), dev)
    work = {"sweep 8 x 61": Entry(sweep, [boundary_radius(h, w) for h, w in sweep.sizes], dev),
            "64 x 1024^2, d = 29": Entry(big, [29] * 64, dev), "64 x 1024^2, d = 463": Entry(big, [463] * 64, dev)}
    if args.kernels:
        for name, e in work.items():
            for _ in range(args.warmup + 10 if args.only in name else 0):
                e.launch()
        torch.cuda.synchronize()
        return 0
    ok = True
    medians = {}
    say(f"{'workload':24s} {'what':52s} median ms (range)")
    for name, e in work.items():
        for _ in range(args.warmup):
            e.launch()
        torch.cuda.synchronize()
        t_dev = [event_ms(e.launch) for _ in range(args.rounds)]
        radii = e.radius.cpu().tolist()
        t_host, areas = [], None
        for _ in range(2 if "463" in name else args.rounds):      # scipy's cost grows with d: two rounds of the probe radius are enough
            t, areas = host_alternative(pool, e.sized, radii)
            t_host.append(t * 1e3)
        same = e.status.item() == 0 and e.area.cpu().tolist() == areas
        ok &= same
        medians[name] = (statistics.median(t_dev), statistics.median(t_host))
        say(f"{name:24s} {'(a) cvlm_mask_boundary_sized, device events':52s} {med(t_dev)}")
        say(f"{name:24s} {'(b) copy + unpackbits + scipy erosion, 16 processes':52s} {med(t_host)}")
        say(f"{name:24s} areas equal to the host alternative's: {same};  host / device = {medians[name][1] / medians[name][0]:.0f}x")
    a, b = medians["64 x 1024^2, d = 29"][0], medians["64 x 1024^2, d = 463"][0]
    say(f"radius independence: d = 463 takes {b / a:.2f}x the time of d = 29 on the same planes (DESIGN.md §25 says what the segments explain)")
    # coco_match with and without boundary=, 8 images of 480 x 640, 61 hypotheses against 10 annotations each
    eng = Engine(dev)
    h, w = 480, 640
    dets, gts = sized_from(list(blobs(h, w, 8 * 61, rng)), dev), sized_from(list(blobs(h, w, 8 * 10, rng)), dev)
    det_image, gt_image = [i // 61 for i in range(8 * 61)], [i // 10 for i in range(8 * 10)]
    scores = torch.rand(8 * 61, device=dev)
    kw = dict(scores=scores, det_image=det_image, gt_image=gt_image)
    runs = {"coco_match()": lambda: eng.coco_match(dets, gts, **kw), "coco_match(boundary=0.02)": lambda: eng.coco_match(dets, gts, boundary=0.02, **kw)}
    runs["coco_match(boundary=0.02)"]().check()
    t_wall, t_event = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t_wall[k].append((time.perf_counter() - t0) * 1e3)
            t_event[k].append(event_ms(fn))
    t_host = []
    for _ in range(args.rounds):
        td, _ = host_alternative(pool, dets, [16] * len(dets.sizes))
        tg, _ = host_alternative(pool, gts, [16] * len(gts.sizes))
        t_host.append((td + tg) * 1e3)
    for k in runs:
        say(f"{'sweep at 480 x 640':24s} {k + ', wall clock':52s} {med(t_wall[k])}")
        say(f"{'sweep at 480 x 640':24s} {k + ', device events around the call':52s} {med(t_event[k])}")
    say(f"{'sweep at 480 x 640':24s} {'the host alternative for the same 568 boundaries':52s} {med(t_host)}")
    added = statistics.median(t_event["coco_match(boundary=0.02)"]) - statistics.median(t_event["coco_match()"])
    m_host = statistics.median(t_host)
    say(f"boundary= adds {added:.3f} ms to coco_match by device events;  host alternative / added = {m_host / max(added, 1e-6):.0f}x;  "
        f"added below host: {added < m_host}")
    ok &= added < m_host
    pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
