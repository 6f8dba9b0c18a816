"""Thinning of sized planes on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/thin_bench.log).  Workloads of cvlm_mask_thin_sized, planes, tables, workspace and outputs resident on the device, every plane
thinned to its fixed point:
  sweep              the 61-class sweep's sized planes, 8 images (480 x 640 and 427 x 640 in turn) x 61 hypotheses = 488 blobs;
  64 x 1024^2 blobs  64 planes of 1024 x 1024, a blob each: hundreds of iterations;
  64 x 1024^2 edges  64 planes of 1024 x 1024, the rim of a blob five pixels thick each, as a thresholded edge map is: few iterations.
Per workload, after --warmup untimed calls, --rounds calls: medians with min and max of
  (a) mode 0, the resident kernel, by device events;
  (b) mode 1, the stepping kernels with as many steps as the slowest plane needs and one more, by device events;
  (c) the host alternative: the planes copied to the host and the sequential host entry, one plane per task on 16 threads that were
      started fresh before this process opened the device (--host-rounds calls);
with the iterations of the workload and pixels and pixel-iterations per second.  And Cascade.mask_thin_sized under path="auto" and
path="steps" (rounds of 64 iterations, one read each) and Cascade.mask_cldice on the sweep's geometry at 480 x 640, 488 predictions
against 10 annotations per image (4880 pairs), wall clock to the synchronisation and device events.
Gated: areas, boxes and iteration counts of (a) and (b) equal the host entry's, plane for plane.
`--kernels` runs (a) and (b) of the three workloads alone -- `--only TEXT`: of those whose name holds TEXT --, for a `rocprofv3
--kernel-trace --stats -- python tools/bench_thin.py --kernels` run of its own.
Usage: python tools/bench_thin.py [--rounds N] [--warmup W] [--host-rounds H] [--kernels [--only TEXT]] [--log PATH]"""
import argparse
import os
import statistics
import sys
import time
from multiprocessing.pool import ThreadPool

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_boundary import Engine, blobs, event_ms, med, sized_from  # noqa: E402
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.engine import SizedMasks, sized_tables  # noqa: E402

LOG = None


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def rims(h: int, w: int, n: int, rng, half: float = 2.5) -> np.ndarray:
    """n planes (n, h, w) bool: the rim of a wavy disc, 2 * half pixels thick -- what a thresholded edge probability looks like."""
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    out = np.empty((n, h, w), dtype=bool)
    for i in range(n):
        cy, cx, r = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w, rng.uniform(0.15, 0.4) * min(h, w)
        ang = np.arctan2(yy - cy, xx - cx)
        out[i] = np.abs(np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r * (1 + 0.15 * np.sin(rng.integers(3, 9) * ang))) <= half
    return out


class Entry:
    """cvlm_mask_thin_sized on planes, tables, workspace and outputs resident on the device."""

    def __init__(self, sized: SizedMasks, dev):
        dims, _, self.max_words = sized_tables(sized.sizes)
        P = len(sized.sizes)
        self.sized, self.dims = sized, torch.from_numpy(dims).to(dev)
        self.limits = torch.zeros(P, dtype=torch.int32, device=dev)
        self.ws = torch.empty(hip.mask_thin_workspace_bytes(sized.bits.numel(), P, hip.THIN_MAX_STEPS), dtype=torch.uint8, device=dev)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        self.out, self.area, self.box, self.iters, self.done, self.status = torch.empty_like(sized.bits), i32(P), i32(P, 4), i32(P), i32(P), i32(1)
        self.steps = hip.THIN_MAX_STEPS

    def launch(self, mode: int):
        steps = self.steps if mode else 0
        hip.mask_thin_sized(self.sized.bits, self.sized.offsets, self.dims, self.limits, self.max_words, mode, steps,
                            self.ws[:hip.mask_thin_workspace_bytes(self.sized.bits.numel(), len(self.sized.sizes), steps)], self.out, self.area,
                            self.box, self.iters, self.done, self.status)

    def tables(self):
        return (self.area.cpu().tolist(), self.box.cpu().tolist(), self.iters.cpu().tolist(), self.done.cpu().tolist(), int(self.status.item()))


def host_task(job):
    """The host alternative for one plane: the sequential host entry on its bytes."""
    rows, h, w = job
    bits = torch.from_numpy(rows)
    off = torch.tensor([0, rows.size], dtype=torch.int64)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
    area, box, iters, done, status = i32(1), i32(1, 4), i32(1), i32(1), i32(1)
    ws = torch.empty(hip.mask_thin_workspace_bytes(rows.size, 1, 1), dtype=torch.uint8)
    hip.mask_thin_sized_host(bits, off, torch.tensor([[h, w]], dtype=torch.int32), torch.zeros(1, dtype=torch.int32), h * ((w + 31) // 32), 0, 1,
                             ws, torch.empty_like(bits), area, box, iters, done, status)
    return int(area[0]), box[0].tolist(), int(iters[0])


def host_alternative(pool, sized: SizedMasks):
    """-> (seconds, [(area, box, iters)]): the copy, then one task per plane."""
    t0 = time.perf_counter()
    raw = sized.bits.cpu().numpy()
    _, off, _ = sized_tables(sized.sizes)
    jobs = [(raw[off[p]:off[p + 1]].copy(), h, w) for p, (h, w) in enumerate(sized.sizes)]
    res = pool.map(host_task, jobs, chunksize=1)
    return time.perf_counter() - t0, res


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "thin_bench.log"))
    args = ap.parse_args()
    hip.load()
    pool = None if args.kernels else ThreadPool(16)                   # the host alternative's threads start before the device is opened
    dev = torch.device("cuda:0")
    if not args.kernels:
        LOG = open(args.log, "w")
    say(f"# tools/bench_thin.py --rounds {args.rounds} --warmup {args.warmup} --host-rounds {args.host_rounds}{' --kernels' if args.kernels else ''}"
        f"   {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(28)
    work = {"sweep 8 x 61": Entry(sized_from([p for i in range(8) for p in blobs(*((480, 640), (427, 640))[i % 2], 61, rng)], dev), dev),
            "64 x 1024^2 blobs": Entry(sized_from(list(blobs(1024, 1024, 64, rng)), dev), dev),
            "64 x 1024^2 edges": Entry(sized_from(list(rims(1024, 1024, 64, rng)), dev), dev)}
    ok = True
    for name, e in work.items():                                      # the resident kernel first: its iteration counts size the steps
        e.launch(0)
        e.steps = min(hip.THIN_MAX_STEPS, int(e.iters.max().item()) + 1)
    if args.kernels:
        for name, e in work.items():
            for mode in (0, 1):
                for _ in range(args.warmup + 5 if args.only in name else 0):
                    e.launch(mode)
        torch.cuda.synchronize()
        return 0
    say(f"{'workload':20s} {'what':62s} median ms (min .. max)")
    for name, e in work.items():
        got, t_mode = {}, {}
        for mode in (0, 1):
            for _ in range(args.warmup):
                e.launch(mode)
            torch.cuda.synchronize()
            t_mode[mode] = [event_ms(lambda: e.launch(mode)) for _ in range(args.rounds)]
            got[mode] = e.tables()
        t_host, ref = [], None
        for _ in range(args.host_rounds):
            t, ref = host_alternative(pool, e.sized)
            t_host.append(t * 1e3)
        P = len(e.sized.sizes)
        want = ([r[0] for r in ref], [r[1] for r in ref], [r[2] for r in ref], [1] * P, 0)
        same = got[0] == want and got[1] == want
        ok &= same
        pixels = sum(h * w for h, w in e.sized.sizes)
        work_px = sum(h * w * (n + 1) for (h, w), n in zip(e.sized.sizes, want[2]))
        say(f"{name:20s} iterations: median {int(statistics.median(want[2]))}, max {max(want[2])}; pixels left: {sum(want[0])} of "
            f"{int(e.sized.area.sum().item())}; stepping path at steps = {e.steps}")
        for mode, what in ((0, "(a) mode 0, resident kernel, device events"), (1, "(b) mode 1, stepping kernels, device events")):
            m = statistics.median(t_mode[mode])
            say(f"{name:20s} {what:62s} {med(t_mode[mode])}   {pixels / m / 1e6:.3f} Gpixel/s, {work_px / m / 1e6:.1f} Gpixel-iterations/s")
        say(f"{name:20s} {'(c) copy + the host entry, 16 threads':62s} {med(t_host)}")
        say(f"{name:20s} tables equal to the host entry's: {same};  stepping / resident = "
            f"{statistics.median(t_mode[1]) / statistics.median(t_mode[0]):.2f}x, host / resident = "
            f"{statistics.median(t_host) / statistics.median(t_mode[0]):.0f}x")
    # through the engine: 8 images of 480 x 640, 61 predictions against 10 annotations each
    eng = Engine(dev)
    dets, gts = sized_from(list(blobs(480, 640, 8 * 61, rng)), dev), sized_from(list(blobs(480, 640, 8 * 10, rng)), dev)
    pairs = [(p, 10 * (p // 61) + q) for p in range(8 * 61) for q in range(10)]
    runs = {"mask_thin_sized(path='auto')": lambda: eng.mask_thin_sized(dets),
            "mask_thin_sized(path='steps', steps=64)": lambda: eng.mask_thin_sized(dets, path="steps"),
            "mask_cldice(), 4880 pairs": lambda: eng.mask_cldice(dets, gts, pairs=pairs)}
    for fn in runs.values():
        fn().check()
    a, b = runs["mask_thin_sized(path='auto')"](), runs["mask_thin_sized(path='steps', steps=64)"]()
    ok &= torch.equal(a.masks.bits, b.masks.bits) and torch.equal(a.iters, b.iters)
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
    for k in runs:
        say(f"{'sweep at 480 x 640':20s} {k + ', wall clock':62s} {med(t_wall[k])}")
        say(f"{'sweep at 480 x 640':20s} {k + ', device events':62s} {med(t_event[k])}")
    pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
