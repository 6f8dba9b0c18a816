"""Distance maps and surface distances on the device, timed.  One process; every line goes to stdout and to --log
(default profiles/distance_bench.log).  Workloads of cvlm_mask_distance_sized, planes, tables and outputs resident on the device:
  sweep            the 61-class sweep's sized planes, 8 images (480 x 640 and 427 x 640 in turn) x 61 hypotheses = 488, unlimited reach;
  sweep, tolerance the same planes, each at the reach of its own tolerance (`surface_tolerance`: 7 pixels);
  64 x 1024^2      64 planes of 1024 x 1024, unlimited reach;
  one corner pixel one plane of 1024 x 1024 with one set pixel in a corner, unlimited reach: the adverse plane, every pixel of a column
                   searches the whole column.
Per workload, after --warmup untimed calls, --rounds calls: medians with min and max of
  (a) the entry per call -- init, row pass, column pass -- by device events;
  (b) the host alternative: the planes copied to the host, numpy.unpackbits and scipy.ndimage.distance_transform_edt, one plane per
      task on 16 processes that were started fresh before this process opened the device.
And Cascade.mask_surface_distances end to end on the sweep's geometry at 480 x 640, 488 predictions against 10 annotations per image
(4880 pairs, both directions, the boundaries included), unlimited and at reach="tolerance", wall clock to the synchronisation and
device events, against the host alternative for the maps of the same 568 surfaces alone.
Gated: the sum of every plane's map equals the host alternative's (squared distances recomputed in integers from scipy's indices).
`--kernels` runs the entries of the four workloads alone -- `--only TEXT`: of those whose name holds TEXT --, for a `rocprofv3
--kernel-trace --stats -- python tools/bench_distance.py --kernels` run of its own, which splits (a) into the passes.
Usage: python tools/bench_distance.py [--rounds N] [--warmup W] [--kernels [--only TEXT]] [--log PATH]"""
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
from bench_boundary import Engine, blobs, event_ms, med, sized_from  # noqa: E402
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.engine import SizedMasks, label_tables, sized_tables, surface_tolerance  # noqa: E402

LOG = None


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


class Entry:
    """cvlm_mask_distance_sized on planes, tables, workspace and output resident on the device."""

    def __init__(self, sized: SizedMasks, reach, dev):
        dims, _, self.max_words = sized_tables(sized.sizes)
        _, pix, _ = label_tables(sized.sizes)
        self.sized, self.dims, self.pix = sized, torch.from_numpy(dims).to(dev), torch.from_numpy(pix).to(dev)
        self.reach = torch.tensor(reach, dtype=torch.int32, device=dev)
        n_pix = int(pix[-1])
        self.d2 = torch.empty(n_pix, dtype=torch.int32, device=dev)
        self.ws = torch.empty((2 * n_pix + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.host_pix = pix

    def launch(self):
        hip.mask_distance_sized(self.sized.bits, self.sized.offsets, self.dims, self.reach, self.max_words, self.pix, self.ws, self.d2, self.status)

    def sums(self):
        """The sum of each plane's map, far entries left out, and their count: what the gate compares."""
        d2 = self.d2.cpu().numpy().astype(np.int64)
        far = d2 == hip.DT_FAR
        d2[far] = 0
        cuts = self.host_pix[:-1]
        return list(zip(np.add.reduceat(d2, cuts).tolist(), np.add.reduceat(far.astype(np.int64), cuts).tolist()))


def host_task(job):
    """The host alternative for one plane: unpack, scipy's exact transform, the squared distances from its indices in integers."""
    from scipy import ndimage
    rows, w, reach = job
    x = np.unpackbits(rows, axis=1)[:, :w].astype(bool)
    if not x.any():
        return 0, x.size
    iy, ix = ndimage.distance_transform_edt(~x, return_indices=True, return_distances=False)
    yy, xx = np.mgrid[0:x.shape[0], 0:w]
    d2 = (yy - iy).astype(np.int64) ** 2 + (xx - ix).astype(np.int64) ** 2
    far = d2 > reach * reach if reach else np.zeros(d2.shape, dtype=bool)
    return int(d2[~far].sum()), int(far.sum())


def host_alternative(pool, sized: SizedMasks, reach):
    """-> (seconds, the gate's sums): the copy, then one task per plane."""
    t0 = time.perf_counter()
    raw = sized.bits.cpu().numpy()
    _, off, _ = sized_tables(sized.sizes)
    jobs = [(raw[off[p]:off[p + 1]].reshape(h, -1), w, int(reach[p])) for p, (h, w) in enumerate(sized.sizes)]
    res = pool.map(host_task, jobs, chunksize=max(1, len(jobs) // 64))
    return time.perf_counter() - t0, [tuple(r) for r in res]


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "distance_bench.log"))
    args = ap.parse_args()
    # the host alternative's workers start before this process opens the device
    pool = None if args.kernels else multiprocessing.get_context("spawn").Pool(16)
    dev = torch.device("cuda:0")
    if not args.kernels:
        LOG = open(args.log, "w")
    say(f"# tools/bench_distance.py --rounds {args.rounds} --warmup {args.warmup}{' --kernels' if args.kernels else ''}   {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(27)
    sweep = sized_from([p for i in range(8) for p in blobs(*((480, 640), (427, 640))[i % 2], 61, rng)], dev)
    big = sized_from(list(blobs(1024, 1024, 64, rng)), dev)
    corner = np.zeros((1024, 1024), dtype=bool)
    corner[0, 0] = True
    work = {"sweep 8 x 61": Entry(sweep, [0] * 488, dev),
            "sweep 8 x 61, tolerance": Entry(sweep, [surface_tolerance(h, w) for h, w in sweep.sizes], dev),
            "64 x 1024^2": Entry(big, [0] * 64, dev), "one corner pixel": Entry(sized_from([corner], dev), [0], dev)}
    if args.kernels:
        for name, e in work.items():
            for _ in range(args.warmup + 10 if args.only in name else 0):
                e.launch()
        torch.cuda.synchronize()
        return 0
    ok = True
    say(f"{'workload':24s} {'what':56s} median ms (min .. max)")
    for name, e in work.items():
        for _ in range(args.warmup):
            e.launch()
        torch.cuda.synchronize()
        t_dev = [event_ms(e.launch) for _ in range(args.rounds)]
        reach = e.reach.cpu().tolist()
        t_host, sums = [], None
        for _ in range(args.rounds):
            t, sums = host_alternative(pool, e.sized, reach)
            t_host.append(t * 1e3)
        same = e.status.item() == 0 and e.sums() == sums
        ok &= same
        pixels = int(e.host_pix[-1])
        say(f"{name:24s} {'(a) cvlm_mask_distance_sized, device events':56s} {med(t_dev)}   {pixels / statistics.median(t_dev) / 1e6:.2f} Gpixel/s")
        say(f"{name:24s} {'(b) copy + unpackbits + scipy EDT, 16 processes':56s} {med(t_host)}")
        say(f"{name:24s} sums equal to the host alternative's: {same};  host / device = {statistics.median(t_host) / statistics.median(t_dev):.0f}x")
    # mask_surface_distances end to end: 8 images of 480 x 640, 61 predictions against 10 annotations each
    eng = Engine(dev)
    dets, gts = sized_from(list(blobs(480, 640, 8 * 61, rng)), dev), sized_from(list(blobs(480, 640, 8 * 10, rng)), dev)
    pairs = [(p, 10 * (p // 61) + q) for p in range(8 * 61) for q in range(10)]
    runs = {"mask_surface_distances()": lambda: eng.mask_surface_distances(dets, gts, pairs=pairs),
            "mask_surface_distances(reach='tolerance')": lambda: eng.mask_surface_distances(dets, gts, pairs=pairs, reach="tolerance")}
    for fn in runs.values():
        fn().check()
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
        td, _ = host_alternative(pool, dets, [0] * len(dets.sizes))
        tg, _ = host_alternative(pool, gts, [0] * len(gts.sizes))
        t_host.append((td + tg) * 1e3)
    for k in runs:
        say(f"{'sweep at 480 x 640':24s} {k + ', wall clock':56s} {med(t_wall[k])}")
        say(f"{'sweep at 480 x 640':24s} {k + ', device events':56s} {med(t_event[k])}")
    say(f"{'sweep at 480 x 640':24s} {'the host alternative for the maps of the 568 planes alone':56s} {med(t_host)}")
    pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
