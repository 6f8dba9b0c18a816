"""COCO matching on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/match_bench.log).  Two workloads:
  sweep   the project's sweep, class-agnostic: 8 images x 61 hypotheses against 10 annotations each (8 groups of 61 x 10);
  coco    a COCO-like table: 2 000 (image, category) groups of 20 detections x 7 annotations.
Per workload, after a warm-up, --rounds alternating rounds, medians and ranges:
  (a) cvlm_coco_match per launch on tables resident on the device, by device events;
  (b) sweep only: Cascade.coco_match end to end -- request, uploads, cvlm_mask_inter_sized, gathers, cvlm_coco_match -- on planes of
      480 x 640, wall clock to the synchronisation;
  (c) the host alternative: the IoUs read back (SizedOverlaps.iou() for the sweep; the same formula in numpy for the table, plus the
      read of inter) and the published loops of tests/match_oracle.py, one group per task on at most 16 processes.
Gated: the device's tables equal the host entry's, which the tests hold against the loops, and (a), the added device time, lies below (c).
`--only-kernel` runs (a) of both workloads alone, for a `rocprofv3 --kernel-trace --stats -- python tools/bench_match.py --only-kernel`
run of its own.
Usage: python tools/bench_match.py [--rounds N] [--warmup W] [--only-kernel] [--log PATH]"""
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import match_oracle as MO  # noqa: E402
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.engine import MaskUtilities, Workspace  # noqa: E402

LOG = None
TABLES = ("dt_order", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


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


def table_groups(E: int, D: int, G: int, seed: int):
    """Groups with areas across COCO's ranges; a detection overlaps one annotation well and the others a little."""
    rng = np.random.default_rng(seed)
    groups = []
    for _ in range(E):
        ga = rng.integers(200, 30000, G)
        da = rng.integers(200, 30000, D)
        inter = (rng.random((D, G)) * 0.2 * np.minimum(da[:, None], ga[None, :])).astype(np.int64)
        hit = rng.integers(0, G, D)
        inter[np.arange(D), hit] = (rng.uniform(0.3, 1.0, D) * np.minimum(da, ga[hit])).astype(np.int64)
        groups.append(dict(inter=inter, det_area=da, scores=rng.random(D).astype(np.float32), gt_area=ga, range_area=None,
                           iscrowd=(rng.random(G) < 0.05).astype(np.uint8)))
    return groups


def oracle_task(group):
    return [r["dtm"].sum() for r in MO.evaluate_group(group)]


class Device:
    """cvlm_coco_match on tables resident on the device."""

    def __init__(self, groups, dev):
        self.tabs = MO.tables(groups)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = self.tabs
        A, T, ND, NG = 4, 10, len(t["det_area"]), len(t["gt_area"])
        self.args = [up(t[k]) for k in ("det_offsets", "gt_offsets", "pair_offsets", "inter", "det_area", "score", "gt_area", "gt_range_area", "gt_crowd")]
        self.args += [up(MO.IOU_THRS), up(np.asarray(MO.AREA_RNGS, dtype=np.float64)), 100]
        self.outs = [torch.empty(s, dtype=d, device=dev) for s, d in (((ND,), torch.int32), ((A, T, ND), torch.int32), ((A, T, ND), torch.uint8),
                                                                      ((A, T, NG), torch.int32), ((A, NG), torch.uint8), ((1,), torch.int32))]

    def launch(self):
        hip.coco_match(*self.args, *self.outs)

    def equals_host(self) -> bool:
        self.launch()
        host = MO.run_entry(hip.coco_match_host, self.tabs)
        return int(self.outs[5].item()) == 0 and all(np.array_equal(o.cpu().numpy(), host[k]) for o, k in zip(self.outs, TABLES))


class Engine(MaskUtilities):
    """The two attributes the packed-mask utilities use of an engine."""

    def __init__(self, dev):
        self.device, self.ws = dev, Workspace(dev)


def discs(h, w, n, rng):
    yy, xx = np.mgrid[:h, :w]
    out = []
    for _ in range(n):
        cy, cx, r = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w, rng.uniform(0.1, 0.3) * min(h, w)
        out.append((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    return out


def counts_of(mask: np.ndarray) -> list:
    f = np.ascontiguousarray(mask.T).reshape(-1).view(np.int8)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0).tolist()


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-kernel", action="store_true")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "match_bench.log"))
    args = ap.parse_args()
    # the host alternative's workers start before this process opens the device
    pool = None if args.only_kernel else multiprocessing.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    if not args.only_kernel:
        LOG = open(args.log, "w")
    say(f"# tools/bench_match.py --rounds {args.rounds} --warmup {args.warmup}{' --only-kernel' if args.only_kernel else ''}   {torch.cuda.get_device_name(0)}")
    ok = True
    work = {"sweep 8 x (61 x 10)": table_groups(8, 61, 10, 1), "coco 2000 x (20 x 7)": table_groups(2000, 20, 7, 2)}
    devs = {name: Device(groups, dev) for name, groups in work.items()}
    if args.only_kernel:
        for d in devs.values():
            for _ in range(args.warmup + 20):
                d.launch()
        torch.cuda.synchronize()
        return 0
    # the sweep through Cascade.coco_match: 8 images of 480 x 640, 61 hypotheses and 10 annotations each
    rng = np.random.default_rng(3)
    eng = Engine(dev)
    h, w = 480, 640
    coco = lambda ms: [{"size": [h, w], "counts": counts_of(m)} for m in ms]
    dets, gts = eng.rle_decode(coco(discs(h, w, 8 * 61, rng))), eng.rle_decode(coco(discs(h, w, 8 * 10, rng)))
    det_image, gt_image = [i // 61 for i in range(8 * 61)], [i // 10 for i in range(8 * 10)]
    scores = torch.rand(8 * 61, device=dev)
    e2e = lambda: eng.coco_match(dets, gts, scores=scores, det_image=det_image, gt_image=gt_image)
    m = e2e()
    m.check()
    say(f"{'workload':24s} {'what':44s} median ms (range)")
    for name, groups in work.items():
        d = devs[name]
        same = d.equals_host()
        ok &= same
        for _ in range(args.warmup):
            d.launch()
            if name.startswith("sweep"):
                e2e()
        torch.cuda.synchronize()
        t_dev, t_e2e, t_host = [], [], []
        inter_dev = d.args[3]
        for _ in range(args.rounds):
            t_dev.append(event_ms(d.launch))
            if name.startswith("sweep"):
                t0 = time.perf_counter()
                r = e2e()
                torch.cuda.synchronize()
                t_e2e.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                ious = r.overlaps.iou()                               # the read-back of the host route
                back = time.perf_counter() - t0
                assert ious.size == 8 * 61 * 10
            else:
                t0 = time.perf_counter()
                inter_dev.cpu().numpy()
                back = time.perf_counter() - t0
            t0 = time.perf_counter()
            pool.map(oracle_task, groups, chunksize=max(1, len(groups) // 64))
            t_host.append((back + time.perf_counter() - t0) * 1e3)
        m_dev, m_host = statistics.median(t_dev), statistics.median(t_host)
        say(f"{name:24s} {'(a) cvlm_coco_match, device events':44s} {med(t_dev)}")
        if t_e2e:
            say(f"{name:24s} {'(b) coco_match end to end, wall clock':44s} {med(t_e2e)}")
        say(f"{name:24s} {'(c) IoUs read back + published loops, host':44s} {med(t_host)}")
        say(f"{name:24s} equal to the host entry: {same};  host / device = {m_host / m_dev:.0f}x;  device below host: {m_dev < m_host}")
        ok &= m_dev < m_host
    pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
