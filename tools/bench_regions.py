"""Instances on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/regions_bench.log).  Workloads of cvlm_mask_regions_sized at M = 8, connectivity 8, planes, tables, workspace and outputs
resident on the device:
  sweep            the 61-class sweep's sized planes, 8 images (480 x 640 and 427 x 640 in turn) x 61 hypotheses = 488 planes of two to
                   four blobs and some speckle each;
  64 x 1024^2      64 planes of 1024 x 1024 of the same kind.
Per workload, after --warmup untimed calls, --rounds calls: medians with min and max of
  (a) the entry with every plane in flight, by device events;
  (b) the entry with the minimum workspace (one plane per round), by device events;
  (c) the host alternative: the planes copied to the host, then per plane numpy.unpackbits, scipy.ndimage.label, the eight largest
      labels and a numpy.packbits per region, on 16 processes that were started before this process opened the device.
Gated: counts and tables of (a) and (b) equal the host alternative's, and the bytes of (a) and (b) are the same.
Then Cascade.classify_regions on the regions of --images images of the --geometry engine (demo: ViT-H / ViT-L at 1024 and 336)
against the same regions scored through host-built alphas -- the region planes copied to the host, unpacked, resized with
torch.nn.functional.interpolate, multiplied with the whole alphas, uploaded, and the same CLIP forwards --, wall clock to the
synchronisation.
`--kernels` runs (a) alone -- `--only TEXT`: of the workloads whose name holds TEXT --, for a `rocprofv3 --kernel-trace --stats --
python tools/bench_regions.py --kernels` run of its own.
Usage: python tools/bench_regions.py [--rounds N] [--warmup W] [--host-rounds H] [--geometry demo|tiny|none] [--images B] [--kernels [--only TEXT]]
                                     [--log PATH]"""
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
from bench_boundary import blobs, event_ms, med, sized_from  # noqa: E402
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.engine import SizedMasks, sized_tables  # noqa: E402

LOG = None
M = 8


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def scenes(h: int, w: int, n: int, rng) -> list:
    """n planes (h, w) bool: two to four blobs at a third of the size and a little speckle each."""
    out = []
    for _ in range(n):
        x = rng.random((h, w)) < 0.0005
        for b in blobs(h // 3, w // 3, int(rng.integers(2, 5)), rng):
            y0, x0 = int(rng.integers(0, h - h // 3)), int(rng.integers(0, w - w // 3))
            x[y0:y0 + h // 3, x0:x0 + w // 3] |= b
        out.append(x)
    return out


class Entry:
    """cvlm_mask_regions_sized on planes, tables, workspace and outputs resident on the device."""

    def __init__(self, sized: SizedMasks, dev):
        dims, _, self.max_words = sized_tables(sized.sizes)
        P, n = len(sized.sizes), int(sized.bits.numel())
        self.sized, self.dims = sized, torch.from_numpy(dims).to(dev)
        self.ws = torch.empty(hip.mask_regions_workspace_bytes(n, P, self.max_words), dtype=torch.uint8, device=dev)
        self.least = hip.mask_regions_workspace_bytes(4 * self.max_words, 1, self.max_words)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        self.n, self.table, self.status, self.out = i32(P), i32(P, M, 6), i32(1), torch.empty(M * n, dtype=torch.uint8, device=dev)

    def launch(self, rounds: bool = False):
        hip.mask_regions_sized(self.sized.bits, self.sized.offsets, self.dims, self.max_words, 8, 0, self.ws[:self.least] if rounds else self.ws,
                               self.n, self.table, self.out, self.status)


def host_task(job):
    """The host alternative for one plane -> (the number of regions, the areas of the eight largest, their packed planes' bytes)."""
    from scipy import ndimage
    rows, w = job
    x = np.unpackbits(rows, axis=1)[:, :w].astype(bool)
    lab, n = ndimage.label(x, structure=np.ones((3, 3), dtype=bool))
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    order = np.lexsort((np.arange(n), -area))[:M]                     # scipy numbers its labels in raster order of their first pixels
    wide = np.zeros((x.shape[0], rows.shape[1] * 8), dtype=bool)
    packed = 0
    for k in order:
        wide[:, :w] = lab == k + 1
        packed += np.packbits(wide, axis=1).size
    return n, area[order].tolist(), packed


def host_alternative(pool, sized: SizedMasks):
    t0 = time.perf_counter()
    raw = sized.bits.cpu().numpy()
    _, off, _ = sized_tables(sized.sizes)
    jobs = [(raw[off[p]:off[p + 1]].reshape(h, -1), w) for p, (h, w) in enumerate(sized.sizes)]
    res = pool.map(host_task, jobs, chunksize=max(1, len(jobs) // 64))
    return time.perf_counter() - t0, res


def bench_classify(args, dev, rng) -> bool:
    import torch.nn.functional as F
    from camouflaged_vlm_amd import host, spec, synth
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c = (spec.DEMO_SAM, spec.DEMO_CLIP) if args.geometry == "demo" else (spec.TINY_SAM, spec.TINY_CLIP)
    cas = Cascade({k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}, g, c, dev,
                  Precision.named("mx" if args.geometry == "demo" else "exact"))
    if args.geometry == "demo":
        consts = host.ovcamo_constants()
        eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
        cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    B, S, R = args.images, g.inp_size, c.image_resolution
    _, ci, _ = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=B))
    planes = scenes(S, S, B, rng)
    logits = torch.from_numpy(np.stack(planes)).to(dev).float().mul_(12).sub_(6).reshape(B, 1, S, S)      # sigmoid: 0.9975 inside, 0.0025 outside
    sizes = [((480, 640), (427, 640))[i % 2] for i in range(B)]

    def device_path():
        sized = cas.pack_masks_sized(logits, sizes)
        regions, plane_of, _ = cas.mask_regions_sized(sized, regions=M, min_area=64).compact()
        return regions, plane_of, cas.classify_regions(regions, plane_of, logits, ci)

    def host_path(regions, plane_of):
        alpha = F.interpolate(torch.sigmoid(logits), (R, R), mode="bilinear", align_corners=False).cpu()      # Cascade._alpha's, in torch
        raw = regions.bits.cpu().numpy()
        _, off, _ = sized_tables(regions.sizes)
        a = torch.empty(len(plane_of), 1, R, R)
        for q, (h, w) in enumerate(regions.sizes):
            x = np.unpackbits(raw[off[q]:off[q + 1]].reshape(h, -1), axis=1)[:, :w].astype(np.float32)
            a[q, 0] = alpha[int(plane_of[q]), 0] * F.interpolate(torch.from_numpy(x)[None, None], (R, R), mode="bilinear", align_corners=False)[0, 0]
        a = a.to(dev)
        out, chunk = [], cas.class_chunk()
        idx = torch.from_numpy(plane_of).to(dev)
        for q0 in range(0, len(plane_of), chunk):
            out.append(cas.clip.forward(ci.index_select(0, idx[q0:q0 + chunk]), a[q0:q0 + chunk])[3].clone())
        return torch.cat(out)

    regions, plane_of, got = device_path()
    got.check()
    ref = host_path(regions, plane_of)
    diff = float((got.logits - ref).abs().max())
    t_dev, t_cls, t_host = [], [], []
    for i in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        regions, plane_of, got = device_path()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        cas.classify_regions(regions, plane_of, logits, ci)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host_path(regions, plane_of)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= args.warmup:
            t_dev.append((t1 - t0) * 1e3), t_cls.append((t2 - t1) * 1e3), t_host.append((t3 - t2) * 1e3)
    name = f"{args.geometry}, {B} images"
    say(f"{name:20s} {len(plane_of)} regions of {B} planes, class chunk {cas.class_chunk()}; logits against the host-built alphas: max |diff| {diff:.2e}")
    say(f"{name:20s} {'pack_masks_sized + mask_regions_sized + compact + classify_regions':72s} {med(t_dev)}")
    say(f"{name:20s} {'classify_regions alone':72s} {med(t_cls)}")
    say(f"{name:20s} {'host-built alphas (copy, unpackbits, interpolate, upload) + the same forwards':72s} {med(t_host)}")
    return diff <= 1e-3


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--geometry", default="demo", choices=("demo", "tiny", "none"))
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "regions_bench.log"))
    args = ap.parse_args()
    hip.load()
    pool = None if args.kernels else multiprocessing.get_context("spawn").Pool(16)     # the workers start before the device is opened
    dev = torch.device("cuda:0")
    if not args.kernels:
        LOG = open(args.log, "w")
    say(f"# tools/bench_regions.py --rounds {args.rounds} --warmup {args.warmup} --host-rounds {args.host_rounds} --geometry {args.geometry} "
        f"--images {args.images}{' --kernels' if args.kernels else ''}   {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(29)
    work = {"sweep 8 x 61": Entry(sized_from([p for i in range(8) for p in scenes(*((480, 640), (427, 640))[i % 2], 61, rng)], dev), dev),
            "64 x 1024^2": Entry(sized_from(scenes(1024, 1024, 64, rng), dev), dev)}
    if args.kernels:
        for name, e in work.items():
            for _ in range(args.warmup + 5 if args.only in name else 0):
                e.launch()
        torch.cuda.synchronize()
        return 0
    ok = True
    say(f"{'workload':20s} {'what':72s} median ms (min .. max)")
    for name, e in work.items():
        t, outs = {}, {}
        for rounds in (False, True):
            for _ in range(args.warmup):
                e.launch(rounds)
            torch.cuda.synchronize()
            t[rounds] = [event_ms(lambda: e.launch(rounds)) for _ in range(args.rounds)]
            outs[rounds] = (e.n.cpu().tolist(), e.table[..., 0].cpu().tolist(), e.out.clone(), int(e.status.item()))
        t_host, ref = [], None
        for _ in range(args.host_rounds):
            s, ref = host_alternative(pool, e.sized)
            t_host.append(s * 1e3)
        want_n = [r[0] for r in ref]
        want_area = [r[1] + [0] * (M - len(r[1])) for r in ref]
        same = all(o[0] == want_n and o[1] == want_area and o[3] == 0 for o in outs.values()) and torch.equal(outs[False][2], outs[True][2])
        ok &= same
        pixels = sum(h * w for h, w in e.sized.sizes)
        say(f"{name:20s} {len(e.sized.sizes)} planes, {pixels / 1e6:.1f} Mpixel, {sum(want_n)} regions, {sum(min(n, M) for n in want_n)} kept; workspace "
            f"{e.ws.numel() / 2 ** 20:.0f} MiB in flight, {e.least / 2 ** 20:.1f} MiB at the least")
        m = statistics.median(t[False])
        say(f"{name:20s} {'(a) every plane in flight, device events':72s} {med(t[False])}   {pixels / m / 1e6:.2f} Gpixel/s")
        say(f"{name:20s} {'(b) the minimum workspace, one plane per round, device events':72s} {med(t[True])}")
        say(f"{name:20s} {'(c) copy + unpackbits + scipy.ndimage.label + packbits per region, 16 processes':72s} {med(t_host)}")
        say(f"{name:20s} counts and areas equal to the host alternative's, (a) and (b) the same bytes: {same};  host / (a) = "
            f"{statistics.median(t_host) / m:.0f}x")
    pool.close()
    if args.geometry != "none":
        ok &= bench_classify(args, dev, rng)
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
