"""Rendering on the device, timed.  One process; every line goes to stdout and to --log (default
profiles/render_bench.log).  Workloads, images, sources, tables and outputs resident on the device:
  sweep 8 x 5          the B = 8, K = 5 sweep's sized planes drawn over synthetic photographs at the sweep's sizes (480 x 640 and 427 x
                       640 in turn): five fills per image, one colour each, alpha 0.5;
  64 x 1024^2, 1 fill  64 images of 1024 x 1024 with one fill each;
  64 x 1024^2, 8 fills the same with eight fills each;
  64 x 1024^2, edges   the same with one LABELS layer with EDGES: 19 ids in blocks, the segment outlines painted at alpha 1.
Per workload, after --warmup untimed calls, --rounds calls: medians with min and max of
  (a) cvlm_render into a second buffer, by device events;
  (b) cvlm_render in place, by device events (the bytes after the first in-place call are painted again: the same traffic);
  (c) a device-to-device `copy_` of the same image buffer, by device events -- the traffic floor of (a);
  (d) the host alternative on --host-rounds rounds: the sources read back, np.unpackbits (np.roll comparisons for the edges), the
      blend rule in float32 numpy on 16 threads over the photographs the host already holds; no upload counted; wall clock.
Gated: the bytes of (a) equal those of (d), and the status word is 0.
`--kernels` runs (a) of the workloads alone, --repeat calls each -- `--only TEXT`: of those whose name holds TEXT --, for a `rocprofv3
--kernel-trace --stats -- python tools/bench_render.py --kernels` run of its own.
Usage: python tools/bench_render.py [--rounds N] [--warmup W] [--host-rounds H] [--kernels [--only TEXT] [--repeat R]] [--log PATH]"""
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
from bench_boundary import blobs, event_ms, med  # noqa: E402
from camouflaged_vlm_amd import hip, maskpost  # noqa: E402

LOG = None
COLORS = [(0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 128, 0), (128, 0, 255)]


def say(line: str) -> None:
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def pack(mask: np.ndarray) -> np.ndarray:
    h, w = mask.shape
    full = np.zeros((h, 32 * ((w + 31) // 32)), dtype=np.uint8)
    full[:, :w] = mask
    return np.packbits(full, axis=1).reshape(-1)


def blend(c: np.ndarray, col, a: float) -> np.ndarray:
    a = np.float32(a)
    return np.clip(np.rint(c.astype(np.float32) * (np.float32(1.0) - a) + np.asarray(col, np.float32) * a), 0, 255).astype(np.uint8)


def edges_of(ids: np.ndarray) -> np.ndarray:
    e = np.zeros(ids.shape, dtype=bool)
    e[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    e[:, :-1] |= ids[:, :-1] != ids[:, 1:]
    e[1:, :] |= ids[1:, :] != ids[:-1, :]
    e[:-1, :] |= ids[:-1, :] != ids[1:, :]
    return e


def host_fills(job):
    """One image of the host alternative: its packed planes, unpacked and blended in turn."""
    photo, planes, alpha = job
    out = photo.copy()
    h, w = photo.shape[:2]
    for k, rows in enumerate(planes):
        m = np.unpackbits(rows.reshape(h, -1), axis=1)[:, :w].astype(bool)
        out[m] = blend(out[m], COLORS[k % len(COLORS)], alpha)
    return out


def host_edges(job):
    photo, ids, pal = job
    out = photo.copy()
    e = edges_of(ids)
    out[e] = pal[ids[e]]                                              # alpha 1: the colour itself
    return out


class Workload:
    """Images, sources and tables of one workload on the device, and what its host alternative needs."""

    def __init__(self, name, photos, dev, *, planes=None, ids=None, alpha=0.5):
        self.name, self.photos, self.alpha = name, photos, alpha
        sizes = [p.shape[:2] for p in photos]
        self.images = maskpost.sized_images(photos, dev)
        self.planes, self.ids = planes, ids
        if planes is not None:
            plane_sizes = [sizes[b] for b, ps in enumerate(planes) for _ in ps]
            off = maskpost.sized_tables(plane_sizes)[1]
            bits = torch.from_numpy(np.concatenate([pack(m) for ps in planes for m in ps])).to(dev)
            sized = maskpost.SizedMasks(bits=bits, offsets=torch.from_numpy(off).to(dev), area=None, box=None,
                                        status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=plane_sizes, level=1)
            p, layers = 0, []
            for ps in planes:
                layers.append([maskpost.fill(sized, p + k, color=COLORS[k % len(COLORS)], alpha=alpha) for k in range(len(ps))])
                p += len(ps)
            self.source = bits
        else:
            class Maps:
                pass
            maps = Maps()
            maps.sizes = [tuple(int(v) for v in s) for s in sizes]
            self.pal = maskpost.palette(19)
            flat = torch.from_numpy(np.concatenate([i.reshape(-1) for i in ids])).to(dev)
            layers = [[maskpost.classes(flat, maps, b, palette=self.pal, alpha=1.0, edges=True)] for b in range(len(photos))]
            self.source = flat
        req = maskpost.render_request(self.images.sizes, layers, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.tables = (up(req.layer_offsets), up(req.layers), up(req.rgb), up(req.alpha))
        self.max_pixels = maskpost.image_tables(self.images.sizes)[2]
        self.out = torch.empty_like(self.images.data)
        self.own = self.images.data.clone()
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.n_layers = req.L

    def launch(self, in_place: bool = False):
        layer_offsets, rows, rgb, alpha = self.tables
        src = self.own if in_place else self.images.data
        hip.render(src, self.images.offsets, self.images.dims, self.max_pixels, layer_offsets, rows,
                   self.source if self.planes is not None else None, None, self.source if self.planes is None else None, rgb, alpha,
                   src if in_place else self.out, self.status)

    def host(self, pool):
        """The host alternative: one read of the sources, then 16 threads -> the images."""
        src = self.source.cpu().numpy()
        if self.planes is not None:
            off = maskpost.sized_tables([self.photos[b].shape[:2] for b, ps in enumerate(self.planes) for _ in ps])[1]
            jobs, p = [], 0
            for b, ps in enumerate(self.planes):
                jobs.append((self.photos[b], [src[int(off[p + k]):int(off[p + k + 1])] for k in range(len(ps))], self.alpha))
                p += len(ps)
            return pool.map(host_fills, jobs)
        off = maskpost.label_tables([p.shape[:2] for p in self.photos])[1]
        return pool.map(host_edges, [(self.photos[b], src[int(off[b]):int(off[b + 1])].reshape(self.photos[b].shape[:2]), self.pal)
                                     for b in range(len(self.photos))])


def workloads(dev, only):
    rng = np.random.default_rng(31)
    want = lambda name: only is None or only in name
    if want("sweep 8 x 5"):
        sizes = [((480, 640), (427, 640))[i % 2] for i in range(8)]
        photos = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
        yield Workload("sweep 8 x 5", photos, dev, planes=[list(blobs(h, w, 5, rng)) for h, w in sizes])
    big = [n for n in ("64 x 1024^2, 1 fill", "64 x 1024^2, 8 fills", "64 x 1024^2, edges") if want(n)]
    if not big:
        return
    photos = [rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8) for _ in range(64)]
    base = blobs(1024, 1024, 8, rng)
    yy, xx = np.mgrid[:1024, :1024]
    blocks = (((yy // 97) * 11 + xx // 131) % 19).astype(np.int32)
    for name in big:
        if name.endswith("edges"):
            yield Workload(name, photos, dev, ids=[np.roll(blocks, 13 * b, axis=1) for b in range(64)], alpha=1.0)
        else:
            k = 1 if "1 fill" in name else 8
            yield Workload(name, photos, dev, planes=[[np.roll(base[i], 13 * b, axis=1) for i in range(k)] for b in range(64)])


def main() -> int:
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "render_bench.log"))
    args = ap.parse_args()
    hip.load()
    pool = None if args.kernels else ThreadPool(16)                   # the host alternative's threads start before the device is opened
    dev = torch.device("cuda:0")
    if not args.kernels:
        LOG = open(args.log, "w")
    say(f"# tools/bench_render.py --rounds {args.rounds} --warmup {args.warmup} --host-rounds {args.host_rounds}{' --kernels' if args.kernels else ''}"
        f"   {torch.cuda.get_device_name(0)}")
    ok = True
    for wl in workloads(dev, args.only):
        if args.kernels:
            for _ in range(args.repeat):
                wl.launch()
            torch.cuda.synchronize()
            say(f"{wl.name:22s} {args.repeat} calls of cvlm_render, status {int(wl.status.item())}")
            continue
        t = {}
        for key, fn in (("a", wl.launch), ("b", lambda: wl.launch(True)), ("c", lambda: wl.out.copy_(wl.images.data))):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t[key] = [event_ms(fn) for _ in range(args.rounds)]
        wl.launch()
        got, status = wl.out.cpu().numpy(), int(wl.status.item())
        t_host, host = [], None
        for _ in range(args.host_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = wl.host(pool)
            t_host.append((time.perf_counter() - t0) * 1e3)
        off = maskpost.image_tables(wl.images.sizes)[1]
        same = status == 0 and all(np.array_equal(got[int(off[b]):int(off[b]) + im.size].reshape(im.shape), im) for b, im in enumerate(host))
        ok &= bool(same)
        mib = wl.images.data.numel() / 2 ** 20
        ma, mb, mc = (statistics.median(t[k]) for k in "abc")
        say(f"{wl.name:22s} {len(wl.photos)} images, {mib:.1f} MiB of pixels, {wl.n_layers} layers, {wl.source.numel() * wl.source.element_size() / 2 ** 20:.1f} MiB of sources")
        say(f"{wl.name:22s} {'(a) cvlm_render into a second buffer, device events':72s} {med(t['a'])}   {2 * mib / 1024 / (ma / 1e3):.0f} GiB/s of pixels")
        say(f"{wl.name:22s} {'(b) cvlm_render in place, device events':72s} {med(t['b'])}")
        say(f"{wl.name:22s} {'(c) copy_ of the image buffer, device events':72s} {med(t['c'])}   {2 * mib / 1024 / (mc / 1e3):.0f} GiB/s")
        say(f"{wl.name:22s} {'(d) sources read back, numpy on 16 threads, wall clock':72s} {med(t_host)}")
        say(f"{wl.name:22s} bytes of (a) and (d) equal, status 0: {same};  (a) / (c) = {ma / mc:.2f}x, (b) / (c) = {mb / mc:.2f}x, "
            f"(d) / (a) = {statistics.median(t_host) / ma:.0f}x")
    if pool is not None:
        pool.close()
    say("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
