"""Contours of sized planes on a full class sweep: demo geometry, B = 8, every class of the bank on one encoded batch --
`decode(enc, classes=all, masks="bits", sizes=..., min_area=64)` gives the sweep's sized planes (raw) and its kept planes (after
min_area=64, wrapped as sized planes of the model's own size).  First the contours of a few planes are held against the sequential
host entry; then, after a warm-up, cvlm_mask_contour_count, cvlm_mask_contour_emit (all rounds) and the whole
Cascade.mask_contours_sized call are timed with device events, `--rounds` times each, medians and spread reported with the vertices,
rings, rounds and bytes out.  Then the host alternative for the same planes: the device-to-host copy of the bits and the sequential
host entry, one plane per task on at most 16 threads (the entry runs outside the interpreter lock).  Gated: the parity and the device
call below the host alternative.
--kernels: instead, the two entries on 64 planes of 1024^2 -- the reference's planes repeated, then speckle at density 0.5 on 1 plane in
8 -- `--repeat` calls each back to back (for `rocprofv3 --kernel-trace --stats -- python tools/bench_contours.py --kernels`, which
gives the split by pass), with the event-timed means.
Usage: python tools/bench_contours.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
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
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import RLE_WS_CAP, Cascade, Precision, SizedMasks, contour_rounds, sized_tables  # noqa: E402


def reference_planes(S: int) -> np.ndarray:
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        return z["mask_bits"].reshape(-1, S * S // 8)


def events(fn, repeat: int) -> list:
    """Milliseconds of each of `repeat` calls of fn, by device events, after two calls that are not timed."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def spread(t: list) -> str:
    return f"median {statistics.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f})"


class Entries:
    """The two entries on one SizedMasks, as Cascade.mask_contours_sized calls them, with every tensor allocated once."""

    def __init__(self, sized: SizedMasks, connectivity: int = 8, cap: int = RLE_WS_CAP):
        dev = sized.bits.device
        self.sized, self.c = sized, connectivity
        dims, _, self.max_words = sized_tables(sized.sizes)
        self.P = len(sized.sizes)
        self.dims = torch.from_numpy(dims).to(dev)
        self.n = torch.empty(self.P, dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.count()
        nv = self.n.cpu().numpy()
        self.vo = torch.zeros(self.P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(self.n, 0, dtype=torch.int64, out=self.vo[1:])
        self.total = int(nv.astype(np.int64).sum())
        self.rounds = contour_rounds(nv, self.max_words, cap, hip.mask_contour_workspace_bytes)
        self.xy = torch.empty(self.total, 2, dtype=torch.int16, device=dev)
        self.start = torch.empty(self.total, dtype=torch.uint8, device=dev)
        self.rings = torch.empty(self.P, 2, dtype=torch.int32, device=dev)
        self.ws = torch.empty(max(r[3] for r in self.rounds), dtype=torch.uint8, device=dev)
        self.nv = nv

    def count(self):
        hip.mask_contour_count(self.sized.bits, self.sized.offsets, self.dims, self.c, self.max_words, self.n, self.status)

    def emit(self):
        for a, b, rv, need in self.rounds:
            hip.mask_contour_emit(self.sized.bits, self.sized.offsets[a:b + 1], self.dims[a:b], self.c, self.max_words, self.vo[a:b + 1], rv,
                                  self.xy, self.start, self.rings[a:b], self.status, self.ws[:need])

    def describe(self) -> str:
        r = self.rings.cpu().numpy()
        out = self.total * 5 + self.P * 12
        return (f"{self.P} planes, {self.sized.bits.numel() / 2**20:.1f} MiB of bits -> {self.total} vertices (per plane {int(self.nv.min())} .. "
                f"{int(self.nv.max())}, median {int(np.median(self.nv))}), {int(r[:, 0].sum())} outer rings + {int(r[:, 1].sum())} holes, "
                f"{out / 2**20:.2f} MiB out; {len(self.rounds)} round(s), workspace {self.ws.numel() / 2**20:.1f} MiB")


def host_contours(bits: np.ndarray, off: np.ndarray, sizes, connectivity: int, threads: int):
    """The sequential host entry, one plane per task -> (vertices, seconds)."""
    def one(p):
        h, w = sizes[p]
        plane = torch.from_numpy(bits[off[p]:off[p + 1]].copy())
        o = torch.tensor([0, plane.numel()], dtype=torch.int64)
        d = torch.tensor([[h, w]], dtype=torch.int32)
        n, st = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        hip.mask_contour_host(plane, o, d, connectivity, n, st)
        total = int(n[0])
        vo = torch.tensor([0, total], dtype=torch.int64)
        xy, start = torch.empty(total, 2, dtype=torch.int16), torch.empty(total, dtype=torch.uint8)
        hip.mask_contour_host(plane, o, d, connectivity, n, st, vo, xy, start, torch.zeros(1, 2, dtype=torch.int32))
        return total, xy, start
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        res = list(pool.map(one, range(len(sizes))))
    return res, time.perf_counter() - t0


def measure(name: str, cas, sized: SizedMasks, args) -> bool:
    ent = Entries(sized)
    ent.emit()
    torch.cuda.synchronize()
    assert int(ent.status) == 0
    print(f"{name}: {ent.describe()}", flush=True)
    t_count, t_emit = events(ent.count, args.rounds), events(ent.emit, args.rounds)
    t_call = events(lambda: cas.mask_contours_sized(sized), args.rounds)
    print(f"  cvlm_mask_contour_count {spread(t_count)}; cvlm_mask_contour_emit {spread(t_emit)}, {statistics.median(t_emit) * 1e3 / ent.P:.1f} us "
          f"per plane; Cascade.mask_contours_sized end to end {spread(t_call)}", flush=True)
    threads = min(16, os.cpu_count() or 1)
    t0 = time.perf_counter()
    bits, off = sized.bits.cpu().numpy(), sized.offsets.cpu().numpy()
    t_copy = time.perf_counter() - t0
    res, t_host = host_contours(bits, off, sized.sizes, 8, threads)
    vo = ent.vo.cpu().numpy()
    some = list(range(0, ent.P, max(1, ent.P // 16)))
    xy, start = ent.xy.cpu(), ent.start.cpu()
    agree = all(res[p][0] == ent.nv[p] and torch.equal(res[p][1], xy[vo[p]:vo[p + 1]]) and torch.equal(res[p][2], start[vo[p]:vo[p + 1]])
                for p in some)
    alt, dev_ms = (t_copy + t_host) * 1e3, statistics.median(t_call)
    print(f"  parity with the host entry on every {max(1, ent.P // 16)}th plane: {'equal' if agree else 'DIFFERENT'}; host alternative: copy "
          f"{t_copy * 1e3:.1f} ms + the sequential entry on {threads} threads {t_host * 1e3:.0f} ms = {alt:.0f} ms; the device call takes "
          f"{dev_ms:.2f} ms: {'below' if dev_ms < alt else 'NOT BELOW'} the host alternative", flush=True)
    return agree and dev_ms < alt


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, P = spec.DEMO_SAM.inp_size, 64
    ref = np.tile(reference_planes(S), (-(-P // 6), 1))[:P].copy()
    rng = np.random.default_rng(26)
    speckled = ref.copy()
    speckled[::8] = np.packbits(rng.random((P // 8, S * S)) < 0.5, axis=1)
    for name, rows in (("the reference's planes repeated", ref), ("speckle at 0.5 on 1 plane in 8", speckled)):
        sizes = [(S, S)] * P
        _, off, _ = sized_tables(sizes)
        sized = SizedMasks(bits=torch.from_numpy(rows.reshape(-1)).to(dev), offsets=torch.from_numpy(off).to(dev), area=None, box=None,
                           status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=sizes, level=0)
        ent = Entries(sized)
        t_count, t_emit = events(ent.count, args.repeat), events(ent.emit, args.repeat)
        torch.cuda.synchronize()
        assert int(ent.status) == 0
        print(f"{P} planes of {S} x {S}, {name}: {ent.describe()}\n  cvlm_mask_contour_count {spread(t_count)} "
              f"({sized.bits.numel() / statistics.median(t_count) / 1e6:.0f} GB/s over the bits); cvlm_mask_contour_emit {spread(t_emit)}", flush=True)
    return 0


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
    B, K, S = args.batch, c.n_cls_test, g.inp_size
    P = B * K
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    sizes = [(480, 640), (427, 640)] * (B // 2) + [(480, 640)] * (B % 2)
    for _ in range(1 + args.warmup):
        h = cas.decode(enc, classes=classes, masks="bits", sizes=sizes, min_area=64)
    torch.cuda.synchronize()
    print(f"demo geometry, B = {B}, all {K} classes ({P} planes), precision {args.precision}, {args.rounds} timed calls each", flush=True)
    kept_sizes = [(S, S)] * P
    _, off, _ = sized_tables(kept_sizes)
    kept = SizedMasks(bits=h.kept_bits.reshape(-1), offsets=torch.from_numpy(off).to(dev), area=None, box=None,
                      status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=kept_sizes, level=0)
    ok = measure("raw sized planes", cas, h.sized, args)
    ok = measure("kept planes (min_area=64) at the model's size", cas, kept, args) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
