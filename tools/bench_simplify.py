"""Simplified contour rings on the workloads of tools/bench_contours.py: `--workload sweep` -- demo geometry, B = 8,
every class of the bank on one encoded batch, the sweep's sized planes raw and its kept planes after min_area=64 -- and `--workload
planes` -- 64 planes of 1024 x 1024, the reference's planes repeated.  The contours come from Cascade.mask_contours_sized; then, at
0.5, 1 and 2 pixels, the polygons of a few planes are held against the sequential host entry and, after two calls that are not
timed, cvlm_contour_simplify_mark (all rounds), cvlm_contour_simplify_emit and the whole Cascade.simplify_contours call are timed with
device events, `--rounds` times each: medians and spread, the vertices and bytes in and out, the rounds of the deepest plane.  The host
alternative is timed beside them: one copy of the three tensors to the host and cvlm_debug_contour_simplify_host, one plane per task on
16 threads.  One workload per process, so that a caller gives each its own time limit.

Usage: python tools/bench_simplify.py --workload sweep|planes [--rounds N] [--batch B] [--precision mx|exact]"""
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
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench_contours as BC  # noqa: E402
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import RLE_WS_CAP, Cascade, MaskContours, Precision, SizedMasks, contour_rounds, simplify_request, sized_tables  # noqa: E402

TOLERANCES = (0.5, 1.0, 2.0)


class Entries:
    """The two entries on one MaskContours, as Cascade.simplify_contours calls them, with every tensor allocated once."""

    def __init__(self, mc: MaskContours, tolerance: float, cap: int = RLE_WS_CAP):
        dev = mc.xy.device
        self.mc, self.P, self.total = mc, len(mc.sizes), int(mc.xy.shape[0])
        self.T = torch.from_numpy(simplify_request(mc, tolerance=tolerance)).to(dev)
        need = lambda planes, vertices, _=0: hip.contour_simplify_workspace_bytes(planes, vertices)
        self.nv = mc.n_vertices.cpu().numpy()
        self.rounds = [(0, self.P, self.total, need(self.P, self.total))]
        if self.rounds[0][3] > cap and self.P > 1:
            self.rounds = contour_rounds(self.nv, 0, cap, need)
        i32 = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
        self.keep, self.n_kept, self.rings, self.status = i32(self.total, dtype=torch.uint8), i32(self.P), i32(self.P, 2), i32(1)
        self.ws = i32(max(r[3] for r in self.rounds), dtype=torch.uint8)
        self.deepest = 0
        for a, b, rv, nbytes in self.rounds:                          # once, round by round: the word behind the arrays of each call
            self.mark_round(a, b, rv, nbytes)
            self.deepest = max(self.deepest, int(self.ws[nbytes - 16:nbytes - 12].view(torch.int32).item()))
            assert int(self.status) == 0
        self.oo = torch.zeros(self.P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(self.n_kept, 0, dtype=torch.int64, out=self.oo[1:])
        self.total_out = int(self.oo[-1])
        self.xy, self.start = i32(self.total_out, 2, dtype=torch.int16), i32(self.total_out, dtype=torch.uint8)

    def mark_round(self, a, b, rv, nbytes):
        hip.contour_simplify_mark(self.mc.xy, self.mc.ring_start, self.mc.vertex_offsets[a:b + 1], self.T[a:b], rv, self.keep, self.n_kept[a:b],
                                  self.rings[a:b], self.status, self.ws[:nbytes])

    def mark(self):
        for r in self.rounds:
            self.mark_round(*r)

    def emit(self):
        hip.contour_simplify_emit(self.mc.xy, self.mc.ring_start, self.mc.vertex_offsets, self.keep, self.oo, self.xy, self.start, self.status)

    def describe(self) -> str:
        r, before = self.rings.cpu().numpy(), self.mc.n_rings.cpu().numpy()
        kept = self.n_kept.cpu().numpy()
        return (f"{self.total} vertices ({self.total * 5 / 2**20:.2f} MiB) -> {self.total_out} ({self.total_out * 5 / 2**20:.2f} MiB), out / in = "
                f"{self.total_out / max(self.total, 1):.4f}; per plane {int(kept.min())} .. {int(kept.max())}, median {int(np.median(kept))}; rings "
                f"{int(before.sum())} -> {int(r.sum())} ({int(before.sum() - r.sum())} dropped); {self.deepest} rounds in the deepest plane; "
                f"{len(self.rounds)} mark call(s), workspace {self.ws.numel() / 2**20:.1f} MiB")


def host_simplify(xy: np.ndarray, start: np.ndarray, vo: np.ndarray, T: np.ndarray, threads: int):
    """The sequential host entry, one plane per task -> ([(vertices, xy, ring_start)], seconds)."""
    def one(p):
        a, b = int(vo[p]), int(vo[p + 1])
        x, s = torch.from_numpy(xy[a:b].copy()), torch.from_numpy(start[a:b].copy())
        v, t = torch.tensor([0, b - a], dtype=torch.int64), torch.from_numpy(T[p:p + 1].copy())
        keep, n, r, st = torch.empty(b - a, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        hip.contour_simplify_sequential(x, s, v, t, keep, n, r, st)
        m = int(n[0])
        out, out_start = torch.empty(m, 2, dtype=torch.int16), torch.empty(m, dtype=torch.uint8)
        hip.contour_simplify_sequential(x, s, v, t, keep, n, r, st, torch.tensor([0, m], dtype=torch.int64), out, out_start)
        return m, out, out_start
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        res = list(pool.map(one, range(vo.size - 1)))
    return res, time.perf_counter() - t0


def measure(name: str, cas, sized: SizedMasks, args) -> bool:
    mc = cas.mask_contours_sized(sized)
    mc.check()
    print(f"{name}: {len(mc.sizes)} planes, {sized.bits.numel() / 2**20:.1f} MiB of bits, {mc.xy.shape[0]} contour vertices", flush=True)
    ok = True
    for tol in TOLERANCES:
        ent = Entries(mc, tol)
        ent.emit()
        torch.cuda.synchronize()
        assert int(ent.status) == 0
        print(f"  tolerance {tol} px: {ent.describe()}", flush=True)
        t_mark, t_emit = BC.events(ent.mark, args.rounds), BC.events(ent.emit, args.rounds)
        t_call = BC.events(lambda: cas.simplify_contours(mc, tolerance=tol), args.rounds)
        print(f"    cvlm_contour_simplify_mark {BC.spread(t_mark)}; cvlm_contour_simplify_emit {BC.spread(t_emit)}; Cascade.simplify_contours end to "
              f"end {BC.spread(t_call)}", flush=True)
        threads = min(16, os.cpu_count() or 1)
        t0 = time.perf_counter()
        xy, start, vo = mc.xy.cpu().numpy(), mc.ring_start.cpu().numpy(), mc.vertex_offsets.cpu().numpy()
        t_copy = time.perf_counter() - t0
        res, t_host = host_simplify(xy, start, vo, ent.T.cpu().numpy(), threads)
        oo, out, out_start = ent.oo.cpu().numpy(), ent.xy.cpu(), ent.start.cpu()
        some = list(range(0, ent.P, max(1, ent.P // 16)))
        agree = all(res[p][0] == oo[p + 1] - oo[p] and torch.equal(res[p][1], out[oo[p]:oo[p + 1]]) and torch.equal(res[p][2], out_start[oo[p]:oo[p + 1]])
                    for p in some)
        alt, dev_ms = (t_copy + t_host) * 1e3, statistics.median(t_call)
        print(f"    parity with the host entry on every {max(1, ent.P // 16)}th plane: {'equal' if agree else 'DIFFERENT'}; host alternative: copy "
              f"{t_copy * 1e3:.1f} ms + the sequential entry on {threads} threads {t_host * 1e3:.0f} ms = {alt:.0f} ms; the device call takes "
              f"{dev_ms:.2f} ms: host / device = {alt / dev_ms:.1f}", flush=True)
        ok = ok and agree
    return ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["sweep", "planes"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    args = ap.parse_args()
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    S = g.inp_size
    if args.workload == "planes":
        P = 64
        rows = np.tile(BC.reference_planes(S), (-(-P // 6), 1))[:P].copy()
        sizes = [(S, S)] * P
        _, off, _ = sized_tables(sizes)
        sized = SizedMasks(bits=torch.from_numpy(rows.reshape(-1)).to(dev), offsets=torch.from_numpy(off).to(dev), area=None, box=None,
                           status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=sizes, level=0)
        print(f"{P} planes of {S} x {S}, the reference's planes repeated, {args.rounds} timed calls each", flush=True)
        return 0 if measure("reference planes", cas, sized, args) else 1
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    B, K = args.batch, c.n_cls_test
    P = B * K
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    sizes = [(480, 640), (427, 640)] * (B // 2) + [(480, 640)] * (B % 2)
    for _ in range(2):
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
