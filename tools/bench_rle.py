"""COCO run-length encoding of packed masks on a full class sweep: demo geometry, B = 8, every class of the bank on one
encoded batch -- `decode(enc, classes=all, masks="bits", min_area=64)` (a) as it is and (b) with rle="kept", one process.  First the
new field is held against the definition in numpy on a few of the call's own planes; then, after a warm-up, the two calls alternate,
each timed with device events around it and a synchronise after it.  Reported: (b) - (a) per plane and per sweep, its ratio to (a),
the runs and bytes of `counts` for rle="mask" and rle="kept" beside the bytes of the bits, and the peak memory of (b) over (a).  Then
the host alternative for the same planes: a device-to-host copy of kept_bits, numpy.unpackbits, the transpose and the run boundaries on
at most 16 threads.  Gated: the parity, the added device time below the host alternative, the peak within the results + RLE_WS_CAP.
--kernels: instead, cvlm_mask_rle_count and cvlm_mask_rle_emit on 64 planes of 1024^2 -- the reference's planes repeated, then full
planes -- `--repeat` calls each back to back (for `rocprofv3 --kernel-trace --stats -- python tools/bench_rle.py --kernels`), with the
event-timed means.
Usage: python tools/bench_rle.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
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
from camouflaged_vlm_amd.engine import RLE_WS_CAP, Cascade, Precision  # noqa: E402


def host_counts(row: np.ndarray, S: int) -> np.ndarray:
    """uint8 [S * S / 8] -> the plane's run counts by the definition: unpackbits, transpose, the positions that differ from their
    predecessor, their differences."""
    f = np.ascontiguousarray(np.unpackbits(row).reshape(S, S).T).reshape(-1).view(np.int8)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0)


def reference_planes(S: int) -> np.ndarray:
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        return z["mask_bits"].reshape(-1, S * S // 8)


def timed(fn, repeat: int) -> float:
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeat):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeat


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, P = spec.DEMO_SAM.inp_size, 64
    ref = torch.from_numpy(np.tile(reference_planes(S), (-(-P // 6), 1))[:P].copy()).to(dev)
    full = torch.full_like(ref, 0xFF)
    ws = torch.empty(hip.mask_rle_workspace_bytes(P, S, S), dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    for name, bits in (("the reference's planes repeated", ref), ("full planes", full)):
        n = torch.empty(P, dtype=torch.int32, device=dev)
        ms_count = timed(lambda: hip.mask_rle_count(bits, S, S, n), args.repeat)
        off = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(n, 0)
        counts = torch.empty(int(off[P]), dtype=torch.int32, device=dev)
        ms_emit = timed(lambda: hip.mask_rle_emit(bits, S, S, off, counts, status, ws), args.repeat)
        assert int(status) == 0
        print(f"{P} planes of {S} x {S}, {name}, {args.repeat} calls back to back: cvlm_mask_rle_count {ms_count * 1e3:.0f} us "
              f"({bits.numel() / ms_count / 1e6:.0f} GB/s over the {bits.numel() / 2**20:.0f} MiB of bits), cvlm_mask_rle_emit "
              f"{ms_emit * 1e3:.0f} us, {ms_emit * 1e3 / P:.2f} us per plane; {int(off[P])} counts = {int(off[P]) * 4 / 2**20:.1f} MiB, "
              f"n_runs {int(n.min())} .. {int(n.max())}; workspace {ws.numel() / 2**20:.0f} MiB", flush=True)
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
    base_kw = dict(masks="bits", min_area=64)
    modes = [("(a) masks=\"bits\", min_area=64", base_kw), ("(b) ... rle=\"kept\"", dict(base_kw, rle="kept"))]
    # parity before any timing: every other field as without rle, the counts as the definition gives them on a few planes
    plain = cas.decode(enc, classes=classes, **base_kw)
    full = cas.decode(enc, classes=classes, **modes[1][1])
    whole = cas.decode(enc, classes=classes, **dict(base_kw, rle="mask"))
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box", "kept_bits",
                                                                           "kept_area", "n_kept", "n_comp"))
    kept = full.kept_bits.view(P, -1).cpu().numpy()
    off, cnt = full.rle.offsets.cpu().numpy(), full.rle.counts.cpu().numpy()
    some = list(range(0, P, max(1, P // 8)))
    agree = all(np.array_equal(cnt[off[p]:off[p + 1]], host_counts(kept[p], S)) for p in some)
    full.rle.check()
    whole.rle.check()
    bits_bytes = full.mask_bits.numel()
    print(f"parity, {B} x {K} hypotheses: the other fields {'equal' if same else 'DIFFERENT'} to the call without rle; counts "
          f"{'equal' if agree else 'DIFFERENT'} to the definition on every {max(1, P // 8)}th plane", flush=True)
    for name, r in (("mask", whole.rle), ("kept", full.rle)):
        n = r.n_runs
        print(f"rle=\"{name}\": {r.counts.numel()} runs in all = {r.counts.numel() * 4 / 2**20:.1f} MiB of counts beside {bits_bytes / 2**20:.0f} MiB "
              f"of bits ({r.counts.numel() * 4 / bits_bytes:.2f} x); n_runs per plane {int(n.min())} .. {int(n.max())}, median "
              f"{int(n.float().median())}", flush=True)
    results = sum(-(-t.numel() * t.element_size() // 512) * 512 for t in (full.rle.counts, full.rle.offsets, full.rle.n_runs, full.rle.status))
    del plain, full, whole
    for _ in range(args.warmup):
        for _, kw in modes:
            cas.decode(enc, classes=classes, **kw)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    peaks = {name: 0 for name, _ in modes}
    for _ in range(args.rounds):
        for name, kw in modes:
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h = cas.decode(enc, classes=classes, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - start)
            bits_dev = h.kept_bits
            del h
    print(f"demo geometry, B = {B}, all {K} classes ({P} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / P:12.3f}", flush=True)
    base, with_r = (statistics.median(times[name]) for name, _ in modes)
    added = with_r - base
    print(f"rle=\"kept\" adds (b) - (a) = {added:+.2f} ms to the sweep, {added / P * 1e3:.1f} us per plane, {100 * added / base:.1f} % of (a)",
          flush=True)
    grow = peaks[modes[1][0]] - peaks[modes[0][0]]
    ws_bytes = cas.ws._flat[("u8", "cls_rle")].numel()
    fits = grow <= results + RLE_WS_CAP
    print(f"peak memory over the starting level: (a) {peaks[modes[0][0]] / 2**20:.1f} MiB, (b) {peaks[modes[1][0]] / 2**20:.1f} MiB: grows by "
          f"{grow / 2**20:.1f} MiB; the result tensors are {results / 2**20:.1f} MiB, the workspace \"cls_rle\" {ws_bytes / 2**20:.0f} MiB "
          f"(cap {RLE_WS_CAP / 2**20:.0f} MiB, allocated before the rounds): {'within' if fits else 'ABOVE'} results + cap", flush=True)
    # the host alternative for the same planes
    threads = min(16, os.cpu_count() or 1)
    t0 = time.perf_counter()
    host_bits = bits_dev.view(P, -1).cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_counts(host_bits[0], S)
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        runs = sum(len(c) for c in pool.map(lambda row: host_counts(row, S), host_bits))
    t_enc = time.perf_counter() - t0
    alt = (t_copy + t_enc) * 1e3
    print(f"host alternative for the same {P} planes: copy to the host {t_copy * 1e3:.1f} ms + unpackbits, transpose and run boundaries on "
          f"{threads} threads {t_enc * 1e3:.0f} ms ({t_one * 1e3:.1f} ms for the first plane; {runs} runs) = {alt:.0f} ms; the device adds "
          f"{added:+.2f} ms: {'below' if added < alt else 'NOT BELOW'} the host alternative", flush=True)
    return 0 if same and agree and fits and added < alt else 1


if __name__ == "__main__":
    sys.exit(main())
