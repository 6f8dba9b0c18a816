"""Packed masks against f32 planes on a full class sweep: demo geometry, B = 8, every class of the bank on one
encoded batch -- `decode(enc, classes=all)` with masks="logits" against masks="bits", overlaps=True, one process.  First the parity of
the two modes (classes, stage-2 logits and predictions bit for bit; mask_bits = packbits(masks > 0) of the default call's planes,
checked on the device); then, after a warm-up, the two calls alternate, each timed with device events around it and a synchronise
after it, and each mode's peak allocated memory over its starting level is read after torch.cuda.reset_peak_memory_stats().  The
bits mode is held against the default: its median may exceed the default's by no more than the default's own spread (max - min).
--kernels: instead, cvlm_mask_pack on 64 planes and cvlm_mask_overlap on B x n_cls planes, `--repeat` launches each back to back
(for `rocprofv3 --kernel-trace --stats -- python tools/bench_compact.py --kernels`), with the event-timed mean and the bytes per
second each launch moves.
Usage: python tools/bench_compact.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402


def kernels(args) -> int:
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    S, P, n, K = g.inp_size, 64, args.batch, c.n_cls_test
    gen = torch.Generator(device=dev).manual_seed(1)
    planes = torch.randn(P, S, S, device=dev, generator=gen)
    bits = torch.empty(P, S * S // 8, dtype=torch.uint8, device=dev)
    area = torch.empty(P, dtype=torch.int32, device=dev)
    box = torch.empty(P, 4, dtype=torch.int32, device=dev)
    many = torch.randint(0, 256, (n, K, S * S // 8), dtype=torch.uint8, device=dev, generator=gen)
    inter = torch.empty(n, K, K, dtype=torch.int32, device=dev)
    runs = [("cvlm_mask_pack", lambda: hip.mask_pack(planes, bits, area, box), planes.numel() * 4 + bits.numel(),
             f"{P} planes of {S} x {S}"),
            ("cvlm_mask_overlap", lambda: hip.mask_overlap(many, inter), many.numel(), f"{n} x {K} planes of {S * S // 32} words")]
    for name, fn, nbytes, what in runs:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeat):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.repeat
        print(f"{name}: {what}, {args.repeat} launches back to back: {ms * 1e3:.1f} us each, {nbytes / 2**20:.1f} MiB compulsory "
              f"traffic, {nbytes / ms / 1e6:.0f} GB/s", flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    del sd
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    B, K, S = args.batch, c.n_cls_test, g.inp_size
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    modes = [("masks=\"logits\"", dict()), ("masks=\"bits\", overlaps=True", dict(masks="bits", overlaps=True))]
    # parity of the two modes before any timing
    full = cas.decode(enc, classes=classes)
    compact = cas.decode(enc, classes=classes, **modes[1][1])
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(full, f), getattr(compact, f)) for f in ("classes", "logits", "pred"))
    check = torch.empty_like(compact.mask_bits).view(B * K, -1)
    for p0 in range(0, B * K, 64):
        hip.mask_pack(full.masks.view(B * K, S, S)[p0:p0 + 64], check[p0:p0 + 64])
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(check.view_as(compact.mask_bits), compact.mask_bits))
    diag = bool(torch.equal(torch.diagonal(compact.inter, dim1=1, dim2=2), compact.area))
    print(f"parity of masks=\"bits\" with the default call, {B} x {K} hypotheses: classes / stage-2 logits / predictions "
          f"{'equal' if same else 'DIFFERENT'}; mask_bits {'equal' if same_bits else 'DIFFERENT'} to the packed default planes; "
          f"diagonal of inter {'equal' if diag else 'DIFFERENT'} to area; areas {int(compact.area.min())} .. {int(compact.area.max())}",
          flush=True)
    del full, compact, check
    for _ in range(args.warmup):
        for _, kw in modes:
            cas.decode(enc, classes=classes, **kw)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    peak = {name: 0 for name, _ in modes}
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
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - start)
            del h
    ta, tb = times[modes[0][0]], times[modes[1][0]]
    base, spread = statistics.median(ta), max(ta) - min(ta)
    print(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    print(f"{'decode(enc, classes=all, ...)':34s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s} {'peak over start':>16s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:34s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / (B * K):12.3f} "
              f"{peak[name] / 2**20:12.1f} MiB", flush=True)
    ok = statistics.median(tb) <= base + spread
    print(f"bits - logits = {statistics.median(tb) - base:+.2f} ms against the default's spread of {spread:.2f} ms: "
          f"{'not slower' if ok else 'SLOWER'}", flush=True)
    return 0 if ok and same and same_bits and diag else 1


if __name__ == "__main__":
    sys.exit(main())
