"""Multimask output against the one-mask step: demo geometry, B = 8, one process.  After a warm-up, `infer_test` and
`infer_test_multimask` (masks 1..3, and all four) alternate, each call timed with device events around it and a synchronise after it;
the median of the rounds is printed per call with its ratio to `infer_test`.
--kernels: no model -- P prompts' buffers at the demo geometry, then `--rounds` launches each of cvlm_mask_head_edge and of
cvlm_mask_head_multi (n_masks = 4, with the edge map) on the same buffers, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_multimask.py --kernels
Usage: python tools/bench_multimask.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels [--prompts P]]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402


def kernels(P: int, rounds: int) -> None:
    g = spec.DEMO_SAM
    dev = torch.device("cuda:0")
    HW, Cc = 16 * g.grid * g.grid, g.prompt_embed_dim // 8
    gen = torch.Generator(device=dev).manual_seed(0)
    up, emb = (torch.randn(P, HW, Cc, device=dev, generator=gen) for _ in range(2))
    hyper = torch.randn(P, 5, Cc, device=dev, generator=gen) * 0.3
    low1, edge1, low4, edge4 = (torch.empty(P, n, HW, device=dev) for n in (1, 1, 4, 1))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for warm in (True, False):
        ev[0].record()
        for _ in range(1 if warm else rounds):
            hip.mask_head_edge(up, emb, hyper, P, HW, Cc, low1, edge1)
        ev[1].record()
        for _ in range(1 if warm else rounds):
            hip.mask_head_multi(up, emb, hyper, P, HW, Cc, 4, low4, edge4)
        ev[2].record()
        torch.cuda.synchronize()
    same = torch.equal(low4[:, 0], low1[:, 0]) and torch.equal(edge4, edge1)
    t1, t4 = ev[0].elapsed_time(ev[1]) * 1e3 / rounds, ev[1].elapsed_time(ev[2]) * 1e3 / rounds
    b1, b4 = (2 * Cc + 2) * 4 * P * HW, (2 * Cc + 5) * 4 * P * HW
    print(f"P = {P}, HW = {HW}, C = {Cc}, {rounds} launches each, device events (a kernel trace gives the per-kernel times)")
    print(f"cvlm_mask_head_edge           {t1:8.1f} us  {b1 / 1e6:6.0f} MB  {b1 / t1 / 1e6:5.2f} TB/s")
    print(f"cvlm_mask_head_multi n = 4    {t4:8.1f} us  {b4 / 1e6:6.0f} MB  {b4 / t4 / 1e6:5.2f} TB/s   {t4 / t1:.3f} x the time, "
          f"{b4 / b1:.3f} x the bytes; plane 0 and edge map bit-equal: {same}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--prompts", type=int, default=40)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.prompts, args.rounds or 20)
    rounds = args.rounds or 10
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    del sd
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    calls = [("infer_test", lambda: cas.infer_test(inp, ci, cm)),
             ("multimask (masks 1..3)", lambda: cas.infer_test_multimask(inp, ci, cm)),
             ("multimask (all four)", lambda: cas.infer_test_multimask(inp, ci, cm, all_masks=True)),
             ("multimask (mask 0)", lambda: cas.infer_test_multimask(inp, ci, cm, multimask_output=False))]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(rounds):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    base = statistics.median(times["infer_test"])
    print(f"demo geometry, B = {args.batch}, precision {args.precision}, {rounds} alternating rounds after {args.warmup} warm-up", flush=True)
    print(f"{'call':24s} {'ms / batch':>11s} {'min':>8s} {'max':>8s} {'x infer_test':>13s}")
    for name, _ in calls:
        t = times[name]
        print(f"{name:24s} {statistics.median(t):11.2f} {min(t):8.2f} {max(t):8.2f} {statistics.median(t) / base:13.3f}", flush=True)


if __name__ == "__main__":
    main()
