"""K class hypotheses per image against the cascade: demo geometry, B = 8, one process.  After a warm-up, `cascade(pipelined=False)` and
`infer_classes(topk=K)` for K = 1, 3, 5 alternate, each call timed with device events around it and a synchronise after it; the median of
the rounds is printed per call, with its ratio to the cascade and, for comparison, K separate cascades (K x the cascade's time).
Usage: python tools/bench_classes.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--ks 1,3,5]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--ks", default="1,3,5")
    args = ap.parse_args()
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    del sd
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    ks = [int(k) for k in args.ks.split(",")]
    calls = [("cascade", 1, lambda: cas.cascade(inp, ci, cm))] + \
            [(f"infer_classes K={k}", k, lambda k=k: cas.infer_classes(inp, ci, cm, topk=k)) for k in ks]
    for _ in range(args.warmup):
        for _, _, fn in calls:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in calls}
    for _ in range(args.rounds):
        for name, _, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    base = statistics.median(times["cascade"])
    print(f"demo geometry, B = {args.batch}, precision {args.precision}, {args.rounds} alternating rounds after {args.warmup} warm-up; "
          f"class chunk {cas.class_chunk()} prompts; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    print(f"{'call':22s} {'ms / batch':>11s} {'min':>8s} {'max':>8s} {'x cascade':>10s} {'K cascades':>11s}")
    for name, k, _ in calls:
        t = times[name]
        print(f"{name:22s} {statistics.median(t):11.2f} {min(t):8.2f} {max(t):8.2f} {statistics.median(t) / base:10.3f} {k * base:11.2f}",
              flush=True)


if __name__ == "__main__":
    main()
