"""Class vocabularies at run time: what they cost.  Demo geometry, precision mx, B = 8, one process; after a warm-up
the calls of a part alternate, each timed with device events around it and a synchronise after it; medians with their spread.
  (a) ClipModel.make_vocabulary at n = 61, 1203 and 4817 prompts (token ids + the embedding table, EOT columns drawn in 6..20)
  (c) infer_classes(topk=5) on the 4817-class vocabulary against the constructor's 61-class bank (the difference: the head and
      top-k launches)
--kernels: only the head kernels, no model -- cvlm_clip_head_wide (its combine pass included) against cvlm_clip_head at C = 1024
  for P = 8 and 40, and alone at C = 4817; text matrix bytes / time.  Held: at C = 1024, P = 40 the wide entry's median may exceed
  cvlm_clip_head's by no more than that entry's own spread (max - min).  Run it under `rocprofv3 --kernel-trace --stats` for the
  per-kernel split.
Usage: python tools/bench_vocab.py [--kernels] [--rounds N] [--warmup W] [--batch B] [--precision mx|exact]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402


def timed(calls, rounds, warmup):
    for _ in range(warmup):
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
    return times


def report(times, unit="ms"):
    print(f"{'call':44s} {'median ' + unit:>11s} {'min':>9s} {'max':>9s}")
    for name, t in times.items():
        print(f"{name:44s} {statistics.median(t):11.3f} {min(t):9.3f} {max(t):9.3f}", flush=True)


REP = 20                    # launches per timed call of --kernels: a single launch is shorter than the events' own overhead


def kernels(args) -> int:
    dev, D = torch.device("cuda:0"), 768
    gen = torch.Generator().manual_seed(0)
    calls, nbytes = [], {}
    for P, Cc, both in ((8, 1024, True), (40, 1024, True), (8, 4817, False), (40, 4817, False)):
        img, txt = torch.randn(P, D, generator=gen).to(dev), torch.randn(Cc, D, generator=gen).to(dev)
        img_n, logits = torch.empty(P, D, device=dev), torch.empty(P, Cc, device=dev)
        pred, sel = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, D, device=dev)
        ws = torch.empty(hip.clip_head_wide_workspace_bytes(P, Cc), dtype=torch.uint8, device=dev)
        if both:
            name = f"cvlm_clip_head      P = {P:2d} C = {Cc}"
            calls.append((name, lambda a=(img, txt, 100.0, P, Cc, D, img_n, logits, pred, sel): [hip.clip_head(*a) for _ in range(REP)]))
            nbytes[name] = Cc * D * 4
        name = f"cvlm_clip_head_wide P = {P:2d} C = {Cc}"
        calls.append((name, lambda a=(img, txt, 100.0, P, Cc, D, img_n, logits, pred, sel, ws): [hip.clip_head_wide(*a) for _ in range(REP)]))
        nbytes[name] = Cc * D * 4
    times = {name: [x / REP for x in t] for name, t in timed(calls, args.rounds, args.warmup).items()}
    print(f"per launch of the entry, {REP} back-to-back launches per timed call")
    report(times)
    for name, t in times.items():
        print(f"{name}: text matrix {nbytes[name] / 1e6:.1f} MB / median = {nbytes[name] / (statistics.median(t) * 1e-3) / 1e9:.1f} GB/s")
    th, tw = times["cvlm_clip_head      P = 40 C = 1024"], times["cvlm_clip_head_wide P = 40 C = 1024"]
    ok = statistics.median(tw) <= statistics.median(th) + (max(th) - min(th))
    print(f"C = 1024, P = 40: wide {statistics.median(tw):.3f} ms vs cvlm_clip_head {statistics.median(th):.3f} ms "
          f"(spread {max(th) - min(th):.3f} ms): {'not slower' if ok else 'SLOWER'}")
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    del sd
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    table = torch.from_numpy(synth.make_tensor("openai.token_embedding.weight", (49408, c.text_width), "embed", 0)).to(dev)
    rng = np.random.default_rng(5)

    def request(n):
        tok = rng.integers(1, 49407, size=(n, c.context_length)).astype(np.int32)
        return dict(tokens=tok, table=table, eot=rng.integers(6, 21, size=n), bank=torch.from_numpy(synth.make_text_bank(n, c.embed_dim, "test")))
    reqs = {n: request(n) for n in (61, 1203, 4817)}
    # (a)
    times = timed([(f"(a) make_vocabulary n = {n}", lambda r=r: cas.make_vocabulary(**r)) for n, r in reqs.items()],
                  max(3, args.rounds // 3), 1)
    print(f"demo geometry, B = {args.batch}, precision {args.precision}")
    report(times)
    # (c)
    v = cas.make_vocabulary(**reqs[4817], name="4817 synthetic prompts")
    times = timed([("(c) infer_classes(topk=5), 61-class bank", lambda: cas.infer_classes(inp, ci, cm, topk=5)),
                   ("(c) infer_classes(topk=5, vocab=4817 classes)", lambda: cas.infer_classes(inp, ci, cm, topk=5, vocab=v))],
                  args.rounds, args.warmup)
    report(times)
    a, b = (statistics.median(t) for t in times.values())
    print(f"(c) vocabulary - bank = {b - a:+.3f} ms per batch; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
