"""Encode once, decode many times against `infer_classes`: demo geometry, B = 8, one process.  First the parity of the two routes
(`decode(encode(x), topk=5)` against `infer_classes(x, topk=5)`, held to the batch tolerance of the GEMM K-splits); then, after a
warm-up, the calls below alternate, each timed with device events around it and a synchronise after it; the median of the rounds is
printed per call with its spread and its fraction of (a):
  (a) infer_classes(topk=5)               (b) encode + decode(topk=5)
  (c) decode alone on one encoded batch, K = 1 and 5, stage 2 on and off
(b) is held against (a): its median may exceed (a)'s by no more than (a)'s own spread (max - min) over the rounds.
Usage: python tools/bench_session.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402

BATCH_TOL = 6e-5            # a batch against other GEMM row counts with the K-splits on (tests/test_classes_gpu.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
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
    # parity of the two routes before any timing
    want = cas.infer_classes(inp, ci, cm, topk=5)
    want = {f: getattr(want, f).clone() for f in ("classes", "pass1_logits", "masks", "edges", "logits", "pred")}
    enc = cas.encode(inp, ci, cm)
    got = cas.decode(enc, topk=5)
    torch.cuda.synchronize()
    diff = {f: float((getattr(got, f).double() - want[f].double()).abs().max()) for f in ("pass1_logits", "masks", "edges", "logits")}
    worst = max(diff.values())
    same_int = bool(torch.equal(got.classes, want["classes"])) and bool(torch.equal(got.pred, want["pred"]))
    print(f"parity decode(encode(x), topk=5) vs infer_classes(x, topk=5): " + ", ".join(f"{k} {v:.2e}" for k, v in diff.items()) +
          f"; classes and predictions {'equal' if same_int else 'DIFFERENT'}; batch tolerance {BATCH_TOL:.0e}: "
          f"{'within' if worst <= BATCH_TOL and same_int else 'EXCEEDED'}", flush=True)
    del got, want
    calls = [("(a) infer_classes K=5", lambda: cas.infer_classes(inp, ci, cm, topk=5)),
             ("(b) encode + decode K=5", lambda: cas.decode(cas.encode(inp, ci, cm), topk=5)),
             ("(c) decode K=1", lambda: cas.decode(enc, topk=1)),
             ("(c) decode K=1 no stage 2", lambda: cas.decode(enc, topk=1, stage2=False)),
             ("(c) decode K=5", lambda: cas.decode(enc, topk=5)),
             ("(c) decode K=5 no stage 2", lambda: cas.decode(enc, topk=5, stage2=False)),
             ("    encode", lambda: cas.encode(inp, ci, cm))]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    ta = times[calls[0][0]]
    base, spread = statistics.median(ta), max(ta) - min(ta)
    print(f"demo geometry, B = {args.batch}, precision {args.precision}, {args.rounds} alternating rounds after {args.warmup} warm-up; "
          f"class chunk {cas.class_chunk()} prompts; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    print(f"{'call':28s} {'ms / batch':>11s} {'min':>8s} {'max':>8s} {'of (a)':>8s}")
    for name, _ in calls:
        t = times[name]
        print(f"{name:28s} {statistics.median(t):11.2f} {min(t):8.2f} {max(t):8.2f} {statistics.median(t) / base:8.3f}", flush=True)
    tb = statistics.median(times[calls[1][0]])
    ok = tb <= base + spread
    print(f"(b) - (a) = {tb - base:+.2f} ms against (a)'s spread of {spread:.2f} ms: {'not slower' if ok else 'SLOWER'}", flush=True)
    return 0 if ok and worst <= BATCH_TOL and same_int else 1


if __name__ == "__main__":
    sys.exit(main())
