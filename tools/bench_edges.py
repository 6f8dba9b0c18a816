"""Packed edge maps on a full class sweep: demo geometry, B = 8, every class of the bank on one encoded batch --
`decode(enc, classes=all, masks="bits", band=2, overlaps=True)` (a) as it is, (b) with edge_threshold=0.5 and (c) the alternative the
engine offered before: masks="both", then `edges > t` and a pack of the booleans on the device.  First the new fields are held against
the call without them and against (c)'s bits; then, after a warm-up, the three calls alternate, each timed with device events around it
and a synchronise after it, and the peak of device memory over the starting level is read for each.  Reported: (b) - (a) against
(c) - (a); the first must lie below the second.
--parity: instead, `infer_classes(..., masks="both", edge_threshold=t)` on the two images and three classes of
tests/golden/demo_classes_digest.npz: edge_bits at `sample_idx` against the reference's `edge_samples > t` at t = 0.5 and 0.9.  A
position may differ only where |edge_sample - t| is within the deviation of the engine's own edge map from the reference's samples,
measured in the same run.
--kernels: instead, cvlm_edge_pack on 64 planes 256^2 -> 1024^2 against cvlm_bilinear alone on the same planes, `--repeat` launches
each back to back (for `rocprofv3 --kernel-trace --stats -- python tools/bench_edges.py --kernels`), with the event-timed mean and the
implied bytes per second over what each reads and writes.
Usage: python tools/bench_edges.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--parity] [--kernels] [--repeat R]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402

RADIUS, T = 2, 0.5


def pack_bool(planes: torch.Tensor) -> torch.Tensor:
    """bool (..., n) -> uint8 (..., n / 8) in numpy.packbits' order, on the device."""
    w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=planes.device)
    return (planes.view(*planes.shape[:-1], -1, 8).to(torch.uint8) * w).sum(-1, dtype=torch.uint8)


def held(nbytes: int) -> int:
    """What torch's caching allocator holds for a tensor of nbytes: 512-byte blocks; from 10 MiB on a segment of whole 2 MiB, kept
    whole when no more than 1 MiB of it is left over."""
    block = -(-nbytes // 512) * 512
    segment = -(-nbytes // 2 ** 21) * 2 ** 21
    return segment if nbytes >= 10 * 2 ** 20 and segment - block <= 2 ** 20 else block


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    P, L, S = 64, 256, 1024
    yy, xx = np.mgrid[0:L, 0:L].astype(np.float32)
    rng = np.random.default_rng(0)
    prob = np.stack([0.5 + 0.45 * np.sin(rng.uniform(0.02, 0.3) * yy) * np.cos(rng.uniform(0.02, 0.3) * xx) for _ in range(P)]).astype(np.float32)
    prob = torch.from_numpy(prob).to(dev)
    bits = torch.empty(P, S * S // 8, dtype=torch.uint8, device=dev)
    band = torch.randint(0, 256, bits.shape, dtype=torch.uint8, device=dev)
    area = torch.empty(P, dtype=torch.int32, device=dev)
    inter = torch.empty(P, dtype=torch.int32, device=dev)
    full = torch.empty(P, S, S, device=dev)
    runs = [("cvlm_edge_pack, area only", lambda: hip.edge_pack(prob, S, S, T, bits, area), prob.numel() * 4 + bits.numel()),
            ("cvlm_edge_pack with a band", lambda: hip.edge_pack(prob, S, S, T, bits, area, band, inter), prob.numel() * 4 + 2 * bits.numel()),
            ("cvlm_bilinear alone", lambda: hip.bilinear(prob, P, L, L, full, S, S), prob.numel() * 4 + full.numel() * 4)]
    ms = {}
    for name, fn, moved in runs:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeat):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name] = e0.elapsed_time(e1) / args.repeat
        print(f"{name}: {P} planes {L} x {L} -> {S} x {S}, {args.repeat} calls back to back: {ms[name] * 1e3:.0f} us each, "
              f"{ms[name] * 1e3 / P:.2f} us per plane, {moved / ms[name] / 1e6:.0f} GB/s over the {moved / 2**20:.0f} MiB read and written", flush=True)
    same = torch.equal(pack_bool((full > T).view(P, -1)), bits)
    frac = area.float() / (S * S)
    faster = ms["cvlm_edge_pack with a band"] < ms["cvlm_bilinear alone"]
    print(f"edge_bits {'equal' if same else 'differ from'} cvlm_bilinear > {T} on these planes (they may differ within 2^-21 of the threshold); "
          f"set {100 * float(frac.min()):.0f} .. {100 * float(frac.max()):.0f} % of a plane; cvlm_edge_pack is "
          f"{ms['cvlm_bilinear alone'] / ms['cvlm_edge_pack with a band']:.1f} x as fast as cvlm_bilinear: {'faster' if faster else 'NOT FASTER'}", flush=True)
    return 0 if faster else 1


def engine(args):
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    return g, c, dev, cas


def parity(args) -> int:
    g, c, dev, cas = engine(args)
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        gold = {k: z[k] for k in z.files}
    with np.load(os.path.join(REPO, "tests", "golden", "ovcamo_constants.npz")) as z:
        bank = torch.from_numpy(z["bank_test"]).float()
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), bank, "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))
    idx, ref = gold["sample_idx"], gold["edge_samples"]
    ok = True
    for t in (0.5, 0.9):
        h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(gold["classes"]), masks="both", edge_threshold=t)
        torch.cuda.synchronize()
        B, K = ref.shape[:2]
        mine = h.edges.view(B, K, -1)[:, :, torch.from_numpy(idx).to(dev)].cpu().numpy()
        dev_max = float(np.abs(mine - ref).max())
        got = np.unpackbits(h.edge_bits.cpu().numpy(), axis=-1)[:, :, idx].astype(bool)
        differ = got != (ref > np.float32(t))
        excused = np.abs(ref - np.float32(t)) <= dev_max
        inside = not (differ & ~excused).any()
        ok = ok and inside
        print(f"demo {args.precision}, t = {t}: edge map deviates from the reference's samples by at most {dev_max:.3g}; of {ref.size} sampled "
              f"positions {int(differ.sum())} differ from edge_samples > t, {int(excused.sum())} lie within that deviation of t: "
              f"{'every difference inside it' if inside else 'A DIFFERENCE OUTSIDE IT'}; set {100 * float(got.mean()):.1f} % "
              f"(reference {100 * float((ref > np.float32(t)).mean()):.1f} %)", flush=True)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    if args.parity:
        return parity(args)
    g, c, dev, cas = engine(args)
    consts = host.ovcamo_constants()
    eot = host.eot_for_classes(consts["names_test"].tolist())[:c.n_cls_test]
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), torch.from_numpy(consts["bank_test"][:c.n_cls_test]).float(), "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=args.batch))
    B, K, S = args.batch, c.n_cls_test, g.inp_size
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    base = dict(masks="bits", band=RADIUS, overlaps=True)

    def alternative():
        h = cas.decode(enc, classes=classes, **dict(base, masks="both"))
        return h, pack_bool((h.edges > T).view(B, K, -1))
    modes = [(f"(a) masks=\"bits\", band={RADIUS}, overlaps=True", lambda: (cas.decode(enc, classes=classes, **base), None)),
             (f"(b) ... edge_threshold={T}", lambda: (cas.decode(enc, classes=classes, edge_threshold=T, **base), None)),
             ("(c) masks=\"both\", edges > t, pack", alternative)]
    # parity before any timing: every other field as without edge_threshold, the new ones against (c)'s bits
    plain, _ = modes[0][1]()
    full, _ = modes[1][1]()
    alt, alt_bits = modes[2][1]()
    torch.cuda.synchronize()
    others = ("classes", "logits", "pred", "mask_bits", "area", "box", "inter", "band_bits", "band_area", "band_inter")
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in others)
    differ = (full.edge_bits ^ alt_bits).view(-1)
    n_differ = int(sum(int(np.unpackbits(differ[i:i + 2 ** 26].cpu().numpy()).sum()) for i in range(0, differ.numel(), 2 ** 26)))
    near = int(((alt.edges - T).abs() <= 2.0 ** -21).sum())
    agree = torch.equal(torch.diagonal(full.edge_inter, dim1=1, dim2=2), full.edge_area) and n_differ <= near
    agree = agree and bool((full.edge_band <= torch.minimum(full.edge_area, full.band_area)).all())
    frac = full.edge_area.view(-1).float() / (S * S)
    share = full.edge_band.view(-1).float() / full.edge_area.view(-1).clamp(min=1).float()
    print(f"parity, {B} x {K} hypotheses: the other fields {'equal' if same else 'DIFFERENT'} to the call without edge_threshold; edge_bits "
          f"differ from masks=\"both\"'s edges > {T} in {n_differ} pixels, {near} pixels lie within 2^-21 of it; the edge map is "
          f"{100 * float(frac.min()):.1f} .. {100 * float(frac.max()):.1f} % of a plane, {100 * float(share.min()):.1f} .. "
          f"{100 * float(share.max()):.1f} % of it on the mask's band", flush=True)
    new_bytes = sum(held(t.numel() * t.element_size()) for t in (full.edge_bits, full.edge_area, full.edge_band, full.edge_inter))
    del plain, full, alt, alt_bits, differ
    for _ in range(args.warmup):
        for _, fn in modes:
            fn()
    torch.cuda.synchronize()
    times, peak = {name: [] for name, _ in modes}, {}
    for _ in range(args.rounds):
        for name, fn in modes:
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            peak[name] = torch.cuda.max_memory_allocated() - start
            del out
    print(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    print(f"{'decode(enc, classes=all, ...)':46s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s} {'peak MiB':>10s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:46s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / (B * K):12.3f} "
              f"{peak[name] / 2**20:10.1f}", flush=True)
    a, b, cc = (statistics.median(times[name]) for name, _ in modes)
    pa, pb, pc = (peak[name] for name, _ in modes)
    print(f"edge_threshold={T} with its band counts and overlaps adds (b) - (a) = {b - a:+.2f} ms to the sweep, {(b - a) / (B * K) * 1e3:.1f} us "
          f"per plane; the alternative adds (c) - (a) = {cc - a:+.2f} ms: {'below' if b - a < cc - a else 'NOT BELOW'} the alternative", flush=True)
    print(f"memory: (b) peaks {pb - pa} B above (a), the allocator's blocks of the new result tensors hold {new_bytes} B: "
          f"{'equal' if pb - pa == new_bytes else 'DIFFERENT'}; (c) peaks {(pc - pa) / 2**20:.0f} MiB above (a)", flush=True)
    return 0 if same and agree and b - a < cc - a and pb - pa == new_bytes else 1


if __name__ == "__main__":
    sys.exit(main())
