"""Edge bands of packed masks on a full class sweep: demo geometry, B = 8, every class of the bank on one encoded
batch -- `decode(enc, classes=all, masks="bits", overlaps=True)` (a) as it is and (b) with band=2, one process.  First the new fields
are held against the reference's own max_pool2d lines on a few of the call's own planes; then, after a warm-up, the two calls
alternate, each timed with device events around it and a synchronise after it.  Reported: (b) - (a) per plane and per sweep.  Then
the host alternative for the same planes: a device-to-host copy of the bits, numpy.unpackbits and the reference's two max_pool2d
lines (models/sam_maskdecoder_edge.py:441-445) on at most 16 threads.  Nothing is gated but the parity.
--parity: instead, `infer_classes(..., masks="bits", band=2)` on the two images and three classes of
tests/golden/demo_classes_digest.npz against the reference's band of the reference's own bits: with d the pixels in which a plane
differs from the reference's, popcount(band XOR band_ref) <= (2 r + 1)^2 d -- one flipped pixel changes dilation and erosion only
inside its own window.
--kernels: instead, cvlm_mask_morph, band only, on 64 planes of 1024^2 -- the reference's planes, repeated -- at r = 2 and r = 16,
`--repeat` launches each back to back (for `rocprofv3 --kernel-trace --stats -- python tools/bench_morph.py --kernels`), with the
event-timed mean and the implied bytes per second over the planes read and written.
Usage: python tools/bench_morph.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--parity] [--kernels] [--repeat R]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from camouflaged_vlm_amd import hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402

RADIUS = 2


def host_band(bits: np.ndarray, S: int, r: int = RADIUS) -> np.ndarray:
    """uint8 [P, S * S / 8] -> the packed bands, by the reference's lines on the unpacked planes."""
    mask = torch.from_numpy(np.unpackbits(bits, axis=-1).reshape(-1, 1, S, S)).float()
    edge_ks = 2 * r + 1
    eroded = -F.max_pool2d(-mask, edge_ks, stride=1, padding=edge_ks // 2)
    dilated = F.max_pool2d(mask, edge_ks, stride=1, padding=edge_ks // 2)
    return np.packbits(((dilated - eroded) > 0).numpy().reshape(bits.shape[0], S * S), axis=-1)


def reference_planes(S: int) -> np.ndarray:
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        return z["mask_bits"].reshape(-1, S * S // 8)


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, P = spec.DEMO_SAM.inp_size, 64
    bits = torch.from_numpy(np.tile(reference_planes(S), (-(-P // 6), 1))[:P].copy()).to(dev)
    band = torch.empty_like(bits)
    area = torch.empty(P, dtype=torch.int32, device=dev)
    for r in (2, 16):
        fn = lambda: hip.mask_morph(bits, S, S, r, band_bits=band, band_area=area)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeat):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.repeat
        moved = 2 * bits.numel()
        print(f"cvlm_mask_morph: {P} planes of {S} x {S}, the reference's planes repeated, band only, r = {r}, {args.repeat} calls back to "
              f"back: {ms * 1e3:.0f} us each, {ms * 1e3 / P:.2f} us per plane, {moved / ms / 1e6:.1f} GB/s over the {moved / 2**20:.0f} MiB read "
              f"and written; band_area {int(area.min())} .. {int(area.max())}", flush=True)
    return 0


def engine(args):
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}
    cas = Cascade(sd, g, c, dev, Precision.named(args.precision))
    return g, c, dev, cas


def parity(args) -> int:
    g, c, dev, cas = engine(args)
    S = g.inp_size
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        gold = {k: z[k] for k in z.files}
    with np.load(os.path.join(REPO, "tests", "golden", "ovcamo_constants.npz")) as z:
        bank = torch.from_numpy(z["bank_test"]).float()
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), bank, "test")
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))
    h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(gold["classes"]), masks="bits", band=RADIUS)
    torch.cuda.synchronize()
    ref = gold["mask_bits"]
    B, K, nb = ref.shape
    got, band = h.mask_bits.cpu().numpy(), h.band_bits.cpu().numpy()
    d = np.unpackbits(got ^ ref, axis=-1).sum(-1).astype(np.int64)
    own = host_band(got.reshape(B * K, nb), S).reshape(B, K, nb)
    theirs = host_band(ref.reshape(B * K, nb), S).reshape(B, K, nb)
    diff = np.unpackbits(band ^ theirs, axis=-1).sum(-1).astype(np.int64)
    ok = True
    for b in range(B):
        for k in range(K):
            same = np.array_equal(band[b, k], own[b, k])
            inside = diff[b, k] <= (2 * RADIUS + 1) ** 2 * d[b, k]
            ok = ok and same and inside
            print(f"demo {args.precision} image {b} class {int(gold['classes'][b, k])}: d = {d[b, k]} pixels, band differs from the reference's "
                  f"band in {diff[b, k]} pixels: {'within' if inside else 'OUTSIDE'} {(2 * RADIUS + 1) ** 2} d = {(2 * RADIUS + 1) ** 2 * d[b, k]}; "
                  f"band_area {int(h.band_area[b, k])}; band {'equal' if same else 'DIFFERENT'} to max_pool2d on the call's own bits", flush=True)
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
    modes = [("(a) masks=\"bits\", overlaps=True", dict(masks="bits", overlaps=True)),
             (f"(b) ... band={RADIUS}", dict(masks="bits", overlaps=True, band=RADIUS))]
    # parity before any timing: every other field as without band, the new ones as the reference's lines give them on a few planes
    plain = cas.decode(enc, classes=classes, **modes[0][1])
    full = cas.decode(enc, classes=classes, **modes[1][1])
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box", "inter"))
    all_bits = full.mask_bits.view(B * K, -1).cpu().numpy()
    got = full.band_bits.view(B * K, -1).cpu().numpy()
    some = list(range(0, B * K, max(1, B * K // 8)))
    agree = np.array_equal(got[some], host_band(all_bits[some], S))
    agree = agree and np.array_equal(full.band_area.view(-1).cpu().numpy(), np.unpackbits(got, axis=-1).sum(-1))
    agree = agree and torch.equal(torch.diagonal(full.band_inter, dim1=1, dim2=2), full.band_area)
    frac = full.band_area.view(-1).float() / (S * S)
    print(f"parity, {B} x {K} hypotheses: the other fields {'equal' if same else 'DIFFERENT'} to the call without band; band_bits "
          f"{'equal' if agree else 'DIFFERENT'} to the reference's max_pool2d lines on every {max(1, B * K // 8)}th plane, band_area to the "
          f"popcounts and to band_inter's diagonal; the band is {100 * float(frac.min()):.1f} .. {100 * float(frac.max()):.1f} % of a plane",
          flush=True)
    del plain, full
    for _ in range(args.warmup):
        for _, kw in modes:
            cas.decode(enc, classes=classes, **kw)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    for _ in range(args.rounds):
        for name, kw in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h = cas.decode(enc, classes=classes, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            bits_dev = h.mask_bits
            del h
    print(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / (B * K):12.3f}", flush=True)
    base, with_b = (statistics.median(times[name]) for name, _ in modes)
    print(f"band={RADIUS} with its overlaps adds (b) - (a) = {with_b - base:+.2f} ms to the sweep, {(with_b - base) / (B * K) * 1e3:.1f} us per "
          f"plane", flush=True)
    # the host alternative for the same planes
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    host_bits = bits_dev.view(B * K, -1).cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_band(host_bits[:1], S)
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    for p0 in range(0, B * K, 8):                                                 # 8 planes at a time: 32 MiB of floats per tensor
        host_band(host_bits[p0:p0 + 8], S)
    t_pool = time.perf_counter() - t0
    alt = (t_copy + t_pool) * 1e3
    print(f"host alternative for the same {B * K} planes: copy to the host {t_copy * 1e3:.1f} ms + unpackbits and the reference's two "
          f"max_pool2d lines on {threads} threads {t_pool * 1e3:.0f} ms ({t_one * 1e3:.1f} ms for the first plane) = {alt:.0f} ms; the device "
          f"adds {with_b - base:+.2f} ms: {'below' if with_b - base < alt else 'NOT BELOW'} the host alternative", flush=True)
    return 0 if same and agree and with_b - base < alt else 1


if __name__ == "__main__":
    sys.exit(main())
