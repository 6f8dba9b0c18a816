"""Holes of packed masks on a full class sweep: demo geometry, B = 8, every class of the bank on one encoded batch --
`decode(enc, classes=all, masks="bits")` (a) as it is, (b) with components=8, min_area=64 and (c) with holes=8, fill_holes=64, one
process.  First the new fields are held against scipy on a few of the call's own planes; then, after a warm-up, the three calls
alternate, each timed with device events around it and a synchronise after it.  Reported: (c) - (a) per plane beside (b) - (a) per
plane.  Then the host alternative for the same planes: a device-to-host copy of the bits, and scipy.ndimage.label of the complement
with the same statistics (count, the 8 largest holes with boxes and seeds, the filled plane with its area) on at most 16 threads.
Nothing is gated but the parity.
--parity: instead, `infer_classes` on the two images and three classes of tests/golden/demo_classes_digest.npz against the
reference's bits: with d the pixels in which a plane differs from the reference's, |n_holes - n_ref| <= 3 d.
--kernels: instead, cvlm_mask_holes on 64 planes of 1024^2 -- the reference's planes of tests/golden/demo_classes_digest.npz,
repeated, then their complements -- `--repeat` launches each back to back (for `rocprofv3 --kernel-trace --stats -- python
tools/bench_holes.py --kernels --planes reference|complement`), with the event-timed mean.
Usage: python tools/bench_holes.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--parity] [--kernels] [--repeat R]
       [--planes reference|complement|both]"""
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
from camouflaged_vlm_amd.engine import COMPONENTS_WS_CAP, Cascade, Precision  # noqa: E402

M, BELOW, CONN = 8, 64, 8
FIELDS = ("n_holes", "holes", "n_filled", "filled_bits", "filled_area")


def host_plane(bits: np.ndarray, S: int):
    """What cvlm_mask_holes gives for one plane, with scipy: (n_holes, rows (M, 6), n_filled, filled bits, filled area)."""
    from scipy import ndimage
    plane = np.unpackbits(bits).reshape(S, S).astype(bool)
    lab, n = ndimage.label(~plane, structure=ndimage.generate_binary_structure(2, 1 if CONN == 8 else 2))
    hole = np.ones(n + 1, bool)
    hole[0] = False
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        hole[edge] = False
    area = np.bincount(lab.ravel(), minlength=n + 1)
    rows = np.tile(np.array([0, -1, -1, -1, -1, -1], np.int32), (M, 1))
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    seed = np.full(n + 1, S * S, np.int64)
    np.minimum.at(seed, flat[idx], idx)
    ids = np.nonzero(hole)[0]
    order = ids[np.lexsort((seed[ids], -area[ids]))][:M]
    objs = ndimage.find_objects(lab)
    for m, k in enumerate(order):
        sy, sx = objs[k - 1]
        rows[m] = (area[k], sx.start, sy.start, sx.stop - 1, sy.stop - 1, seed[k])
    small = hole & (area < BELOW)
    filled = plane | small[lab]
    return len(ids), rows, int(small.sum()), np.packbits(filled), int(filled.sum())


def reference_planes(S: int) -> np.ndarray:
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        return z["mask_bits"].reshape(-1, S * S // 8)


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, P = spec.DEMO_SAM.inp_size, 64
    ref = np.tile(reference_planes(S), (-(-P // 6), 1))[:P].copy()
    planes = {"reference": ("the reference's planes, repeated", torch.from_numpy(ref).to(dev)),
              "complement": ("their complements", torch.from_numpy(~ref).to(dev))}
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = (i32(P), i32(P, M, 6), i32(P), torch.empty(P, S * S // 8, dtype=torch.uint8, device=dev), i32(P))
    ws = torch.empty(min(hip.mask_holes_workspace_bytes(P, S, S), COMPONENTS_WS_CAP), dtype=torch.uint8, device=dev)
    per_plane = hip.mask_holes_workspace_bytes(1, S, S)
    print(f"workspace: {per_plane // (S * S)} bytes per pixel, {per_plane / 2**20:.0f} MiB per plane of {S} x {S}; {ws.numel() / 2**20:.0f} MiB "
          f"here: rounds of {ws.numel() // per_plane} planes", flush=True)
    for which, (what, bits) in planes.items():
        if args.planes not in ("both", which):
            continue
        fn = lambda: hip.mask_holes(bits, S, S, CONN, BELOW, ws, *out)
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
        print(f"cvlm_mask_holes: {P} planes of {S} x {S}, {what}, connectivity {CONN}, M = {M}, fill_below = {BELOW}, {args.repeat} calls "
              f"back to back: {ms * 1e3:.0f} us each, {ms * 1e3 / P:.1f} us per plane; n_holes {int(out[0].min())} .. {int(out[0].max())}",
              flush=True)
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
    h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(gold["classes"]), masks="bits", holes=M, fill_holes=BELOW, connectivity=CONN)
    torch.cuda.synchronize()
    ref = gold["mask_bits"]
    B, K, nb = ref.shape
    got = h.mask_bits.cpu().numpy()
    d = np.unpackbits(got ^ ref, axis=-1).sum(-1).astype(np.int64)
    ok = True
    for b in range(B):
        for k in range(K):
            want = host_plane(got[b, k], S)
            same = all(np.array_equal(getattr(h, f)[b, k].cpu().numpy(), w) for f, w in zip(FIELDS, want))
            n_ref, n_dev = host_plane(ref[b, k], S)[0], int(h.n_holes[b, k])
            inside = abs(n_dev - n_ref) <= 3 * d[b, k]
            ok = ok and same and inside
            print(f"demo {args.precision} image {b} class {int(gold['classes'][b, k])}: d = {d[b, k]} pixels, n_holes {n_dev} / reference {n_ref}: "
                  f"{'within' if inside else 'OUTSIDE'} 3 d; the new fields {'equal' if same else 'DIFFERENT'} to scipy on the call's own bits",
                  flush=True)
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
    ap.add_argument("--planes", default="both", choices=("reference", "complement", "both"), help="--kernels: which of the two plane sets run")
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
    modes = [("(a) masks=\"bits\"", dict(masks="bits")),
             (f"(b) ... components={M}, min_area={BELOW}", dict(masks="bits", components=M, min_area=BELOW, connectivity=CONN)),
             (f"(c) ... holes={M}, fill_holes={BELOW}", dict(masks="bits", holes=M, fill_holes=BELOW, connectivity=CONN))]
    # parity before any timing: every other field as without the new arguments, the new ones as scipy gives them on a few planes
    plain = cas.decode(enc, classes=classes, **modes[0][1])
    full = cas.decode(enc, classes=classes, **modes[2][1])
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box"))
    got = {f: getattr(full, f).view(B * K, *getattr(full, f).shape[2:]).cpu().numpy() for f in FIELDS}
    all_bits = full.mask_bits.view(B * K, -1).cpu().numpy()
    agree = True
    for p in range(0, B * K, max(1, B * K // 8)):
        want = host_plane(all_bits[p], S)
        agree = agree and all(np.array_equal(got[f][p], w) for f, w in zip(FIELDS, want))
    dense = full.area.view(-1).float() / (S * S)
    print(f"parity, {B} x {K} hypotheses: the other fields {'equal' if same else 'DIFFERENT'} to the call without holes; the new fields "
          f"{'equal' if agree else 'DIFFERENT'} to scipy on every {max(1, B * K // 8)}th plane; n_holes {got['n_holes'].min()} .. "
          f"{got['n_holes'].max()}, n_filled {got['n_filled'].min()} .. {got['n_filled'].max()}, largest hole {got['holes'][:, 0, 0].max()}; "
          f"{100 * float(dense.min()):.1f} .. {100 * float(dense.max()):.1f} % of a plane set", flush=True)
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
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts; workspace cls_comp {cas.ws._flat[('u8', 'cls_comp')].numel() / 2**20:.0f} MiB",
          flush=True)
    print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / (B * K):12.3f}", flush=True)
    base, with_c, with_h = (statistics.median(times[name]) for name, _ in modes)
    print(f"per plane: components add (b) - (a) = {(with_c - base) / (B * K) * 1e3:.1f} us, holes add (c) - (a) = "
          f"{(with_h - base) / (B * K) * 1e3:.1f} us ({(with_h - base) / max(with_c - base, 1e-9):.2f} x)", flush=True)
    # the host alternative for the same planes
    threads = min(16, os.cpu_count() or 1)
    t0 = time.perf_counter()
    host_bits = bits_dev.view(B * K, -1).cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_plane(host_bits[0], S)
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda row: host_plane(row, S), host_bits))
    t_label = time.perf_counter() - t0
    alt = (t_copy + t_label) * 1e3
    print(f"host alternative for the same {B * K} planes: copy to the host {t_copy * 1e3:.1f} ms + scipy.ndimage.label of the complement and "
          f"the same statistics on {threads} threads {t_label * 1e3:.0f} ms ({t_one * 1e3:.1f} ms for one plane on one thread) = {alt:.0f} ms; "
          f"holes add {with_h - base:+.2f} ms to the sweep on the device", flush=True)
    return 0 if same and agree else 1


if __name__ == "__main__":
    sys.exit(main())
