"""Connected components of packed masks on a full class sweep: demo geometry, B = 8, every class of the bank on one
encoded batch -- `decode(enc, classes=all, masks="bits")` without and with components=8, min_area=64, one process.  First the new
fields are held against scipy on a few of the call's own planes; then, after a warm-up, the two calls alternate, each timed with
device events around it and a synchronise after it, and each mode's peak allocated memory over its starting level is read after
torch.cuda.reset_peak_memory_stats().  Then the host alternative for the same planes: a device-to-host copy of the bits, and
scipy.ndimage.label with the same statistics (count, the 8 largest regions with boxes and seeds, the kept plane with area and box) on
at most 16 threads.  Condition: the device time the new arguments add is below the host alternative's time; and the peak grows by no
more than the workspace cap plus the new result tensors.  The ratio to the plain sweep is reported, not gated.
--kernels: instead, cvlm_mask_components on 64 planes of 1024^2 -- the reference's planes of tests/golden/demo_classes_digest.npz,
repeated, then 64 full planes -- `--repeat` launches each back to back (for `rocprofv3 --kernel-trace --stats -- python
tools/bench_components.py --kernels --planes reference|full`), with the event-timed mean.
Usage: python tools/bench_components.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R] [--planes reference|full|both]"""
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

M, MIN_AREA, CONN = 8, 64, 8
FIELDS = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")


def host_plane(bits: np.ndarray, S: int):
    """What cvlm_mask_components gives for one plane, with scipy: (n_comp, rows (M, 6), n_kept, kept bits, kept area, kept box)."""
    from scipy import ndimage
    plane = np.unpackbits(bits).reshape(S, S).astype(bool)
    lab, n = ndimage.label(plane, structure=ndimage.generate_binary_structure(2, 2))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    rows = np.tile(np.array([0, -1, -1, -1, -1, -1], np.int32), (M, 1))
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    seed = np.full(n + 1, S * S, np.int64)
    np.minimum.at(seed, flat[idx], idx)
    order = np.lexsort((seed[1:], -area[1:]))[:M] + 1
    objs = ndimage.find_objects(lab)
    for m, k in enumerate(order):
        sy, sx = objs[k - 1]
        rows[m] = (area[k], sx.start, sy.start, sx.stop - 1, sy.stop - 1, seed[k])
    big = area >= MIN_AREA
    kept = big[lab]
    ys, xs = np.nonzero(kept.any(1))[0], np.nonzero(kept.any(0))[0]
    box = (xs[0], ys[0], xs[-1], ys[-1]) if ys.size else (-1, -1, -1, -1)
    return n, rows, int(big.sum()), np.packbits(kept), int(kept.sum()), np.array(box, np.int32)


def kernels(args) -> int:
    dev = torch.device("cuda:0")
    S, P = spec.DEMO_SAM.inp_size, 64
    with np.load(os.path.join(REPO, "tests", "golden", "demo_classes_digest.npz")) as z:
        ref = z["mask_bits"].reshape(-1, S * S // 8)
    planes = {"reference": ("the reference's planes, repeated", torch.from_numpy(np.tile(ref, (-(-P // len(ref)), 1))[:P].copy()).to(dev)),
              "full": ("full planes", torch.full((P, S * S // 8), 255, dtype=torch.uint8, device=dev))}
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = (i32(P), i32(P, M, 6), i32(P), torch.empty(P, S * S // 8, dtype=torch.uint8, device=dev), i32(P), i32(P, 4))
    ws = torch.empty(min(hip.mask_components_workspace_bytes(P, S, S), COMPONENTS_WS_CAP), dtype=torch.uint8, device=dev)
    per_plane = hip.mask_components_workspace_bytes(1, S, S)
    print(f"workspace: {per_plane // (S * S)} bytes per pixel, {per_plane / 2**20:.0f} MiB per plane of {S} x {S}; {ws.numel() / 2**20:.0f} MiB "
          f"here: rounds of {ws.numel() // per_plane} planes", flush=True)
    for which, (what, bits) in planes.items():
        if args.planes not in ("both", which):
            continue
        fn = lambda: hip.mask_components(bits, S, S, CONN, MIN_AREA, ws, *out)
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
        print(f"cvlm_mask_components: {P} planes of {S} x {S}, {what}, connectivity {CONN}, M = {M}, min_area = {MIN_AREA}, {args.repeat} calls "
              f"back to back: {ms * 1e3:.0f} us each, {ms * 1e3 / P:.1f} us per plane; n_comp {int(out[0].min())} .. {int(out[0].max())}",
              flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="mx")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--planes", default="both", choices=("reference", "full", "both"), help="--kernels: which of the two plane sets run")
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
    modes = [("masks=\"bits\"", dict(masks="bits")),
             (f"... components={M}, min_area={MIN_AREA}", dict(masks="bits", components=M, min_area=MIN_AREA, connectivity=CONN))]
    # parity before any timing: every other field as without the new arguments, the new ones as scipy gives them on a few planes
    plain = cas.decode(enc, classes=classes, **modes[0][1])
    full = cas.decode(enc, classes=classes, **modes[1][1])
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box"))
    got = {f: getattr(full, f).view(B * K, *getattr(full, f).shape[2:]).cpu().numpy() for f in FIELDS}
    all_bits = full.mask_bits.view(B * K, -1).cpu().numpy()
    agree = True
    for p in range(0, B * K, max(1, B * K // 8)):
        want = host_plane(all_bits[p], S)
        agree = agree and all(np.array_equal(got[f][p], w) for f, w in zip(FIELDS, want))
    results = sum(getattr(full, f).numel() * getattr(full, f).element_size() for f in FIELDS)
    print(f"parity, {B} x {K} hypotheses: the other fields {'equal' if same else 'DIFFERENT'} to the call without components; the new fields "
          f"{'equal' if agree else 'DIFFERENT'} to scipy on every {max(1, B * K // 8)}th plane; n_comp {got['n_comp'].min()} .. "
          f"{got['n_comp'].max()}, n_kept {got['n_kept'].min()} .. {got['n_kept'].max()}", flush=True)
    del plain, full
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
            bits_dev = h.mask_bits
            del h
    (na, _), (nb, _) = modes
    base, with_c = statistics.median(times[na]), statistics.median(times[nb])
    print(f"demo geometry, B = {B}, all {K} classes ({B * K} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts; workspace cls_comp {cas.ws._flat[('u8', 'cls_comp')].numel() / 2**20:.0f} MiB",
          flush=True)
    print(f"{'decode(enc, classes=all, ...)':38s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s} {'peak over start':>16s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:38s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / (B * K):12.3f} "
              f"{peak[name] / 2**20:12.1f} MiB", flush=True)
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
    added, alt = with_c - base, (t_copy + t_label) * 1e3
    print(f"host alternative for the same {B * K} planes: copy to the host {t_copy * 1e3:.1f} ms + scipy.ndimage.label and the same statistics "
          f"on {threads} threads {t_label * 1e3:.0f} ms ({t_one * 1e3:.1f} ms for one plane on one thread) = {alt:.0f} ms", flush=True)
    ok_time = added < alt
    print(f"components add {added:+.2f} ms to the sweep ({with_c / base:.3f} x the plain sweep, {added / (B * K) * 1e3:.1f} us per plane): "
          f"{'below' if ok_time else 'NOT BELOW'} the host alternative's {alt:.0f} ms", flush=True)
    grow = peak[nb] - peak[na]
    ok_mem = grow <= COMPONENTS_WS_CAP + results
    print(f"peak grows by {grow / 2**20:.1f} MiB; the new result tensors are {results / 2**20:.1f} MiB, the workspace cap {COMPONENTS_WS_CAP / 2**20:.0f} "
          f"MiB: {'within' if ok_mem else 'ABOVE'} cap + results", flush=True)
    return 0 if ok_time and ok_mem and same and agree else 1


if __name__ == "__main__":
    sys.exit(main())
