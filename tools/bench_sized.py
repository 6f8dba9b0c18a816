"""Masks at each image's own size on a full class sweep: demo geometry, B = 8, every class of the bank on one encoded
batch -- `decode(enc, classes=all, masks="bits", min_area=64)` (a) as it is and (b) with sizes=... and rle="sized", one process.  The
sizes are drawn once, with a fixed seed, from eight typical photo sizes, reductions and enlargements of the model's 1024^2 among them.
First the new fields are held against the call without them and against numpy on a few of the call's own planes; then, after a
warm-up, the two calls alternate, each timed with device events around it and a synchronise after it.  Reported: (b) - (a) per plane
and per sweep, the bytes of the sized bits and of the counts, and the peak memory of both beside masks="both".  Then the host
alternative for the same planes, the only route to COCO output at the images' sizes without this: masks="both", `evaltail.mask_to_u8`
per image, the compare on the device, a device-to-host copy, then numpy.packbits, the transpose and the run boundaries on at most 16
threads.  Gated: the parity, and the added device time below the host alternative.
--kernels: instead, cvlm_mask_pack_sized on 64 planes of 1024^2 -> 683 x 1024 and -> 1500 x 2000 beside cvlm_mask_to_u8 on the same,
`--repeat` calls each back to back (for `rocprofv3 --kernel-trace --stats -- python tools/bench_sized.py --kernels`), with the
event-timed means, the bytes moved and the rate.
Usage: python tools/bench_sized.py [--rounds N] [--warmup W] [--batch B] [--precision mx|exact] [--kernels] [--repeat R]"""
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
from camouflaged_vlm_amd import evaltail, hip, host, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision, sized_tables  # noqa: E402

PHOTO_SIZES = [(480, 640), (427, 640), (640, 480), (683, 1024), (768, 1024), (1080, 1920), (1500, 2000), (1333, 2000)]


def host_counts(mask: np.ndarray) -> np.ndarray:
    """bool (h, w) -> the plane's run counts by the definition: transpose, the positions that differ from their predecessor."""
    f = np.ascontiguousarray(mask.T).reshape(-1).view(np.int8)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0)


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
    yy, xx = np.mgrid[0:S, 0:S]
    rng = np.random.default_rng(19)
    plane = (6 * np.sin(yy / 170.0) * np.cos(xx / 230.0) + rng.normal(0, 1.5, (S, S))).astype(np.float32)
    logits = torch.from_numpy(plane).to(dev).expand(P, S, S).contiguous()
    # the streaming rate this is held against: a device-to-device copy of the same logits
    copy = torch.empty_like(logits)
    ms_copy = timed(lambda: copy.copy_(logits), args.repeat)
    rate = 2 * logits.numel() * 4 / ms_copy / 1e6
    print(f"device copy of {P} planes of {S}^2 f32 ({logits.numel() * 4 / 2**20:.0f} MiB read + written): {ms_copy * 1e3:.0f} us = {rate:.0f} GB/s", flush=True)
    del copy
    for h, w in ((683, 1024), (1500, 2000)):
        dims, off, max_words = sized_tables([(h, w)] * P)
        bits = torch.empty(int(off[P]), dtype=torch.uint8, device=dev)
        area, box = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, 4, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        d, o = torch.from_numpy(dims).to(dev), torch.from_numpy(off).to(dev)
        ms_pack = timed(lambda: hip.mask_pack_sized(logits, d, o, 128, bits, max_words, area, box, status), args.repeat)
        assert int(status) == 0
        u8 = torch.empty(P, h, w, dtype=torch.uint8, device=dev)
        ms_u8 = timed(lambda: hip.mask_to_u8(logits, h, w, u8), args.repeat)
        same = int((u8 >= 128).sum()) == int(area.sum())
        moved_pack = logits.numel() * 4 + bits.numel()
        moved_u8 = logits.numel() * 4 + u8.numel()
        px = P * h * w
        print(f"{P} planes {S}^2 -> {h} x {w}, {args.repeat} calls back to back: cvlm_mask_pack_sized {ms_pack * 1e3:.0f} us, "
              f"{moved_pack / 2**20:.0f} MiB moved at most ({moved_pack / ms_pack / 1e6:.0f} GB/s = {100 * moved_pack / ms_pack / 1e6 / rate:.0f} % of "
              f"the copy's rate), {px / ms_pack / 1e6:.1f} Gpx/s = {4 * px / ms_pack / 1e6:.0f} G sigmoid/s; cvlm_mask_to_u8 {ms_u8 * 1e3:.0f} us, "
              f"{moved_u8 / 2**20:.0f} MiB ({moved_u8 / ms_u8 / 1e6:.0f} GB/s), {px / ms_u8 / 1e6:.1f} Gpx/s; set pixels "
              f"{'equal' if same else 'DIFFERENT'} to (u8 >= 128)", flush=True)
        del u8, bits
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
    sizes = [PHOTO_SIZES[i] for i in np.random.default_rng(19).integers(0, len(PHOTO_SIZES), B)]
    if B >= 2:
        sizes[0], sizes[1] = PHOTO_SIZES[0], PHOTO_SIZES[6]            # a reduction and an enlargement whatever was drawn
    classes = torch.arange(K, dtype=torch.int64).repeat(B, 1)
    enc = cas.encode(inp, ci, cm)
    base_kw = dict(masks="bits", min_area=64)
    modes = [("(a) masks=\"bits\", min_area=64", base_kw), ("(b) ... sizes=, rle=\"sized\"", dict(base_kw, sizes=sizes, rle="sized")),
             ("(c) masks=\"both\", min_area=64", dict(base_kw, masks="both"))]
    # parity before any timing
    plain = cas.decode(enc, classes=classes, **base_kw)
    full = cas.decode(enc, classes=classes, **modes[1][1])
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(plain, f), getattr(full, f)) for f in ("classes", "logits", "pred", "mask_bits", "area", "box", "kept_bits",
                                                                           "kept_area", "n_kept", "n_comp"))
    full.sized.check()
    full.rle.check()
    off, cnt = full.rle.offsets.cpu().numpy(), full.rle.counts.cpu().numpy()
    some = list(range(0, P, max(1, P // 8)))
    agree = all(np.array_equal(cnt[off[p]:off[p + 1]], host_counts(full.sized.to_numpy(p))) for p in some)
    areas = full.sized.area.cpu().numpy()
    agree = agree and all(int(areas[p]) == int(full.sized.to_numpy(p).sum()) for p in some)
    print(f"parity, {B} x {K} hypotheses at the sizes {sizes}: the other fields {'equal' if same else 'DIFFERENT'} to the call without sizes; "
          f"counts and areas {'equal' if agree else 'DIFFERENT'} to numpy on every {max(1, P // 8)}th plane of the call's own sized bits", flush=True)
    n = full.rle.n_runs
    print(f"sized bits {full.sized.bits.numel() / 2**20:.1f} MiB beside {full.mask_bits.numel() / 2**20:.0f} MiB of mask_bits; rle=\"sized\": "
          f"{full.rle.counts.numel()} runs = {full.rle.counts.numel() * 4 / 2**20:.1f} MiB of counts, n_runs per plane {int(n.min())} .. {int(n.max())}, "
          f"median {int(n.float().median())}", flush=True)
    del plain, full
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
            del h
    print(f"demo geometry, B = {B}, all {K} classes ({P} prompts), precision {args.precision}, {args.rounds} alternating rounds after "
          f"{args.warmup} warm-up; class chunk {cas.class_chunk()} prompts", flush=True)
    print(f"{'decode(enc, classes=all, ...)':42s} {'ms / call':>10s} {'min':>9s} {'max':>9s} {'ms / prompt':>12s} {'peak MiB':>9s}")
    for name, _ in modes:
        t = times[name]
        print(f"{name:42s} {statistics.median(t):10.2f} {min(t):9.2f} {max(t):9.2f} {statistics.median(t) / P:12.3f} {peaks[name] / 2**20:9.1f}",
              flush=True)
    base, with_s, both = (statistics.median(times[name]) for name, _ in modes)
    added = with_s - base
    print(f"sizes= and rle=\"sized\" add (b) - (a) = {added:+.2f} ms to the sweep, {added / P * 1e3:.1f} us per plane, {100 * added / base:.1f} % of (a)",
          flush=True)
    # the host alternative for the same planes: from masks="both" (its sweep costs (c) - (a) more than (a) already)
    threads = min(16, os.cpu_count() or 1)
    h = cas.decode(enc, classes=classes, **modes[2][1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_masks = []
    for b, (hh, ww) in enumerate(sizes):
        host_masks.append((evaltail.mask_to_u8(h.masks[b], hh, ww) >= 128).cpu().numpy())
    t_dev = time.perf_counter() - t0

    def encode(m):
        np.packbits(m, axis=1)
        return len(host_counts(m))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        runs = sum(pool.map(encode, [m for per_image in host_masks for m in per_image]))
    t_enc = time.perf_counter() - t0
    alt = (t_dev + t_enc) * 1e3
    print(f"host alternative for the same {P} planes: masks=\"both\" costs (c) - (a) = {both - base:+.2f} ms and {(peaks[modes[2][0]] - peaks[modes[0][0]]) / 2**20:.0f} MiB "
          f"more than (a); then mask_to_u8 per image, compare and copy to the host {t_dev * 1e3:.0f} ms + packbits, transpose and run boundaries "
          f"on {threads} threads {t_enc * 1e3:.0f} ms ({runs} runs) = {alt:.0f} ms; the device adds {added:+.2f} ms: "
          f"{'below' if added < alt else 'NOT BELOW'} the host alternative", flush=True)
    return 0 if same and agree and added < alt else 1


if __name__ == "__main__":
    sys.exit(main())
