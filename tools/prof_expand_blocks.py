"""cvlm_expand_blocks against the per-image copies it replaces, for one kernel trace: demo sizes (T = 4096 tokens, C = 256, six decoder
tokens), B = 8 images, P = 40 prompts (K = 5 per image).  Per round: the five tensors of the decoder's image state -- keys f32, keys
planes, queries f32, queries planes, edge_feat f32 -- expanded by one launch each, then as the decoder issues them (three launches:
f32 and planes of a tensor together), then the same blocks moved by `dst[b * K:(b + 1) * K].copy_(src[b].expand(K, ...))`, eight
copies per tensor.  Run under `rocprofv3 --kernel-trace --stats -- python tools/prof_expand_blocks.py` (no counters) and read the
kernel rows; without a profiler it prints device-event times of the three forms and the bytes each moves.
Usage: python tools/prof_expand_blocks.py [--rounds N]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camouflaged_vlm_amd import hip  # noqa: E402
from camouflaged_vlm_amd.hip import H2  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, K, T, C, NT = 8, 5, 4096, 256, 6
    P = B * K
    image_of = torch.arange(P, dtype=torch.int32, device=dev) // K
    sizes = {"keys": T * C, "queries": NT * C, "edge_feat": 16 * T * (C // 8)}
    src_f = {n: torch.randn(B, e, device=dev) for n, e in sizes.items()}
    dst_f = {n: torch.empty(P, e, device=dev) for n, e in sizes.items()}
    src_h = {n: H2(torch.randn(2, B, sizes[n], device=dev).half()) for n in ("keys", "queries")}
    dst_h = {n: H2.empty(P, sizes[n], device=dev) for n in ("keys", "queries")}
    moved = sum(2 * 4 * P * e for e in sizes.values()) + sum(2 * 4 * P * sizes[n] for n in ("keys", "queries"))   # read + written

    def five():
        for n in sizes:
            hip.expand_blocks(image_of, P, B, sizes[n], src_f32=src_f[n], dst_f32=dst_f[n])
        for n in src_h:
            hip.expand_blocks(image_of, P, B, sizes[n], src_h2=src_h[n], dst_h2=dst_h[n])

    def three():
        for n in src_h:
            hip.expand_blocks(image_of, P, B, sizes[n], src_f32=src_f[n], dst_f32=dst_f[n], src_h2=src_h[n], dst_h2=dst_h[n])
        hip.expand_blocks(image_of, P, B, sizes["edge_feat"], src_f32=src_f["edge_feat"], dst_f32=dst_f["edge_feat"])

    def copies():
        for b in range(B):
            for n in sizes:
                dst_f[n][b * K:(b + 1) * K].copy_(src_f[n][b:b + 1].expand(K, -1))
            for n in src_h:
                dst_h[n].t[:, b * K:(b + 1) * K].copy_(src_h[n].t[:, b:b + 1].expand(2, K, -1))

    forms = [("expand_blocks, 5 launches", five), ("expand_blocks, 3 launches", three), ("copy_, 8 per tensor", copies)]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    for n in sizes:
        assert torch.equal(dst_f[n].view(B, K, -1), src_f[n][:, None].expand(B, K, -1))
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    print(f"B = {B}, P = {P}: {moved / 2**20:.0f} MiB read + written per form; {args.rounds} rounds, device events around each form (us)")
    for name, _ in forms:
        t = times[name]
        print(f"{name:28s} median {statistics.median(t):8.1f}  min {min(t):8.1f}  max {max(t):8.1f}  "
              f"{moved / statistics.median(t) / 1e6:7.2f} TB/s")


if __name__ == "__main__":
    main()
