#!/usr/bin/env python3
"""A/B of the streamed-key attention path (ViT(..., long_attn=True), csrc/attn_stream.hip) against the materialised path on ViT-B/16 in the bf16
mode: forward + backward ms per step through the device entry points, and the device memory each mode holds (hipMemGetInfo deltas around the
handle's life: the library allocates outside torch's caching allocator).  Modes alternate, each run on a fresh handle.

    python tools/bench_long_attn.py --image 384 --batch 64 [--runs 3 --steps 10 --warmup 3]

One line per run and a JSON summary line; profiles/long_attn/ holds the logs DESIGN.md quotes."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def one_run(args, long_attn):
    import torch
    from vit_tensorflow import ViT
    from vit_tensorflow import _native as N
    lib = N.lib()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    m = ViT(image_size=args.image, patch_size=16, num_classes=1000, dim=768, depth=args.depth, heads=12, mlp_dim=3072, compute="bf16",
            max_batch=args.batch, seed=0, long_attn=long_attn)
    h = m._ensure_handle(args.batch)
    img = torch.randn(args.batch, args.image, args.image, 3, device="cuda")
    labels = torch.randint(0, 1000, (args.batch,), device="cuda", dtype=torch.int32)

    def step():
        N.check(lib.vitx_forward_dev(h, C.c_void_p(img.data_ptr()), args.batch, args.image, args.image, 0, 0, None))
        N.check(lib.vitx_ce_loss_grad_dev(h, C.c_void_p(labels.data_ptr()), 1.0 / args.batch, None))
        N.check(lib.vitx_backward_dev(h, None, None))

    for _ in range(args.warmup):
        step()
    N.check(lib.vitx_sync(h))
    import time
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    N.check(lib.vitx_sync(h))
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    held = free0 - torch.cuda.mem_get_info()[0] - img.numel() * 4
    prof = m.profile(step)
    attn_ms = sum(v[1] for k, v in prof.items() if k.startswith(("attn_", "softmax")))
    classes = sorted(k for k in prof if k.startswith(("attn_", "softmax")))
    N.check(lib.vitx_destroy(h))
    m._handle = None
    return ms, held / 2 ** 30, attn_ms, classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", type=int, default=384)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tokens = (args.image // 16) ** 2 + 1
    res = {"off": [], "on": []}
    for r in range(args.runs):
        for mode in ("off", "on"):
            ms, gib, attn_ms, classes = one_run(args, mode == "on")
            res[mode].append(ms)
            print(f"image {args.image} tokens {tokens} batch {args.batch} run {r} long_attn {mode}: {ms:.2f} ms/step fwd+bwd, attention classes {attn_ms:.2f} ms "
                  f"of a profiled step, device memory held {gib:.2f} GiB, classes {','.join(classes)}", flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    print(json.dumps({"image": args.image, "tokens": tokens, "batch": args.batch, "depth": args.depth, "ms_per_step_off": res["off"], "ms_per_step_on": res["on"],
                      "median_off": med["off"], "median_on": med["on"], "on_over_off": med["on"] / med["off"]}))


if __name__ == "__main__":
    main()
