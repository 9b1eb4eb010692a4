"""CrossViT training-step benchmark: the README configuration (README.md:325-342) in bf16 at batch 256, forward + backward on device
buffers (vitx_crossvit_forward_dev / _backward_dev).  Prints one JSON line: ms per step and images per second.

    python tools/bench_crossvit.py [--batch 256] [--steps 20] [--warmup 5] [--compute bf16]

Per-kernel time (the cross-attention kernels are crossvit_xattn_fwd_kernel / crossvit_xattn_bwd_kernel):
    rocprofv3 --kernel-trace --stats -- python tools/bench_crossvit.py --steps 3 --warmup 1
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-tensorflow_amd"))

README_KW = dict(image_size=256, num_classes=1000, depth=4, sm_dim=192, sm_patch_size=16, sm_enc_depth=2, sm_enc_heads=8, sm_enc_mlp_dim=2048,
                 lg_dim=384, lg_patch_size=64, lg_enc_depth=3, lg_enc_heads=8, lg_enc_mlp_dim=2048, cross_attn_depth=2, cross_attn_heads=8,
                 dropout=0.1, emb_dropout=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compute", default="bf16")
    a = ap.parse_args()
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.cross_vit import CrossViT
    b = a.batch
    m = CrossViT(**README_KW, compute=a.compute, max_batch=b, seed=0)
    h = m._ensure_handle(b)
    img = torch.randn(b, 256, 256, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step(i):
        N.check(l.vitx_crossvit_forward_dev(h, ptr(img), b, 256, 256, 1, 1000 + i, None))
        N.check(l.vitx_crossvit_backward_dev(h, ptr(dl), None))

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    print(json.dumps({"workload": "crossvit_readme", "compute": a.compute, "batch": b, "steps": a.steps, "ms_per_step": round(ms, 3),
                      "images_per_s": round(b * 1e3 / ms, 1)}))


if __name__ == "__main__":
    main()
