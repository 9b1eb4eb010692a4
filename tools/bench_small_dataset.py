"""vit_for_small_dataset.ViT training-step benchmark: the reference's usage configuration (vit_for_small_dataset.py:218-228: image 256, patch 16,
dim 1024, depth 6, heads 16, mlp_dim 2048 -> 257 tokens) in bf16 at batch 256, forward + backward on device buffers, and in the same run the
plain vit.ViT of the same configuration.  Prints one JSON line: ms per step of both, their ratio, and the share of the attn_lsa_* / spt_*
kernel classes in one profiled step (vitx_profile_begin / _end).

    python tools/bench_small_dataset.py [--batch 256] [--steps 10] [--warmup 3] [--compute bf16]
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

USAGE_KW = dict(image_size=256, patch_size=16, num_classes=1000, dim=1024, depth=6, heads=16, mlp_dim=2048, dropout=0.1, emb_dropout=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compute", default="bf16")
    a = ap.parse_args()
    import torch
    from vit_tensorflow import ViT as PlainViT
    from vit_tensorflow import _native as N
    from vit_tensorflow.vit_for_small_dataset import ViT
    b = a.batch
    img = torch.randn(b, 256, 256, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = {"workload": "vit_for_small_dataset_usage", "compute": a.compute, "batch": b, "steps": a.steps}
    for tag, cls in (("small_dataset", ViT), ("plain_vit", PlainViT)):
        m = cls(**USAGE_KW, compute=a.compute, max_batch=b, seed=0)
        h = m._ensure_handle(b)

        def step(i):
            N.check(l.vitx_forward_dev(h, ptr(img), b, 256, 256, 1, 1000 + i, None))
            N.check(l.vitx_backward_dev(h, ptr(dl), None))

        for i in range(a.warmup):
            step(i)
        N.check(l.vitx_sync(h))
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(i)
        N.check(l.vitx_sync(h))
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        out[tag + "_ms_per_step"] = round(ms, 3)
        if tag == "small_dataset":
            N.check(l.vitx_profile_begin(h))
            step(0)
            N.check(l.vitx_sync(h))
            stats = (N.KernelStat * 256)()
            n = C.c_int32()
            N.check(l.vitx_profile_end(h, stats, 256, C.byref(n)))
            rows = {stats[i].name.decode(): stats[i].total_ms for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
            total = sum(rows.values())
            out["profiled_step_kernel_ms"] = round(total, 3)
            for k in ("attn_lsa_fwd", "attn_lsa_bwd", "spt_fwd", "spt_bwd"):
                out[k + "_ms"] = round(rows.get(k, 0.0), 3)
                out[k + "_share"] = round(rows.get(k, 0.0) / total, 4) if total else None
        del m
    out["ratio_small_dataset_over_plain"] = round(out["small_dataset_ms_per_step"] / out["plain_vit_ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
