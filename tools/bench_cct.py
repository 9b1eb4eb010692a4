"""CCT training-step benchmark: cct_14(img_size=224, n_conv_layers=2, kernel_size=7, num_classes=1000, positional_embedding='learnable') in bf16
at batch 256, forward + backward on device buffers (vitx_cct_forward_dev / _backward_dev).  Prints one JSON line: ms per step, images per
second and, from one more step under the library's profiler (vitx_cct_profile_begin / _end), the share of every kernel class
the CCT composite adds (cct_*).

    python tools/bench_cct.py [--batch 256] [--steps 10] [--warmup 3] [--compute bf16]
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

KW = dict(img_size=224, n_conv_layers=2, kernel_size=7, num_classes=1000, positional_embedding='learnable')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compute", default="bf16")
    a = ap.parse_args()
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.cct import cct_14
    b = a.batch
    m = cct_14(**KW, compute=a.compute, max_batch=b, seed=0)
    h = m._ensure_handle(b)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_cct_forward_dev(h, ptr(img), b, None))
        N.check(l.vitx_cct_backward_dev(h, ptr(dl), None))

    import numpy as np
    host = np.empty(b * 384, dtype=np.float32)

    def sync():   # a host read joins the handle's stream
        N.check(l.vitx_cct_read(h, b"pooled", host.ctypes.data_as(C.c_void_p), host.size, None))

    for _ in range(a.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    N.check(l.vitx_cct_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_cct_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): stats[i].total_ms for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(rows.values())
    shares = {k: {"ms": round(v, 3), "share": round(v / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1]) if k.startswith("cct_")}
    print(json.dumps({"workload": "cct_14_224_2conv7", "compute": a.compute, "batch": b, "steps": a.steps, "tokens": m.sequence_length,
                      "ms_per_step": round(ms, 3), "images_per_s": round(b * 1e3 / ms, 1), "profiled_kernel_ms": round(total, 3),
                      "cct_kernel_classes": shares}))


if __name__ == "__main__":
    main()
