"""CvT training-step benchmark: the reference usage (cvt.py:204-236: 224-pixel images, 1000 classes, emb_dim 64 / 192 / 384, heads 1 / 3 / 4,
depths 1 / 2 / 10, 3 x 3 projections with kv stride 2: 3136 / 784, 784 / 196 and 196 / 49 queries / keys), forward (training=True: batch
statistics) + backward without d(img) on device buffers (vitx_cvt_forward_dev / _backward_dev).  Prints one JSON line per run: ms per step,
images per second and, from one more step under the library's profiler (vitx_cvt_profile_begin / _end), the share of every kernel class and
of three groups: depthwise convolution + BatchNormalization, the embeddings, the attention.

    python tools/bench_cvt.py [--batch 256] [--steps 6] [--warmup 2] [--compute bf16] [--repeats 2] [--fused default|on|off]
    python tools/bench_cvt.py --ab          # bf16: fused_attn=True and False alternating, `--rounds` runs each, every run a child with a time limit
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-tensorflow_amd"))

RUN_LIMIT_S = 240
GROUPS = {"dwbn": ("cvt_dwbn_",), "embeddings": ("cvt_im2col", "cvt_conv_gemm", "cvt_col2im", "cvt_embed_norm"),
          "attention": ("attn_",)}   # attn_fewkey_*, attn_manykey_*, attn_generic_bgemm / _softmax / _headops, attn_bgemm_mfma
USAGE = dict(num_classes=1000, s3_heads=4)


def run(a):
    import numpy as np
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.cvt import CvT
    b = a.batch
    m = CvT(**USAGE, compute=a.compute, max_batch=b, seed=0, image_size=224, fused_attn={"default": None, "on": True, "off": False}[a.fused])
    h = m._ensure_handle(b)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_cvt_forward_dev(h, ptr(img), b, 1, None))
        N.check(l.vitx_cvt_backward_dev(h, ptr(dl), None))

    host = np.empty(b * 384, dtype=np.float32)

    def sync():   # a host read joins the handle's stream
        N.check(l.vitx_cvt_read(h, b"pooled", host.ctypes.data_as(C.c_void_p), host.size, None))

    for _ in range(a.warmup):
        step()
    sync()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        sync()
        times.append((time.perf_counter() - t0) * 1e3 / a.steps)
    ms = min(times)
    N.check(l.vitx_cvt_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_cvt_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): (stats[i].total_ms, stats[i].launches) for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(v[0] for v in rows.values())
    shares = {k: {"ms": round(v[0], 3), "launches": int(v[1]), "share": round(v[0] / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1][0])}
    groups = {g: round(sum(v[0] for k, v in rows.items() if k.startswith(pre)) / total, 4) for g, pre in GROUPS.items()}
    print(json.dumps({"workload": "cvt_usage_224", "compute": a.compute, "batch": b, "steps": a.steps, "fused_attn": a.fused,
                      "ms_per_step": round(ms, 3), "ms_per_step_runs": [round(t, 3) for t in times], "images_per_s": round(b * 1e3 / ms, 1),
                      "profiled_kernel_ms": round(total, 3), "group_shares": groups, "kernel_classes": shares}), flush=True)


def ab(a):
    """bf16: fused_attn=True and fused_attn=False alternating, `--rounds` times each; stops at the first failure."""
    for _ in range(a.rounds):
        for fused in ("on", "off"):
            cmd = [sys.executable, os.path.abspath(__file__), "--compute", "bf16", "--batch", str(a.batch), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--fused", fused]
            try:
                rc = subprocess.run(cmd, timeout=RUN_LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"failed": cmd, "returncode": rc}), flush=True)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2, help="timed windows of --steps steps; the fastest is reported, all are listed")
    ap.add_argument("--compute", default="bf16")
    ap.add_argument("--fused", default="default", choices=["default", "on", "off"],
                    help="the fused attention kernels: the measured default, wherever they apply, or nowhere")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    sys.exit(ab(a)) if a.ab else run(a)


if __name__ == "__main__":
    main()
