"""RegionViT training-step benchmark: the reference usage (regionvit.py:265-277: 224-pixel images, 1000 classes, widths 64 / 128 / 256 / 512,
depths 2 / 2 / 8 / 2, window_size 7: windows of 49 tokens plus their region token, region sequences of 64, 16, 4 and 1 tokens), forward +
backward without d(img) on device buffers (vitx_regionvit_forward_dev / _backward_dev).  Prints one JSON line per run: ms per step, the host's time to enqueue a step, images per
second and, from one more step under the library's profiler (vitx_regionvit_profile_begin / _end), the share of every kernel class and of
four groups: the convolutions (encoders, Downsample), the window partitions, the attention, the bias gradient.

    python tools/bench_regionvit.py [--batch 256] [--steps 6] [--warmup 2] [--compute bf16] [--repeats 2] [--window default|on|off]
    python tools/bench_regionvit.py --ab          # bf16: window_attn=True and False alternating, `--rounds` runs each, every run a child with a time limit
    python tools/bench_regionvit.py --sweep       # the three compute modes, `--rounds` runs each, every run a child with a time limit
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
GROUPS = {"convolutions": ("rv_im2col", "rv_conv_gemm", "rv_col2im", "rv_encoder"), "windows": ("rv_windows",), "attention": ("attn_window", "attn_small"),
          "bias_gradient": ("attn_dbias", "rv_bias")}
USAGE = dict(num_classes=1000)


def run(a):
    import numpy as np
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.regionvit import RegionViT
    b = a.batch
    m = RegionViT(**USAGE, compute=a.compute, max_batch=b, seed=0, image_size=224, window_attn={"default": None, "on": True, "off": False}[a.window])
    h = m._ensure_handle(b)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_regionvit_forward_dev(h, ptr(img), b, None))
        N.check(l.vitx_regionvit_backward_dev(h, ptr(dl), None))

    host = np.empty(b * 512, dtype=np.float32)

    def sync():   # a host read joins the handle's stream
        N.check(l.vitx_regionvit_read(h, b"pooled", host.ctypes.data_as(C.c_void_p), host.size, None))

    for _ in range(a.warmup):
        step()
    sync()
    times, enqueue = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        t1 = time.perf_counter()   # every launch of the window is enqueued; the GPU may still be running
        sync()
        times.append((time.perf_counter() - t0) * 1e3 / a.steps)
        enqueue.append((t1 - t0) * 1e3 / a.steps)
    ms = min(times)
    N.check(l.vitx_regionvit_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_regionvit_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): (stats[i].total_ms, stats[i].launches) for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(v[0] for v in rows.values())
    shares = {k: {"ms": round(v[0], 3), "launches": int(v[1]), "share": round(v[0] / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1][0])}
    groups = {g: round(sum(v[0] for k, v in rows.items() if k.startswith(tuple(pre))) / total, 4) for g, pre in GROUPS.items()}
    print(json.dumps({"workload": "regionvit_usage_224", "compute": a.compute, "batch": b, "steps": a.steps, "window_attn": a.window,
                      "ms_per_step": round(ms, 3), "ms_per_step_runs": [round(t, 3) for t in times], "host_enqueue_ms_per_step": [round(t, 3) for t in enqueue], "launches_per_step": int(sum(v[1] for v in rows.values())),
                      "images_per_s": round(b * 1e3 / ms, 1),
                      "profiled_kernel_ms": round(total, 3), "group_shares": groups, "kernel_classes": shares}), flush=True)


def children(a, forms):
    """One child process per run, the forms alternating, `--rounds` times each; stops at the first failure."""
    for _ in range(a.rounds):
        for extra in forms:
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--repeats", str(a.repeats), *extra]
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
    ap.add_argument("--window", default="default", choices=["default", "on", "off"],
                    help="the window attention kernels: the measured default, wherever they apply, or nowhere")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.ab:
        sys.exit(children(a, [("--compute", "bf16", "--window", "on"), ("--compute", "bf16", "--window", "off")]))
    if a.sweep:
        sys.exit(children(a, [("--compute", c) for c in ("bf16", "bf16x3", "fp32")]))
    run(a)


if __name__ == "__main__":
    main()
