"""TwinsSVT training-step benchmark: the reference usage (twins_svt.py:271-298: 224-pixel images, 1000 classes, emb_dim 64 / 128 / 256 / 512,
7 x 7 windows, global_k 7, depths 1 / 1 / 5 / 4), forward + backward without d(img) on device buffers (vitx_twins_forward_dev /
_backward_dev).  Prints one JSON line per run: ms per step, images per second and, from one more step under the library's profiler
(vitx_twins_profile_begin / _end), the share of every kernel class.

    python tools/bench_twins.py [--batch 32] [--steps 8] [--warmup 2] [--compute bf16] [--repeats 2]
    python tools/bench_twins.py --sweep       # every mode, `--rounds` runs each, every run a child process with a time limit
    python tools/bench_twins.py --ab          # bf16: few-key kernels, fused_global_attn=False and VITX_GENERIC_ATTN=1 alternating, `--rounds` runs each
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

SWEEP = ["bf16", "bf16x3", "fp32"]
RUN_LIMIT_S = 240


def run(a):
    import numpy as np
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.twins_svt import TwinsSVT
    b = a.batch
    m = TwinsSVT(num_classes=1000, compute=a.compute, max_batch=b, seed=0, image_size=224,
                 fused_global_attn={"default": None, "on": True, "off": False}[a.fused])
    h = m._ensure_handle(b)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_twins_forward_dev(h, ptr(img), b, None))
        N.check(l.vitx_twins_backward_dev(h, ptr(dl), None))

    host = np.empty(b * 512, dtype=np.float32)

    def sync():   # a host read joins the handle's stream
        N.check(l.vitx_twins_read(h, b"pooled", host.ctypes.data_as(C.c_void_p), host.size, None))

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
    N.check(l.vitx_twins_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_twins_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): stats[i].total_ms for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(rows.values())
    shares = {k: {"ms": round(v, 3), "share": round(v / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}
    print(json.dumps({"workload": "twins_svt_usage_224", "compute": a.compute, "batch": b, "steps": a.steps, "fused_global_attn": a.fused,
                      "generic_attn": os.environ.get("VITX_GENERIC_ATTN", "0"), "ms_per_step": round(ms, 3),
                      "ms_per_step_runs": [round(t, 3) for t in times], "images_per_s": round(b * 1e3 / ms, 1),
                      "profiled_kernel_ms": round(total, 3), "kernel_classes": shares}), flush=True)


def sweep(a):
    """Every mode `--rounds` times, the modes alternating, every run a child with its own time limit; stops at the first failure."""
    for _ in range(a.rounds):
        for compute in SWEEP:
            cmd = [sys.executable, os.path.abspath(__file__), "--compute", compute, "--batch", str(a.batch), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            try:
                rc = subprocess.run(cmd, timeout=RUN_LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"failed": cmd, "returncode": rc}), flush=True)
                return rc
    return 0


def ab(a):
    """bf16: the few-key kernels, the same handle with fused_global_attn=False (only the global attention changes) and VITX_GENERIC_ATTN=1 (every
    attention of the model on the materialised path) alternating, `--rounds` times each; stops at the first failure."""
    for _ in range(a.rounds):
        for fused, generic in (("on", "0"), ("off", "0"), ("on", "1")):
            env = dict(os.environ)
            env.pop("VITX_GENERIC_ATTN", None)
            if generic == "1":
                env["VITX_GENERIC_ATTN"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--compute", "bf16", "--batch", str(a.batch), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--fused", fused]
            try:
                rc = subprocess.run(cmd, env=env, timeout=RUN_LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"failed": cmd, "generic_attn": generic, "returncode": rc}), flush=True)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2, help="timed windows of --steps steps; the fastest is reported, all are listed")
    ap.add_argument("--compute", default="bf16")
    ap.add_argument("--fused", default="default", choices=["default", "on", "off"],
                    help="the few-key attention kernels of the global pairs: the measured default, wherever they apply, or nowhere")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    sys.exit(sweep(a)) if a.sweep else sys.exit(ab(a)) if a.ab else run(a)


if __name__ == "__main__":
    main()
