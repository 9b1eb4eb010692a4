"""NesT training-step benchmark: the reference usage (nest.py:218-231: image 224, patch 4, dim 96, heads 3, three hierarchies, block_repeats
(2, 2, 8), 1000 classes; dim_head 32 and 196 tokens per block at every level) at batch 256, forward + backward on device buffers
(vitx_nest_forward_dev / _backward_dev).  Prints one JSON line per run: ms per step, images per second and, from one more step under the
library's profiler (vitx_nest_profile_begin / _end), the share of every kernel class.

    python tools/bench_nest.py [--batch 256] [--steps 10] [--warmup 3] [--compute bf16x3] [--dim 96] [--heads 3] [--repeats 3]
    python tools/bench_nest.py --sweep       # every mode, small-head kernels and VITX_GENERIC_ATTN=1 alternating, each run a child with a time limit

The bf16 mode refuses dim 96 (widths in multiples of 64): it is measured on the same model at dim 128, heads 4 (dim_head 32 as well)."""
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

KW = dict(image_size=224, patch_size=4, num_hierarchies=3, block_repeats=(2, 2, 8), num_classes=1000)
SWEEP = [("bf16x3", 96, 3), ("fp32", 96, 3), ("bf16", 128, 4)]
RUN_LIMIT_S = 240


def run(a):
    import numpy as np
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.nest import NesT
    b = a.batch
    m = NesT(**KW, dim=a.dim, heads=a.heads, compute=a.compute, max_batch=b, seed=0, small_attn={"default": None, "on": True, "off": False}[a.small_attn])
    h = m._ensure_handle(b)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_nest_forward_dev(h, ptr(img), b, None))
        N.check(l.vitx_nest_backward_dev(h, ptr(dl), None))

    host = np.empty(b * a.dim * 4, dtype=np.float32)

    def sync():   # a host read joins the handle's stream
        N.check(l.vitx_nest_read(h, b"pooled", host.ctypes.data_as(C.c_void_p), host.size, None))

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
    N.check(l.vitx_nest_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_nest_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): stats[i].total_ms for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(rows.values())
    shares = {k: {"ms": round(v, 3), "share": round(v / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}
    print(json.dumps({"workload": "nest_usage_224", "compute": a.compute, "dim": a.dim, "heads": a.heads, "batch": b, "steps": a.steps,
                      "small_attn": a.small_attn, "generic_attn": os.environ.get("VITX_GENERIC_ATTN", "0"), "ms_per_step": round(ms, 3),
                      "ms_per_step_runs": [round(t, 3) for t in times], "images_per_s": round(b * 1e3 / ms, 1),
                      "profiled_kernel_ms": round(total, 3), "kernel_classes": shares}), flush=True)


def sweep(a):
    """Every mode: the small-head kernels (asked for: they are the default only where this comparison found them faster) and the materialised
    attention path (VITX_GENERIC_ATTN=1: the attention the library ran before the small-head kernels) alternating, `--rounds` times each, every run a child with its own time limit; stops at the first failure."""
    for compute, dim, heads in SWEEP:
        for _ in range(a.rounds):
            for generic in ("0", "1"):
                env = dict(os.environ)
                env.pop("VITX_GENERIC_ATTN", None)
                if generic == "1":
                    env["VITX_GENERIC_ATTN"] = "1"
                cmd = [sys.executable, os.path.abspath(__file__), "--compute", compute, "--dim", str(dim), "--heads", str(heads), "--batch", str(a.batch),
                       "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--small-attn", "on"]
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows of --steps steps; the fastest is reported, all are listed")
    ap.add_argument("--compute", default="bf16x3")
    ap.add_argument("--dim", type=int, default=96)
    ap.add_argument("--heads", type=int, default=3)
    ap.add_argument("--small-attn", default="default", choices=["default", "on", "off"],
                    help="the plain small-head attention kernels: per-mode default (on in bf16), wherever they apply, or nowhere")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    sys.exit(sweep(a)) if a.sweep else run(a)


if __name__ == "__main__":
    main()
