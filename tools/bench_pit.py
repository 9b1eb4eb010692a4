"""PiT training-step benchmark: the reference usage (pit.py:221-235: 224-pixel images, patch 14 every 7 pixels: 31 x 31 + 1 = 962 tokens, 1000
classes, dim 256, depth (3, 3, 3), 16 heads of 64, mlp_dim 2048), forward + backward without d(img) on device buffers (vitx_pit_forward_dev /
_backward_dev).  Prints one JSON line per run: ms per step, images per second and, from one more step under the library's profiler
(vitx_pit_profile_begin / _end), the share of every kernel class and of three groups: the tokenizer, Pool, the attention.

    python tools/bench_pit.py [--batch 256] [--steps 4] [--warmup 2] [--compute bf16] [--repeats 2] [--long-attn 0|1] [--pool-stages 0|1]
    python tools/bench_pit.py --ab [--pool-stages 0|1]   # bf16: long_attn on and off alternating, `--rounds` runs each, every run a child
                                                         # process with a time limit
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
GROUPS = {"tokenizer": ("pit_unfold", "pit_embed"), "pool": ("pit_pool_",), "attention": ("attn_",)}
USAGE = dict(image_size=224, patch_size=14, dim=256, num_classes=1000, depth=(3, 3, 3), heads=16, mlp_dim=2048)


def run(a):
    import torch
    from vit_tensorflow import _native as N
    from vit_tensorflow.pit import PiT
    b = a.batch
    m = PiT(**USAGE, compute=a.compute, max_batch=b, seed=0, long_attn=bool(a.long_attn), pool_stages=bool(a.pool_stages))
    h = m._ensure_handle(b, 224, 224)
    img = torch.randn(b, 224, 224, 3, device="cuda")
    dl = torch.randn(b, 1000, device="cuda") / b
    torch.cuda.synchronize()   # the library runs on its own stream
    l = N.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def step():
        N.check(l.vitx_pit_forward_dev(h, ptr(img), b, None))
        N.check(l.vitx_pit_backward_dev(h, ptr(dl), None))

    sync = torch.cuda.synchronize   # the whole device: the handle's own stream included

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
    N.check(l.vitx_pit_profile_begin(h))
    step()
    stats, n = (N.KernelStat * 256)(), C.c_int32()
    N.check(l.vitx_pit_profile_end(h, stats, 256, C.byref(n)))
    rows = {stats[i].name.decode(): (stats[i].total_ms, stats[i].launches) for i in range(n.value) if not stats[i].name.decode().startswith("shape ")}
    total = sum(v[0] for v in rows.values())
    shares = {k: {"ms": round(v[0], 3), "launches": int(v[1]), "share": round(v[0] / total, 4)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1][0])}
    groups = {g: round(sum(v[0] for k, v in rows.items() if k.startswith(pre)) / total, 4) for g, pre in GROUPS.items()}
    print(json.dumps({"workload": "pit_usage_224", "compute": a.compute, "batch": b, "steps": a.steps, "long_attn": int(a.long_attn),
                      "pool_stages": int(a.pool_stages), "tokens": [1 + hh * ww for hh, ww, _ in m.maps_of(224, 224)],
                      "ms_per_step": round(ms, 3), "ms_per_step_runs": [round(t, 3) for t in times], "images_per_s": round(b * 1e3 / ms, 1),
                      "profiled_kernel_ms": round(total, 3), "group_shares": groups, "kernel_classes": shares}), flush=True)


def ab(a):
    """bf16: long_attn=1 and long_attn=0 alternating, `--rounds` times each; stops at the first failure."""
    for _ in range(a.rounds):
        for long_attn in (1, 0):
            cmd = [sys.executable, os.path.abspath(__file__), "--compute", "bf16", "--batch", str(a.batch), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--long-attn", str(long_attn), "--pool-stages", str(a.pool_stages)]
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
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2, help="timed windows of --steps steps; the fastest is reported, all are listed")
    ap.add_argument("--compute", default="bf16")
    ap.add_argument("--long-attn", type=int, default=0, choices=[0, 1], help="the streamed-key attention kernels past 288 tokens")
    ap.add_argument("--pool-stages", type=int, default=0, choices=[0, 1], help="Pool behind every stage but the last (962 -> 257 -> 65 tokens)")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    sys.exit(ab(a)) if a.ab else run(a)


if __name__ == "__main__":
    main()
