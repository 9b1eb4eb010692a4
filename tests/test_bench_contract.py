"""bench.py's contract with the driver: the FLOP model behind `value` / `roofline` (CPU tier) and the one-line JSON schema of a
real run, plain and with --full (GPU tier, small batch so that it finishes in seconds)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("vitx_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flop_model_matches_the_survey_figures():
    b = _bench_module()
    # ViT-B/16 224 = 105.383 GFLOP fwd+bwd per image, ViT-L/16 224 = 369.328, README cfg1 = 21.155
    assert abs(b.flops_per_image(b.WORKLOADS["vit_b16_224"]) / 1e9 - 105.383) < 5e-3
    assert abs(b.flops_per_image(b.WORKLOADS["vit_l16_224"]) / 1e9 - 369.328) < 5e-3
    assert abs(b.flops_per_image(b.WORKLOADS["vit_readme_256"]) / 1e9 - 21.155) < 5e-3
    assert b.MFMA_BF16_PEAK == 2516.6e12 and b.HBM_PEAK == 8.0e12
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert "images/sec" in base["metric"]


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "8", "--cpu-seconds", "1", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "images/sec" and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2516.6 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_repeatable_outputs(tmp_path):
    """Without --full the line carries the headline figure only (no per-kernel timing, no CPU baseline); --dump-outputs writes the last
    timed step's logits and gradient sample as float32, a second run with the same arguments writes the same arrays, and both are
    what the step computes: the same step run here, with the logits taken from vitx_forward_dev's own output, gives them again."""
    dumps = []
    for run in ("a", "b"):
        d_out = tmp_path / run
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                              "--dump-outputs", str(d_out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, out.stdout
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "bf16" and d["unit"] == "images/sec"
        for k in ("roofline", "kernel_classes", "cpu_baseline"):
            assert k not in d, k
        assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
        logits, grads = np.load(d_out / "logits.npy"), np.load(d_out / "grads_sample.npy")
        assert logits.dtype == np.float32 and logits.shape == (8, 1000) and np.isfinite(logits).all() and np.abs(logits).max() > 0
        assert grads.dtype == np.float32 and grads.ndim == 1 and 0.9 * (1 << 22) < grads.size <= 1 << 22 and np.isfinite(grads).all()
        assert np.abs(grads).max() > 0
        dumps.append((logits, grads))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])

    # the step of bench.py at the same seeds (weights seed 1, inputs from a device generator seeded 1234), once, in this process
    import ctypes as C
    import torch
    from vit_tensorflow import ViT, _native as N
    bm = _bench_module()
    kw = bm.WORKLOADS["vit_b16_224"]
    dev = torch.device("cuda", 0)
    m = ViT(**kw, compute="bf16", max_batch=8, device=0, seed=1)
    m.build((8,))
    g = torch.Generator(device=dev).manual_seed(1234)
    img = torch.randn(8, 224, 224, 3, device=dev, generator=g)
    labels = torch.randint(0, kw["num_classes"], (8,), device=dev, generator=g, dtype=torch.int32)
    logits_t = torch.full((8, kw["num_classes"]), float("nan"), device=dev)
    torch.cuda.synchronize()
    lib, h = N.lib(), m._handle
    N.check(lib.vitx_params_changed(h))
    N.check(lib.vitx_forward_dev(h, C.c_void_p(img.data_ptr()), 8, 224, 224, 0, 0, C.c_void_p(logits_t.data_ptr())))
    N.check(lib.vitx_ce_loss_grad_dev(h, C.c_void_p(labels.data_ptr()), 1.0 / 8, None))
    N.check(lib.vitx_backward_dev(h, None, None))
    N.check(lib.vitx_sync(h))
    torch.cuda.synchronize()
    grads = np.empty(m._n, dtype=np.float32)
    N.check(lib.vitx_get_grads(h, grads.ctypes.data_as(C.c_void_p), m._n))
    idx = bm.grad_sample_index(m._n)
    want_logits, want_grads = logits_t.cpu().numpy(), (grads if idx is None else grads[idx])
    logits, gsample = dumps[0]
    assert want_grads.shape == gsample.shape
    assert np.abs(logits - want_logits).max() <= 1e-5 * np.abs(want_logits).max(), np.abs(logits - want_logits).max()
    assert np.abs(gsample - want_grads).max() <= 1e-5 * np.abs(want_grads).max(), np.abs(gsample - want_grads).max()


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["native", "torch", "native-unavailable"])
def test_bench_data_parallel_path_on_a_group_of_one(impl):
    """The N > 1 code path of bench.py (rendezvous, weight broadcast, the gradient exchange overlapped with the backward pass, the join) on the one GPU
    a test box has: VITX_FORCE_DP=1 forms an RCCL group of one.  native = the library's own bucketed exchange (csrc/comm.hip), torch = GradSync."""
    env = dict(os.environ, VITX_FORCE_DP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    if impl == "native-unavailable":   # the native exchange reports an error at start-up: every rank falls back to the torch exchange (own NCCL group)
        env["VITX_BENCH_SIMULATE_NATIVE_FAILURE"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "8", "--no-cpu-baseline", "--no-profile",
                          "--bucket-mb", "16", "--dp-impl", "torch" if impl == "torch" else "native"], capture_output=True, text=True, timeout=600, cwd=ROOT,
                         env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak"
    if impl == "native-unavailable":
        assert "unavailable" in d["config"]["dp_impl"] and "exchange" not in d["config"]
    if impl == "native":
        ex = d["config"]["exchange"]
        assert ex["buckets"] >= 2 and 1 <= ex["sent_during_backward"] <= ex["buckets"], ex   # 346 MB of gradients in 16-MiB buckets, most sent early
