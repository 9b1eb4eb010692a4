"""The attention path of a block: its backward runs the kernel family its forward ran (csrc/engine.hip: select_attn_path, attn_forward,
attn_backward).

One case per path and per q / k / v layout that reaches it, taken from the test modules that own them.  Each case profiles one forward and,
separately, its backward, and reads the launch counts of the profiler classes `attn_<family>_fwd` / `attn_<family>_bwd`:
  * the class of the path the case is there for appears in the forward,
  * every family with both classes launches its `_bwd` exactly as often in the backward as its `_fwd` in the forward,
  * no `attn_*_bwd` class appears whose `_fwd` did not.
The materialised path books no class of its own name: it shows as its batched products and head-axis kernels (MATERIALISED).
"""
import os
import re

import numpy as np
import pytest

import test_gpu_crossformer as CF
import test_gpu_cvt as CV
import test_gpu_long_attn as LA
import test_gpu_nest as NE
import test_gpu_regionvit as RV
import test_gpu_small_dataset as SD
import test_gpu_twins as TW
from util import CONFIGS, make_engine_model
from vit_tensorflow import ViT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
SEED = 7
FAMILIES = ("lsa", "window", "small", "x3", "bf16", "stream", "fewkey", "manykey", "deepvit_fused", "cait_fused")
MATERIALISED = ("attn_generic", "attn_bgemm", "attn_headchain", "attn_deepvit_fused_fwd", "attn_cait_fused_fwd")
# 2 x 2 patches and the class token: 5 tokens of dim_head 64
VIT5 = dict(image_size=32, patch_size=16, num_classes=10, dim=128, depth=2, heads=2, mlp_dim=256, dim_head=64)


def _families_with_both_classes():
    with open(os.path.join(ROOT, "vit-tensorflow_amd", "csrc", "engine.hip")) as f:
        src = f.read()
    return [x for x in FAMILIES if f'"attn_{x}_fwd"' in src and f'"attn_{x}_bwd"' in src]


def _rand(hw, num_classes):
    rng = np.random.default_rng(SEED)
    img = rng.standard_normal((B, hw[0], hw[1], 3)).astype(np.float32)
    return img, (rng.standard_normal((B, num_classes)) / B).astype(np.float32)


def _vit(compute, pool, kw=VIT5, **extra):
    m = ViT(**dict(kw, pool=pool), compute=compute, max_batch=B, seed=0, **extra)
    s = kw["image_size"]
    return (m,) + _rand(s if isinstance(s, tuple) else (s, s), kw["num_classes"])


def _n289(long_attn):
    c = LA.CASES["n289"]
    kw = LA._kw(**c)
    return _vit("bf16", kw.pop("pool"), kw, long_attn=long_attn)


def _small_dataset(case, compute):
    kw = SD.BF16_CASES[case]
    return (SD._model(kw, compute, B),) + _rand(SD._size(kw), kw["num_classes"])


def _nest(compute):   # (the fp32 modes take the small-head kernels only when asked to)
    kw = NE.BF16_SHAPES["dh32"]
    return (NE._model(kw, compute, B, small_attn=True),) + NE._inputs(kw, B, SEED)


def _fixture(mod, case, compute):
    kw, P, img, dl = mod._fixture(case)[:4]
    return mod._model(kw, compute, B, P, image_size=mod.G.image_of(case)), img[:B], dl[:B]


def _shape(mod, shape, **extra):
    hw, kw = mod.BF16_SHAPES[shape]
    return (mod._model(kw, "bf16", B, image_size=hw, **extra),) + mod._inputs(kw, hw, B, SEED)


def _golden(name, compute):
    kw = CONFIGS[name][1]
    return (make_engine_model(name, compute, B),) + _rand((kw["image_size"],) * 2, kw["num_classes"])


# id: (family whose _fwd class the forward must show, or None for the materialised path; builder of (model, images, d(logits)); environment)
CASES = {
    "fused": ("bf16", lambda: _vit("bf16", "mean"), {}),
    "fused_cls_rows": ("bf16", lambda: _vit("bf16", "cls"), {}),
    "fused_cls_rows_off": ("bf16", lambda: _vit("bf16", "cls"), {"VITX_LAST_BLOCK_FULL": "1"}),
    "stream_n289": ("stream", lambda: _n289(True), {}),
    "generic_n289": (None, lambda: _n289(False), {}),
    "x3": ("x3", lambda: _vit("bf16x3", "mean"), {}),
    "lsa_2tok_bf16": ("lsa", lambda: _small_dataset("sd_2tok", "bf16"), {}),
    "lsa_2tok_fp32": ("lsa", lambda: _small_dataset("sd_2tok", "fp32"), {}),
    "lsa_dh64_bf16": ("lsa", lambda: _small_dataset("sd_dh64", "bf16"), {}),
    "lsa_dh64_fp32": ("lsa", lambda: _small_dataset("sd_dh64", "fp32"), {}),
    "small_bf16": ("small", lambda: _nest("bf16"), {}),
    "small_fp32": ("small", lambda: _nest("fp32"), {}),
    "window_bias": ("window", lambda: _fixture(CF, "cf_bf16", "bf16"), {}),
    "small_bias_fp32": ("small", lambda: _fixture(CF, "cf_bf16", "fp32"), {}),
    "window_head_bias": ("window", lambda: _fixture(RV, RV.BF16_CASES[0], "bf16"), {}),
    "fewkey": ("fewkey", lambda: _shape(TW, "m16_9_4_1"), {}),
    "generic_global_k": (None, lambda: _shape(TW, "n324_m81"), {}),
    "manykey": ("manykey", lambda: _shape(CV, "q65_k65"), {}),
    "generic_fp32": (None, lambda: _vit("fp32", "mean"), {}),
    "generic_deepvit_fp32": (None, lambda: _golden("deepvit_small", "fp32"), {}),
    "generic_deepvit_bf16": (None, lambda: _golden("deepvit_small", "bf16"), {}),
    "generic_cait_fp32": (None, lambda: _golden("cait_small", "fp32"), {}),
    "generic_cait_bf16": (None, lambda: _golden("cait_small", "bf16"), {}),
}


def profile_passes(m, img, dl):
    """({class: launches} of one forward, of its backward)"""
    fwd = m.profile(lambda: m(img))
    bwd = m.profile(lambda: m.backward(dl))
    return {k: v[0] for k, v in fwd.items()}, {k: v[0] for k, v in bwd.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_backward_takes_the_forwards_path(case, monkeypatch):
    family, build, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fwd, bwd = profile_passes(*build())
    counts = {x: (fwd.get(f"attn_{x}_fwd", 0), bwd.get(f"attn_{x}_bwd", 0)) for x in FAMILIES}
    print(f"[attn_paths:{case}] (forward, backward) launches: " + ", ".join(f"{x} {c}" for x, c in counts.items() if any(c)) +
          f"; materialised classes in the forward: {sorted(k for k in fwd if k.startswith(MATERIALISED))}")
    if family is None:
        assert any(k.startswith(MATERIALISED) for k in fwd), fwd
    else:
        assert fwd.get(f"attn_{family}_fwd", 0) >= 1, fwd
    for x in _families_with_both_classes():
        assert counts[x][1] == counts[x][0], (x, counts[x], fwd, bwd)
    for k in bwd:
        mt = re.fullmatch(r"attn_(\w+)_bwd", k)
        if mt:
            assert fwd.get(f"attn_{mt.group(1)}_fwd", 0) >= 1, (k, fwd, bwd)
