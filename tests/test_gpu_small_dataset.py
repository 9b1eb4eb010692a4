"""vit_for_small_dataset.ViT / SPT on the MI355X through the Python drop-in, against fixtures produced by the reference's own
vit_for_small_dataset.py (tests/golden/ref_sd_*.npz) and against the float64 torch restatement (tests/small_dataset_ref.py) where no fixture
exists.

Gates: fp32 and bf16x3 modes, the gate tests/test_gpu_ref_fixtures.py applies to the plain ViT (logits <= 1e-3 abs, every gradient and d(img)
<= 1e-3 of the tensor's max).  bf16 mode: BF16_GATES below."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import small_dataset_ref as R  # noqa: E402
import gen_small_dataset_fixtures as G  # noqa: E402
from test_gpu_ref_fixtures import FP32_GRAD_RTOL, FP32_LOGIT_TOL  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

# The engine's bf16 mode needs dim, heads * dim_head and mlp_dim in multiples of 64, which none of the four fixture cases is: the bf16 checks
# run the fixture cases' structure at such widths against the float64 restatement (which the fixtures pin).
BF16_CASES = {
    "sd_small": dict(image_size=16, patch_size=4, num_classes=5, dim=64, depth=2, heads=4, dim_head=16, mlp_dim=64, pool="cls"),
    "sd_rect_mean": dict(image_size=(8, 24), patch_size=8, num_classes=4, dim=64, depth=1, heads=2, dim_head=32, mlp_dim=64, pool="mean"),
    "sd_2tok": dict(image_size=4, patch_size=4, num_classes=3, dim=64, depth=1, heads=4, dim_head=16, mlp_dim=64, pool="cls"),
    "sd_dh64": dict(image_size=32, patch_size=4, num_classes=6, dim=64, depth=1, heads=2, dim_head=64, mlp_dim=64, pool="cls"),
}
# bf16 vs float64: (max|dlogit| / max(1, logit std), worst gradient / d(img) error relative to the tensor's max).  Observed on MI355X (DESIGN.md
# section 17): logits 1.05e-2 (sd_bf16 against the reference's fixture), gradients 2.45e-2 (transformer.0.attn.temperature at batch 3 of
# test_batch_changes_on_one_handle; every other tensor <= 1.8e-2).  The gates are 2.1x and 1.8x these: a little tighter than the project's 2x
# for the gradients.
BF16_GATES = (2.2e-2, 4.4e-2)


def _load(case):
    return np.load(os.path.join(ROOT, "tests", "golden", f"ref_{case}.npz"))


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.vit_for_small_dataset import ViT
    m = ViT(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
    if P is not None:
        m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    return m


def _params(kw, seed=3):
    from vit_tensorflow.vit_for_small_dataset import ViT
    return R.init_params([(w.name, w.shape, 0) for w in ViT(**kw).weights], seed=seed, dim_head=kw.get("dim_head", 64))


def _size(kw):
    s = kw["image_size"]
    return s if isinstance(s, tuple) else (s, s)


def _check_fp32(tag, m, img, dl, rl, rg, rd, training=False):
    logits = m(img, training=training, seed=5)
    grads, dimg = m.backward(dl, want_dimg=True)
    le = float(np.abs(logits - rl).max())
    errs = {n: rel_max_err(grads[n], rg[n]) for n in rg if np.abs(rg[n]).max() > 0}
    errs["dimg"] = rel_max_err(dimg, rd)
    worst = max(errs, key=errs.get)
    print(f"[sd:{tag}] max|dlogit| {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}); temperature " +
          ", ".join(f"{errs[n]:.2e}" for n in errs if n.endswith("temperature")))
    gate(le, FP32_LOGIT_TOL, f"{tag} logits")
    for n, e in errs.items():
        gate(e, FP32_GRAD_RTOL, f"{tag} grad {n}")
    for n in rg:                                  # (a 2-token model: the temperature's gradient is exactly zero)
        if np.abs(rg[n]).max() == 0:
            assert np.abs(grads[n]).max() <= 1e-6, n
    return logits, grads, dimg


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    z = _load(case)
    P = G.params_of(z, case)
    m = _model(G.kwargs_of(case), compute, 2, P)
    _check_fp32(f"{case} {compute}", m, z["img"].astype(np.float32), z["dlogits"].astype(np.float32), z["logits"],
                {n: z["grad/" + n] for n in P}, z["dimg"], training=True)       # dropout rates are 0 in the fixtures


def test_bf16_matches_reference_source():
    """The one fixture case whose widths the bf16 mode accepts, against the reference's own numbers."""
    case = "sd_bf16"
    z = _load(case)
    P = G.params_of(z, case)
    m = _model(G.kwargs_of(case), "bf16", 2, P)
    logits = m(z["img"].astype(np.float32), training=True)
    grads, dimg = m.backward(z["dlogits"].astype(np.float32), want_dimg=True)
    le = float(np.abs(logits - z["logits"]).max()) / max(1.0, float(z["logits"].std()))
    errs = {n: rel_max_err(grads[n], z["grad/" + n]) for n in P}
    errs["dimg"] = rel_max_err(dimg, z["dimg"])
    worst = max(errs, key=errs.get)
    print(f"[sd:{case} fixture] bf16 logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}); temperature " +
          ", ".join(f"{errs[n]:.2e}" for n in errs if n.endswith("temperature")))
    gate(le, BF16_GATES[0], f"{case} bf16 logits", "small_dataset bf16 logits")
    for n, e in errs.items():
        gate(e, BF16_GATES[1], f"{case} bf16 grad {n}", "small_dataset bf16 gradients")


def test_spt_alone_beyond_the_attention_limit():
    """SPT has no attention: 1024 patches (far past the LSA kernels' 288 tokens) tokenize."""
    import torch
    from vit_tensorflow.vit_for_small_dataset import SPT
    rng = np.random.default_rng(5)
    img = rng.standard_normal((1, 64, 64, 3)).astype(np.float32)
    s = SPT(dim=16, patch_size=2, seed=2)
    w = s.weights
    P = {k: torch.tensor(a.astype(np.float64)) for k, a in zip(("patch_embedding.norm.gamma", "patch_embedding.norm.beta", "patch_embedding.kernel",
                                                                 "patch_embedding.bias"), w)}
    got = s(img)
    assert got.shape == (1, 1024, 16)
    gate(rel_max_err(got, R.spt(torch.tensor(img.astype(np.float64)), P, 2).numpy()), FP32_GRAD_RTOL, "SPT tokens, 1024 patches")


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_bf16_matches_restatement(case):
    kw = BF16_CASES[case]
    P = _params(kw)
    rng = np.random.default_rng(1)
    img = rng.standard_normal((2, *_size(kw), 3)).astype(np.float32)
    dl = (rng.standard_normal((2, kw["num_classes"])) / 2).astype(np.float32)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    m = _model(kw, "bf16", 2, P)
    logits = m(img, training=False)
    grads, dimg = m.backward(dl, want_dimg=True)
    le = float(np.abs(logits - rl).max()) / max(1.0, float(rl.std()))
    errs = {n: rel_max_err(grads[n], rg[n]) for n in rg if np.abs(rg[n]).max() > 0}
    errs["dimg"] = rel_max_err(dimg, rd)
    worst = max(errs, key=errs.get)
    print(f"[sd:{case}] bf16 logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}); temperature " +
          ", ".join(f"{errs[n]:.2e}" for n in errs if n.endswith("temperature")))
    gate(le, BF16_GATES[0], f"{case} bf16 logits", "small_dataset bf16 logits")
    for n, e in errs.items():
        gate(e, BF16_GATES[1], f"{case} bf16 grad {n}", "small_dataset bf16 gradients")


# kernel edges through a depth-1 model, fp32, against the restatement: 2 tokens; one past the 64-row tile; 257 tokens at dim_head 64 (forward
# and d(q) pass 4 rows per wave, d(k) / d(v) pass 2); 288 tokens at dim_head 64, the advertised limit (forward and d(q) pass 2 rows per wave,
# d(k) / d(v) pass 1); dim_head 32 (two lane groups in the second product)
EDGES = {
    "n288_dh64": (dict(image_size=(28, 164), patch_size=4, num_classes=3, dim=16, depth=1, heads=1, dim_head=64, mlp_dim=16), 1),
    "n2": (dict(image_size=4, patch_size=4, num_classes=3, dim=16, depth=1, heads=2, dim_head=16, mlp_dim=16), 2),
    "n65": (dict(image_size=32, patch_size=4, num_classes=3, dim=16, depth=1, heads=1, dim_head=16, mlp_dim=16), 2),
    "n257_dh64": (dict(image_size=64, patch_size=4, num_classes=3, dim=16, depth=1, heads=1, dim_head=64, mlp_dim=16), 1),
    "dh32_n10": (dict(image_size=12, patch_size=4, num_classes=3, dim=24, depth=1, heads=3, dim_head=32, mlp_dim=16, pool="mean"), 3),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_kernel_edges(edge):
    kw, b = EDGES[edge]
    P = _params(kw)
    rng = np.random.default_rng(2)
    img = rng.standard_normal((b, *_size(kw), 3)).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    _check_fp32(edge, _model(kw, "fp32", b, P), img, dl, rl, rg, rd)


def test_spt_alone_reads_zero_fill_at_the_border():
    """SPT(dim, patch_size)(img) against the restatement; the last row and column are 1e3, everything else small: a wrapped-around read (roll
    without the zero fill) would put 1e3 into the first row's / column's shifted copies."""
    import torch
    from vit_tensorflow.vit_for_small_dataset import SPT
    rng = np.random.default_rng(4)
    img = (0.01 * rng.standard_normal((2, 8, 12, 3))).astype(np.float32)
    img[:, -1, :, :] = 1e3
    img[:, :, -1, :] = 1e3
    s = SPT(dim=24, patch_size=4, seed=1)
    feat = 5 * 4 * 4 * 3
    w = [1.0 + 0.2 * rng.standard_normal(feat), 0.2 * rng.standard_normal(feat), rng.standard_normal((feat, 24)) / np.sqrt(feat), 0.2 * rng.standard_normal(24)]
    w = [a.astype(np.float32) for a in w]
    s.set_weights(w)
    got = s(img)
    P = {"patch_embedding.norm.gamma": w[0], "patch_embedding.norm.beta": w[1], "patch_embedding.kernel": w[2], "patch_embedding.bias": w[3]}
    P = {k: torch.tensor(v.astype(np.float64)) for k, v in P.items()}
    want = R.spt(torch.tensor(img.astype(np.float64)), P, 4).numpy()
    assert got.shape == (2, 6, 24)
    # the unfolded rows themselves: the first patch's shifted copies hold the zero fill, not the 1e3 of the far border
    rows = R.shifted(torch.tensor(img.astype(np.float64))).numpy()
    assert np.all(rows[:, :, 0, 3:6] == 0) and np.all(rows[:, 0, :, 9:12] == 0)
    gate(rel_max_err(got, want), FP32_GRAD_RTOL, "SPT tokens")
    assert [a.shape for a in s.weights] == [(feat,), (feat,), (feat, 24), (24,)]


def test_diagonal_is_masked():
    """2 tokens: with the diagonal masked each token's attention output is the OTHER token's v exactly.  Another image changes q, k and v of the
    patch token only, so the patch token's own output row (= v of the cls token) must not move at all, while the cls token's row does."""
    kw = dict(image_size=4, patch_size=4, num_classes=3, dim=16, depth=1, heads=2, dim_head=16, mlp_dim=16)
    m = _model(kw, "fp32", 1, _params(kw))
    rng = np.random.default_rng(6)
    outs = []
    for _ in range(2):
        m(rng.standard_normal((1, 4, 4, 3)).astype(np.float32), training=False)
        outs.append((m.debug_read("attn_out", 0).reshape(2, 32), m.debug_read("qkv", 0).reshape(2, 3, 32)))
    (o_a, qkv_a), (o_b, qkv_b) = outs
    assert np.abs(qkv_a[1] - qkv_b[1]).max() > 1e-3 and np.array_equal(qkv_a[0], qkv_b[0])
    assert np.array_equal(o_a[1], o_b[1]) and np.array_equal(o_a[1], qkv_a[0, 2])    # patch row = v of the cls token, bit for bit
    assert np.array_equal(o_a[0], qkv_a[1, 2]) and np.abs(o_a[0] - o_b[0]).max() > 1e-3


def test_smaller_image():
    """H = W = 8 on a handle built for 16: the position embedding is sliced and the shifts' zero fill sits at the smaller image's border."""
    z = _load("sd_small")
    P = G.params_of(z, "sd_small")
    kw = G.kwargs_of("sd_small")
    rng = np.random.default_rng(3)
    img = rng.standard_normal((3, 8, 8, 3)).astype(np.float32)
    dl = (rng.standard_normal((3, kw["num_classes"])) / 3).astype(np.float32)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    _check_fp32("8px on 16px", _model(kw, "fp32", 3, P), img, dl, rl, rg, rd)


def test_batch_changes_on_one_handle():
    kw = BF16_CASES["sd_small"]
    P = _params(kw)
    m = _model(kw, "bf16", 3, P)
    rng = np.random.default_rng(11)
    for b in (3, 2, 3):
        img = rng.standard_normal((b, 16, 16, 3)).astype(np.float32)
        dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
        rl, rg, rd = R.forward_backward(kw, P, img, dl)
        logits = m(img, training=False)
        grads, dimg = m.backward(dl, want_dimg=True)
        gate(float(np.abs(logits - rl).max()) / max(1.0, float(rl.std())), BF16_GATES[0], f"batch {b} logits", "small_dataset bf16 logits")
        for n in rg:
            gate(rel_max_err(grads[n], rg[n]), BF16_GATES[1], f"batch {b} grad {n}", "small_dataset bf16 gradients")
        gate(rel_max_err(dimg, rd), BF16_GATES[1], f"batch {b} dimg", "small_dataset bf16 gradients")


def test_dropout_seeds_and_eval_mode():
    z = _load("sd_small")
    P = G.params_of(z, "sd_small")
    kw = {**G.kwargs_of("sd_small"), "dropout": 0.1, "emb_dropout": 0.1}
    m, m0 = _model(kw, "fp32", 2, P), _model(G.kwargs_of("sd_small"), "fp32", 2, P)
    img = z["img"].astype(np.float32)
    ev = m(img, training=False, seed=1)
    np.testing.assert_allclose(ev, m0(img, training=True, seed=1), rtol=0, atol=1e-5)   # dropout off == rate 0
    a, b_ = m(img, training=True, seed=7), m(img, training=True, seed=7)
    assert np.array_equal(a, b_)
    c = m(img, training=True, seed=8)
    assert np.abs(a - c).max() > 1e-4 and np.abs(a - ev).max() > 1e-4


def test_dropout_backward_replays_masks():
    """fp32, dropout = emb_dropout = 0.1, one seed: the directional derivative from backward matches a central difference of the same
    masked forward."""
    z = _load("sd_small")
    P = G.params_of(z, "sd_small")
    kw = {**G.kwargs_of("sd_small"), "dropout": 0.1, "emb_dropout": 0.1}
    m = _model(kw, "fp32", 2, P)
    img, dl = z["img"].astype(np.float32), z["dlogits"]
    m(img, training=True, seed=42)
    grads, _ = m.backward(dl.astype(np.float32))
    rng = np.random.default_rng(9)
    V = {n: rng.standard_normal(np.shape(p)) * (np.abs(p).mean() + 0.05) for n, p in P.items()}   # about the tensor's own scale
    analytic = sum(float((grads[n].astype(np.float64) * V[n]).sum()) for n in P)
    eps = 2e-3

    def loss(sign):
        m.load_state_dict({n: (P[n] + sign * eps * V[n]).astype(np.float32) for n in P})
        return float((m(img, training=True, seed=42).astype(np.float64) * dl).sum())

    numeric = (loss(1) - loss(-1)) / (2 * eps)
    print(f"[sd:dropout fd] analytic {analytic:.6e} numeric {numeric:.6e}")
    assert abs(analytic - numeric) <= 2e-2 * max(1.0, abs(analytic)), (analytic, numeric)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_two_runs_give_the_same_bits(compute):
    kw = BF16_CASES["sd_dh64"]
    P = _params(kw)
    rng = np.random.default_rng(8)
    img = rng.standard_normal((2, 32, 32, 3)).astype(np.float32)
    dl = (rng.standard_normal((2, kw["num_classes"])) / 2).astype(np.float32)
    runs = []
    for _ in range(2):
        m = _model(kw, compute, 2, P)
        logits = m(img, training=False)
        grads, dimg = m.backward(dl, want_dimg=True)
        runs.append((logits, grads, dimg))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for n in runs[0][1]:
        assert np.array_equal(runs[0][1][n], runs[1][1][n]), n
    assert np.abs(runs[0][1]["transformer.0.attn.temperature"]).max() > 0 and np.abs(runs[0][1]["patch_embedding.norm.gamma"]).max() > 0


def test_flag_does_not_leak_into_a_plain_vit():
    from vit_tensorflow import ViT as PlainViT
    kw = dict(image_size=16, patch_size=4, num_classes=5, dim=64, depth=1, heads=4, dim_head=16, mlp_dim=64)
    img = np.random.default_rng(12).standard_normal((2, 16, 16, 3)).astype(np.float32)
    outs = []
    for step in range(2):
        outs.append(PlainViT(**kw, compute="bf16", max_batch=2, seed=3)(img, training=False))
        if step == 0:
            m = _model(kw, "bf16", 2, _params(kw))
            m(img, training=False)
            m.backward(np.ones((2, 5), np.float32))
    assert np.array_equal(outs[0], outs[1])
