"""cct.CCT on the MI355X through the Python drop-in, against fixtures produced by the reference's own cct.py (tests/golden/ref_cct_*.npz) and
against the float64 torch restatement (tests/cct_ref.py) where no fixture exists.

Gates: fp32 and bf16x3 modes, the gate tests/test_gpu_ref_fixtures.py applies to the plain ViT (logits <= 1e-3 abs, every gradient and d(img)
<= 1e-3 of the tensor's max; attention_pool.bias, whose true gradient is 0, <= 1e-6 abs).  bf16 mode: BF16_GATES below."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cct_ref as R  # noqa: E402
import gen_cct_fixtures as G  # noqa: E402
from test_gpu_ref_fixtures import FP32_GRAD_RTOL, FP32_LOGIT_TOL  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

POOL_BIAS = "classifier.attention_pool.bias"
POOL_BIAS_TOL = 1e-6
# bf16 vs float64: (max|dlogit| / max(1, logit std), worst gradient / d(img) error relative to the tensor's max).  Observed on MI355X (DESIGN.md
# section 18), worst case first:
#   logits     4.17e-3 (batch 3 of test_batch_changes_on_one_handle); 3.40e-3 (k147_k3136), 3.13e-3 (cct_bf16 fixture), 2.45e-3 (head_dim 32), 2.11e-3 (n392)
#   gradients  2.32e-2 (classifier.attention_pool.kernel of k147_k3136); every other tensor and case <= 7.0e-3 (classifier.positional_emb, batch 3)
# The gates are 2x the worst observed value of each kind.  The gradient gate is above the small-dataset model's 4.4e-2 because of that one tensor in
# the 2-token shape: with two tokens d(attention_pool.kernel) = dlogit_0 (x_0 - x_1), a difference of two normalised token rows that each carry the
# blocks' bf16 error, so the tensor's own maximum is small against the terms it is the difference of.  At 64 and 392 tokens the same tensor is
# within 6.3e-3.
OBSERVED_BF16 = (4.17e-3, 2.32e-2)
BF16_GATES = (8.4e-3, 4.7e-2)

BF16_SHAPES = {
    # two conv layers, K = 147 and 3136 (64 intermediate planes): 12 x 20 -> 6 x 10 -> 3 x 5 -> 2 x 3 -> 1 x 2 = 2 tokens
    "k147_k3136": dict(img_size=(12, 20), embedding_dim=128, n_conv_layers=2, kernel_size=7, stride=2, num_layers=1, num_heads=2, mlp_ratio=1,
                       num_classes=4, positional_embedding="none"),
    # 392 tokens (the reference usage's count at 224 x 448), more than one wave and no power of two: 28 x 56 -> 14 x 28
    "n392": dict(img_size=(28, 56), embedding_dim=128, n_conv_layers=1, kernel_size=3, stride=1, num_layers=1, num_heads=2, mlp_ratio=1,
                 num_classes=5, positional_embedding="learnable"),
}


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.cct import CCT
    m = CCT(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
    if P is not None:
        m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    return m


def _params(kw, seed=3):
    return R.init_params(R.table_of(kw), seed=seed)


def _inputs(kw, b, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((b, *R.pair(kw["img_size"]), kw.get("n_input_channels", 3))).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    return img, dl


def _errors(m, img, dl, rl, rg, rd):
    logits = m(img, training=False)
    grads, dimg = m.backward(dl, want_dimg=True)
    errs = {n: rel_max_err(grads[n], rg[n]) for n in rg if n != POOL_BIAS and np.abs(rg[n]).max() > 0}
    errs["dimg"] = rel_max_err(dimg, rd)
    return logits, grads, dimg, errs


def _check_fp32(tag, m, img, dl, rl, rg, rd):
    logits, grads, dimg, errs = _errors(m, img, dl, rl, rg, rd)
    le = float(np.abs(logits - rl).max())
    worst = max(errs, key=errs.get)
    print(f"[cct:{tag}] max|dlogit| {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), |d pool bias| {np.abs(grads[POOL_BIAS]).max():.2e}")
    gate(le, FP32_LOGIT_TOL, f"{tag} logits")
    for n, e in errs.items():
        gate(e, FP32_GRAD_RTOL, f"{tag} grad {n}")
    assert np.abs(grads[POOL_BIAS]).max() <= POOL_BIAS_TOL            # softmax is shift-invariant: the true value is 0
    for n in rg:                                                       # (one token: the pooling weight is 1 whatever the logit)
        if n != POOL_BIAS and np.abs(rg[n]).max() == 0:
            assert np.abs(grads[n]).max() <= 1e-6, n
    return logits, grads, dimg


def _check_bf16(tag, m, img, dl, rl, rg, rd):
    logits, grads, dimg, errs = _errors(m, img, dl, rl, rg, rd)
    le = float(np.abs(logits - rl).max()) / max(1.0, float(rl.std()))
    worst = max(errs, key=errs.get)
    print(f"[cct:{tag}] bf16 logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), |d pool bias| {np.abs(grads[POOL_BIAS]).max():.2e}")
    gate(le, BF16_GATES[0], f"{tag} bf16 logits", "cct bf16 logits")
    for n, e in errs.items():
        gate(e, BF16_GATES[1], f"{tag} bf16 grad {n}", "cct bf16 gradients")
    return logits, grads, dimg


def _fixture(case):
    z = G.load(case)
    P = G.params_of(z, case)
    return z, P, z["img"].astype(np.float32), z["dlogits"].astype(np.float32), z["logits"], {n: z["grad/" + n] for n in P}, z["dimg"]


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    z, P, img, dl, rl, rg, rd = _fixture(case)
    _check_fp32(f"{case} {compute}", _model(G.kwargs_of(case), compute, 2, P), img, dl, rl, rg, rd)


def test_bf16_matches_reference_source():
    """The fixture case whose widths the bf16 mode accepts (head_dim 64: the fused attention kernels), against the reference's own numbers."""
    z, P, img, dl, rl, rg, rd = _fixture("cct_bf16")
    _check_bf16("cct_bf16 fixture", _model(G.kwargs_of("cct_bf16"), "bf16", 2, P), img, dl, rl, rg, rd)


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_bf16_matches_restatement(shape):
    kw = BF16_SHAPES[shape]
    P = _params(kw)
    img, dl = _inputs(kw, 2, 1)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    _check_bf16(shape, _model(kw, "bf16", 2, P), img, dl, rl, rg, rd)


def test_sine_matches_restatement():
    """positional_embedding='sine' (the reference cannot run it: cct.py:271-272): the constant table against tests/cct_ref.py:sine_table."""
    kw = {**G.kwargs_of("cct_small"), "positional_embedding": "sine"}
    P = _params(kw)
    assert "classifier.positional_emb" not in P
    img, dl = _inputs(kw, 2, 4)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    m = _model(kw, "fp32", 2, P)
    _check_fp32("sine", m, img, dl, rl, rg, rd)
    prof = m.profile(lambda: (m(img, training=False), m.backward(dl, want_dimg=True)))   # {class: (launches, total_ms)}
    assert prof["cct_im2col"][0] > 0 and prof["cct_conv_gemm"][0] > 0, prof


# kernel edges through a one-block model, fp32, against the restatement.  Conv k3 s1 keeps the extent, so the 3/2 pool sees the image's extents:
# 1, 2, 3, 5, 6 cover both pad parities (odd: 1 + 1, even: 0 + 1) and a single output; the token counts 1, 2, 65 and 392 the sequence pooling
# (one token, fewer than a wave, one past a wave, several rounds of the four waves and no power of two); embedding_dim 6 a channel count that
# is not a multiple of 4 (the scalar pooling kernels).
_EDGE = dict(n_conv_layers=1, kernel_size=3, stride=1, num_layers=1, num_heads=1, mlp_ratio=1, num_classes=3, positional_embedding="none")
EDGES = {
    "pool_1x2_n1": (dict(_EDGE, img_size=(1, 2), embedding_dim=8), 2),
    "pool_3x5": (dict(_EDGE, img_size=(3, 5), embedding_dim=8), 2),
    "pool_6x6_c6": (dict(_EDGE, img_size=6, embedding_dim=6), 3),
    "n2": (dict(_EDGE, img_size=(2, 4), embedding_dim=8), 2),
    "n65": (dict(_EDGE, img_size=(10, 26), embedding_dim=8, positional_embedding="learnable"), 2),
    "n392": (dict(_EDGE, img_size=(28, 56), embedding_dim=8), 1),
    # a batch that is no multiple of the im2col chunk, through both conv layers
    "chunk2_batch3": (dict(_EDGE, img_size=(12, 20), embedding_dim=8, n_conv_layers=2, kernel_size=7, stride=2, conv_chunk=2), 3),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_kernel_edges(edge):
    kw, b = EDGES[edge]
    kw = dict(kw)
    extra = {k: kw.pop(k) for k in ("conv_chunk",) if k in kw}
    P = _params(kw)
    img, dl = _inputs(kw, b, 2)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    m = _model(kw, "fp32", b, P, **extra)
    assert m.sequence_length == R.sequence_length(kw)
    _check_fp32(edge, m, img, dl, rl, rg, rd)


def test_all_negative_conv_output():
    """A positive image under an all-negative kernel: every pre-activation is negative, so every token is exactly 0 and the tokenizer's
    gradients (the kernel's and d(img)) are exactly 0, while the classifier still trains."""
    kw = G.kwargs_of("cct_small")
    P = _params(kw)
    P["tokenizer.conv_layers.0.kernel"] = -np.abs(P["tokenizer.conv_layers.0.kernel"]) - 0.01
    rng = np.random.default_rng(5)
    img = (np.abs(rng.standard_normal((2, 16, 16, 3))) + 0.1).astype(np.float32)
    dl = (rng.standard_normal((2, 5)) / 2).astype(np.float32)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    m = _model(kw, "fp32", 2, P)
    logits = m(img)
    assert np.all(m.read("tokens") == 0)
    grads, dimg = m.backward(dl, want_dimg=True)
    assert np.all(grads["tokenizer.conv_layers.0.kernel"] == 0) and np.all(dimg == 0)
    assert np.abs(rg["tokenizer.conv_layers.0.kernel"]).max() == 0 and np.abs(rd).max() == 0
    gate(float(np.abs(logits - rl).max()), FP32_LOGIT_TOL, "all-negative logits")
    gate(rel_max_err(grads["classifier.fc.kernel"], rg["classifier.fc.kernel"]), FP32_GRAD_RTOL, "all-negative fc.kernel")


def test_batch_changes_on_one_handle():
    """3 -> 1 -> 4 images on one bf16 handle: stale rows of a larger batch, or operand padding zeroed only once, would show in the gradients."""
    kw = G.kwargs_of("cct_bf16")
    P = _params(kw)
    m = _model(kw, "bf16", 4, P)
    for b in (3, 1, 4):
        img, dl = _inputs(kw, b, 10 + b)
        rl, rg, rd = R.forward_backward(kw, P, img, dl)
        _check_bf16(f"batch {b}", m, img, dl, rl, rg, rd)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_two_runs_give_the_same_bits(compute):
    kw = G.kwargs_of("cct_bf16")
    P = _params(kw)
    img, dl = _inputs(kw, 3, 8)
    runs = []
    for _ in range(2):
        m = _model(kw, compute, 3, P, conv_chunk=2)
        logits = m(img)
        grads, dimg = m.backward(dl, want_dimg=True)
        runs.append((logits, grads, dimg))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for n in runs[0][1]:
        assert np.array_equal(runs[0][1][n], runs[1][1][n]), n
    assert np.abs(runs[0][1]["tokenizer.conv_layers.0.kernel"]).max() > 0 and np.abs(runs[0][1]["classifier.attention_pool.kernel"]).max() > 0


def test_flag_does_not_leak_into_a_plain_vit():
    from vit_tensorflow import ViT as PlainViT
    kw = dict(image_size=16, patch_size=4, num_classes=5, dim=64, depth=1, heads=4, dim_head=16, mlp_dim=64)
    img = np.random.default_rng(12).standard_normal((2, 16, 16, 3)).astype(np.float32)
    outs = []
    for step in range(2):
        outs.append(PlainViT(**kw, compute="bf16", max_batch=2, seed=3)(img, training=False))
        if step == 0:
            ckw = G.kwargs_of("cct_bf16")
            m = _model(ckw, "bf16", 2, _params(ckw))
            m(img)
            m.backward(np.ones((2, 5), np.float32))
    assert np.array_equal(outs[0], outs[1])


def test_bf16_generic_attention_head_width():
    """head_dim 32 in the bf16 mode: not the fused kernels' width, so the existing generic attention path runs under the CCT block form."""
    kw = {**G.kwargs_of("cct_bf16"), "embedding_dim": 64, "num_heads": 2, "num_layers": 1}
    P = _params(kw)
    img, dl = _inputs(kw, 2, 6)
    rl, rg, rd = R.forward_backward(kw, P, img, dl)
    _check_bf16("head_dim 32", _model(kw, "bf16", 2, P), img, dl, rl, rg, rd)


def test_cct_block_engine_refuses_the_image_entry_points():
    """A vitx_config.cct_block handle serves the transformer entry points only: the image entry points (forward, embed) are unsupported."""
    import ctypes as C
    from vit_tensorflow import _native as N
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h = c.image_w = 16
    c.patch_h = c.patch_w = 4
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 3, 5, 32, 1, 2, 16, 32
    c.pool, c.ln_eps, c.max_batch, c.cct_block = N.POOL_CLS, 1e-3, 1, 1
    l, h = N.lib(), C.c_void_p()
    N.check(l.vitx_create(C.byref(c), C.byref(h)))
    try:
        img, out = np.zeros((1, 16, 16, 3), np.float32), np.zeros(17 * 32, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert l.vitx_forward(h, p(img), 1, 16, 16, 0, 0, p(out)) == N.ERR_UNSUPPORTED
        assert l.vitx_embed_forward(h, p(img), 1, 16, 16, p(out)) == N.ERR_UNSUPPORTED
    finally:
        l.vitx_destroy(h)


def test_training_true_is_refused():
    m = _model(G.kwargs_of("cct_1tok"), "fp32", 1)
    img = np.zeros((1, 4, 4, 3), np.float32)
    with pytest.raises(NotImplementedError, match="dropout on the attention probabilities.*stochastic depth"):
        m(img, training=True)
    assert m(img).shape == (1, 3)
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()
