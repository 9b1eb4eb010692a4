"""nest.NesT on the MI355X through the Python drop-in, against fixtures produced by the reference's own nest.py (tests/golden/ref_nest_*.npz) and
against the float64 torch restatement (tests/nest_ref.py) where no fixture exists.

Gates: fp32 and bf16x3 modes, the gate tests/test_gpu_ref_fixtures.py applies to the plain ViT (logits <= 1e-3 abs, every gradient and d(img)
<= 1e-3 of the tensor's max).  The last level's pos_emb has a true gradient of exactly zero (tests/test_nest_oracle.py); it is gated absolutely:
fp32 / bf16x3 at 4x the magnitude a float32 evaluation of tests/nest_ref.py gives it on the CPU (the noise of an honest fp32 evaluation, computed
here), bf16 at 2x the worst value observed on the MI355X.  bf16 mode: BF16_GATES below."""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nest_ref as R  # noqa: E402
import gen_nest_fixtures as G  # noqa: E402
from test_gpu_ref_fixtures import FP32_GRAD_RTOL, FP32_LOGIT_TOL  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

# bf16 vs float64: (max|dlogit| / max(1, logit std), worst gradient / d(img) error relative to the tensor's max, max |d(last pos_emb)|).
# Observed on MI355X, as (logits, worst gradient and its tensor, |d last pos_emb|):
#   nest_bf16 fixture (dim_head 64, attn_bf16)      4.353e-3  3.703e-2 (nest_layers.0.aggregate.conv.kernel)  5.029e-8
#   dh32 (4 tokens, three levels)       small-head  6.763e-3  1.669e-1 (dimg)                                 1.229e-7
#                                       generic     4.668e-3  9.956e-2 (dimg)                                 1.155e-7
#   dh32_196tok (196 tokens, two levels) small-head 4.755e-3  1.112e-1 (dimg)                                 6.286e-9
#                                       generic     4.663e-3  1.094e-1 (dimg)                                 1.164e-8
# The gates are 2x the worst observed value of each kind.  The gradient gate is far above the other models'; the worst tensor is d(img) in both
# restatement shapes, and it is as large on the materialised attention path, whose kernels this change does not touch (9.96e-2 / 1.09e-1), so it
# is not the small-head kernels' error.  A likely source, not isolated: the 3/2 max-pool routes each window's gradient to ONE input, and a bf16
# run that picks another tap of a near-tie moves that window's whole gradient to another pixel.
OBSERVED_BF16 = (6.763e-3, 1.669e-1, 1.229e-7)
BF16_GATES = (1.36e-2, 3.34e-1, 2.5e-7)

BF16_SHAPES = {
    # dim_head 32 at every level, 4 tokens per block, three levels
    "dh32": dict(image_size=16, patch_size=2, num_classes=5, dim=64, heads=2, num_hierarchies=3, block_repeats=1, mlp_mult=1),
    # dim_head 32, 196 tokens per block (the usage's count)
    "dh32_196tok": dict(image_size=28, patch_size=1, num_classes=4, dim=64, heads=2, num_hierarchies=2, block_repeats=1, mlp_mult=1),
}


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.nest import NesT
    m = NesT(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
    if P is not None:
        m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    return m


@contextlib.contextmanager
def _generic_attention():
    """VITX_GENERIC_ATTN=1 around the construction of a handle: the materialised attention path, i.e. what runs without the small-head kernels."""
    old = os.environ.get("VITX_GENERIC_ATTN")
    os.environ["VITX_GENERIC_ATTN"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VITX_GENERIC_ATTN"]
        else:
            os.environ["VITX_GENERIC_ATTN"] = old


def _params(kw, seed=3):
    return R.init_params(R.table_of(kw), seed=seed)


def _inputs(kw, b, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((b, kw["image_size"], kw["image_size"], 3)).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    return img, dl


def _key(kw, P, img, dl):
    return (tuple(sorted((k, v) for k, v in kw.items())), hash(b"".join(np.ascontiguousarray(P[n]).tobytes() for n in sorted(P))), img.tobytes(), dl.tobytes())


_REF = {}


def _reference(kw, P, img, dl):
    """(float64 logits, gradients, d(img), the float32 evaluation's |d(last pos_emb)|): computed once per case and shared."""
    k = _key(kw, P, img, dl)
    if k not in _REF:
        rl, rg, rd = R.forward_backward(kw, P, img, dl)
        _, g32, _ = R.forward_backward(kw, P, img, dl, dtype=torch.float32)
        _REF[k] = (rl, rg, rd, float(np.abs(g32[R.last_pos_emb(kw)]).max()))
    return _REF[k]


def _errors(kw, m, img, dl, rg, rd):
    logits = m(img)
    grads, dimg = m.backward(dl, want_dimg=True)
    zero = R.last_pos_emb(kw)
    errs = {n: rel_max_err(grads[n], rg[n]) for n in rg if n != zero}
    errs["dimg"] = rel_max_err(dimg, rd)
    return logits, grads, dimg, errs, float(np.abs(grads[zero]).max())


def _check_fp32(tag, kw, m, img, dl, rl, rg, rd, noise32):
    logits, grads, dimg, errs, z = _errors(kw, m, img, dl, rg, rd)
    le = float(np.abs(logits - rl).max())
    worst = max(errs, key=errs.get)
    print(f"[nest:{tag}] max|dlogit| {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), |d last pos_emb| {z:.3e} (float32 on the CPU: {noise32:.3e})")
    gate(le, FP32_LOGIT_TOL, f"{tag} logits")
    for n, e in errs.items():
        gate(e, FP32_GRAD_RTOL, f"{tag} grad {n}")
    assert z <= 4.0 * noise32, f"{tag}: |d(last pos_emb)| {z:.3e} > 4 x {noise32:.3e}"
    return logits, grads, dimg


def _check_bf16(tag, kw, m, img, dl, rl, rg, rd):
    logits, grads, dimg, errs, z = _errors(kw, m, img, dl, rg, rd)
    le = float(np.abs(logits - rl).max()) / max(1.0, float(rl.std()))
    worst = max(errs, key=errs.get)
    print(f"[nest:{tag}] bf16 logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), |d last pos_emb| {z:.3e}")
    gate(le, BF16_GATES[0], f"{tag} bf16 logits", "nest bf16 logits")
    for n, e in errs.items():
        gate(e, BF16_GATES[1], f"{tag} bf16 grad {n}", "nest bf16 gradients")
    assert z <= BF16_GATES[2], f"{tag}: bf16 |d(last pos_emb)| {z:.3e} > {BF16_GATES[2]:.1e}"
    return logits, grads, dimg


@functools.lru_cache(maxsize=None)
def _fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    img, dl = z["img"].astype(np.float32), z["dlogits"].astype(np.float32)
    _, g32, _ = R.forward_backward(kw, P, img, dl, dtype=torch.float32)
    return kw, P, img, dl, z["logits"], {n: z["grad/" + n] for n in P}, z["dimg"], float(np.abs(g32[R.last_pos_emb(kw)]).max())


def _small_counts(kw):
    """Blocks the small-head kernels serve: the profiler books one attn_small_fwd and one attn_small_bwd scope per such block and step."""
    lv, n = R.levels_of(kw)
    return sum(depth for (_, _, dh, _, depth, _) in lv if dh in (16, 32) and n <= 288)


def _profile_step(m, img, dl):
    return m.profile(lambda: (m(img), m.backward(dl, want_dimg=True)))


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    kw, P, img, dl, rl, rg, rd, noise32 = _fixture(case)
    _check_fp32(f"{case} {compute}", kw, _model(kw, compute, 2, P), img, dl, rl, rg, rd, noise32)


def test_bf16_matches_reference_source():
    """The fixture case whose widths the bf16 mode accepts (dim_head 64 with heads 1: to_out kept, on the existing fused kernels)."""
    kw, P, img, dl, rl, rg, rd, _ = _fixture("nest_bf16")
    _check_bf16("nest_bf16 fixture", kw, _model(kw, "bf16", 2, P), img, dl, rl, rg, rd)


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_bf16_matches_restatement(shape):
    kw = BF16_SHAPES[shape]
    P = _params(kw)
    img, dl = _inputs(kw, 2, 1)
    rl, rg, rd, _ = _reference(kw, P, img, dl)
    _check_bf16(shape, kw, _model(kw, "bf16", 2, P), img, dl, rl, rg, rd)


# Where the small-head kernels are the default: the modes in which they measured faster than the materialised path at the usage shape (DESIGN.md
# section 20).  In the other modes they run on request (small_attn=True), which is how their fp32 FMA form is tested here.
SMALL_BY_DEFAULT = {"fp32": False, "bf16x3": False, "bf16": True}


def _fused_and_generic(kw, compute, P, img, dl, check):
    b = img.shape[0]
    m = _model(kw, compute, b, P, small_attn=True)
    m._ensure_handle(b)
    d = _model(kw, compute, b, P)
    d._ensure_handle(b)
    with _generic_attention():
        g = _model(kw, compute, b, P, small_attn=True)
        g._ensure_handle(b)
    check("fused", m)
    check("generic", g)
    blocks = _small_counts(kw)
    assert blocks > 0
    pm, pd, pg = _profile_step(m, img, dl), _profile_step(d, img, dl), _profile_step(g, img, dl)
    assert pm["attn_small_fwd"][0] == blocks and pm["attn_small_bwd"][0] == blocks, pm
    assert not any(k.startswith("attn_small") for k in pg), pg
    if SMALL_BY_DEFAULT[compute]:
        assert pd["attn_small_fwd"][0] == blocks and pd["attn_small_bwd"][0] == blocks, pd
    else:
        assert not any(k.startswith("attn_small") for k in pd), pd
    off = _model(kw, compute, b, P, small_attn=False)
    assert not any(k.startswith("attn_small") for k in _profile_step(off, img, dl))


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", ["nest_dh32_9tok", "nest_196tok"])
def test_fused_against_generic(case, compute):
    kw, P, img, dl, rl, rg, rd, noise32 = _fixture(case)
    _fused_and_generic(kw, compute, P, img, dl, lambda tag, m: _check_fp32(f"{case} {compute} {tag}", kw, m, img, dl, rl, rg, rd, noise32))


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_fused_against_generic_bf16(shape):
    kw = BF16_SHAPES[shape]
    P = _params(kw)
    img, dl = _inputs(kw, 2, 1)
    rl, rg, rd, _ = _reference(kw, P, img, dl)
    _fused_and_generic(kw, "bf16", P, img, dl, lambda tag, m: _check_bf16(f"{shape} {tag}", kw, m, img, dl, rl, rg, rd))


def test_dispatch_bound():
    """324 tokens per block, over LSA_N_MAX = 288, with the small-head kernels asked for: the generic path, no attn_small_* class, fp32 against
    the restatement."""
    kw = dict(image_size=36, patch_size=1, num_classes=3, dim=32, heads=2, num_hierarchies=2, block_repeats=1, mlp_mult=1)
    P = _params(kw)
    img, dl = _inputs(kw, 1, 2)
    rl, rg, rd, noise32 = _reference(kw, P, img, dl)
    m = _model(kw, "fp32", 1, P, small_attn=True)
    _check_fp32("324 tokens", kw, m, img, dl, rl, rg, rd, noise32)
    prof = _profile_step(m, img, dl)
    assert prof and not any(k.startswith("attn_small") for k in prof), prof


def test_one_token():
    """seq_len 1: softmax over one key, and the plain mode's n >= 1 (dim_head 16 at both levels)."""
    kw = dict(image_size=4, patch_size=2, num_classes=3, dim=16, heads=1, num_hierarchies=2, block_repeats=1, mlp_mult=2)
    P = _params(kw)
    img, dl = _inputs(kw, 2, 3)
    rl, rg, rd, noise32 = _reference(kw, P, img, dl)
    m = _model(kw, "fp32", 2, P, small_attn=True)
    _check_fp32("one token", kw, m, img, dl, rl, rg, rd, noise32)
    prof = _profile_step(m, img, dl)
    assert prof["attn_small_fwd"][0] == 2 and prof["attn_small_bwd"][0] == 2, prof


@pytest.mark.parametrize("dim", [8, 10])
def test_block_partition_is_bit_exact(dim):
    """A depth-0 level with a zeroed pos_emb: the partition and its inverse are pure copies, so 'level.0' equals 'embedded' bitwise (dim 8: the
    float4 path; dim 10: the scalar one).  With pos_emb set, the level adds pos_emb[h * w_ + w] of the position inside its block."""
    kw = dict(image_size=16, patch_size=2, num_classes=3, dim=dim, heads=1, num_hierarchies=3, block_repeats=(0, 1, 1), mlp_mult=1)
    P = _params(kw)
    pos = P["nest_layers.0.transformer.pos_emb"].copy()
    P["nest_layers.0.transformer.pos_emb"] = np.zeros_like(pos)
    img, dl = _inputs(kw, 2, 4)
    m = _model(kw, "fp32", 2, P)
    m(img)
    emb = m.read("embedded")
    assert emb.shape == (2, 8, 8, dim) and np.abs(emb).max() > 0
    assert np.array_equal(m.read("level.0"), emb)
    P["nest_layers.0.transformer.pos_emb"] = pos
    m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    m(img)
    want = m.read("embedded") + np.tile(pos.astype(np.float32).reshape(2, 2), (4, 4))[None, :, :, None]
    assert np.array_equal(m.read("level.0"), want.astype(np.float32))
    rl, rg, rd, noise32 = _reference(kw, P, img, dl)
    _check_fp32(f"depth-0 level, dim {dim}", kw, m, img, dl, rl, rg, rd, noise32)


def test_reads_match_restatement():
    kw, P, img, dl, *_ = _fixture("nest_small")
    m = _model(kw, "fp32", 2, P)
    m(img)
    taps = {}
    R.forward(kw, {n: torch.tensor(v) for n, v in P.items()}, torch.tensor(img.astype(np.float64)), taps)
    for name in ("embedded", "level.0", "aggregated.0", "level.1", "aggregated.1", "level.2", "pooled"):
        got, want = m.read(name), taps[name].numpy()
        assert got.shape == want.shape, name
        gate(rel_max_err(got, want), FP32_GRAD_RTOL, f"read {name}")
    with pytest.raises(Exception, match="unknown tensor name"):
        m.read("aggregated.2")


def test_batch_changes_and_repeated_passes_on_one_handle():
    """1 -> 3 -> 2 images on one handle, each against the restatement; two backward passes after one forward, and two whole steps, give the
    same bits (fixed-order reductions: d(pos_emb), the convolution's weight gradient, the LayerNorm parameter gradients)."""
    kw = G.kwargs_of("nest_196tok")
    P = _params(kw)
    m = _model(kw, "fp32", 3, P, conv_chunk=2, small_attn=True)
    for b in (1, 3, 2):
        img, dl = _inputs(kw, b, 10 + b)
        rl, rg, rd, noise32 = _reference(kw, P, img, dl)
        l1, g1, d1 = _check_fp32(f"batch {b}", kw, m, img, dl, rl, rg, rd, noise32)
        g2, d2 = m.backward(dl, want_dimg=True)
        l3 = m(img)
        g3, d3 = m.backward(dl, want_dimg=True)
        assert np.array_equal(d1, d2) and np.array_equal(d1, d3) and np.array_equal(l1, l3)
        for n in g1:
            assert np.array_equal(g1[n], g2[n]) and np.array_equal(g1[n], g3[n]), n
        assert np.abs(g1["nest_layers.0.transformer.pos_emb"]).max() > 0 and np.abs(g1["nest_layers.0.aggregate.conv.kernel"]).max() > 0


def test_nest_block_engine_refuses_the_image_entry_points():
    from vit_tensorflow import _native as N
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h = c.image_w = 16
    c.patch_h = c.patch_w = 4
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 3, 5, 32, 1, 2, 16, 32
    c.pool, c.ln_eps, c.max_batch, c.nest_block = N.POOL_CLS, 1e-5, 1, 1
    l, h = N.lib(), C.c_void_p()
    N.check(l.vitx_create(C.byref(c), C.byref(h)))
    try:
        img, out = np.zeros((1, 16, 16, 3), np.float32), np.zeros(17 * 32, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert l.vitx_forward(h, p(img), 1, 16, 16, 0, 0, p(out)) == N.ERR_UNSUPPORTED
        assert l.vitx_embed_forward(h, p(img), 1, 16, 16, p(out)) == N.ERR_UNSUPPORTED
    finally:
        l.vitx_destroy(h)


def test_training_with_dropout_is_refused():
    kw = G.kwargs_of("nest_1level")
    m = _model(kw, "fp32", 1)
    img = np.zeros((1, 8, 8, 3), np.float32)
    assert m(img, training=True).shape == (1, 3) and np.array_equal(m(img, training=True), m(img, training=False))
    from vit_tensorflow.nest import NesT
    d = NesT(**kw, dropout=0.2, max_batch=1)
    with pytest.raises(NotImplementedError, match="dropout"):
        d(img)
    assert d(img, training=False).shape == (1, 3)
