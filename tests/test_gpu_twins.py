"""twins_svt.TwinsSVT on the MI355X through the Python drop-in, against fixtures produced by the reference's own twins_svt.py
(tests/golden/ref_twins_*.npz) and against the float64 torch restatement (tests/twins_ref.py) where no fixture exists.

Every error is relative to the reference tensor's max (logits: absolute in the fp32 modes, over max(1, std) in bf16).  A tensor whose true
gradient is zero (to_q of an attention with one key) is gated against the largest gradient of the model.  The gates are 2x the worst value of
each kind observed on the MI355X (DESIGN.md section 21 lists them per case):

                                    logits      worst gradient or d(img) (case, tensor)
    fp32, fixtures + restatement    1.039e-5    7.755e-5 (global_k 7, svt_layers.0.transformer.0.0.ff2.fc2.bias)
    bf16x3                          1.197e-4    4.520e-4 (twins_k64, svt_layers.0.transformer.0.0.ff2.norm.b)
    bf16, restatement shapes        2.634e-2    1.898e-2 (call sequence, batch 1, svt_layers.0.transformer.0.0.local_attn.to_q.kernel)

The fp32 gradient figure is 2.5x NesT's bound: the worst tensors are bias and LayerNorm-offset gradients, column sums over every map position
whose terms largely cancel, behind a to_out that sums 512 products into a width of 4 or 8.  The bf16 row was observed on the materialised
attention path; with the few-key kernels (attn_fewkey.hip, the default in bf16 for at most 64 keys) the worst values are 2.634e-2 and 1.815e-2,
and on the materialised path of test_fewkey_against_materialised 2.942e-2 and 1.649e-2: the gates stay at 2x the first observation.
"""
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

import twins_ref as R  # noqa: E402
import gen_twins_fixtures as G  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

# (logits, worst gradient or d(img)), observed on the MI355X and the gates at 2x
OBSERVED_FP32 = (1.039e-5, 7.755e-5)
OBSERVED_X3 = (1.197e-4, 4.520e-4)
OBSERVED_BF16 = (2.634e-2, 1.898e-2)
FP32_GATES = (2.1e-5, 1.6e-4)
X3_GATES = (2.4e-4, 9.1e-4)
BF16_GATES = (5.3e-2, 3.8e-2)
# few-key kernels against the materialised path, both bf16: (logits over max(1, std), worst gradient or d(img) over the tensor's max)
# observed: logits 2.879e-2 (n49), worst gradient 1.515e-2 (m64_16_4_1, svt_layers.1.transformer.1.0.local_attn.to_q.kernel); gates at 2x.  (Under
# VITX_GENERIC_ATTN=1 the local pairs' attention leaves its fused kernels too, so the difference holds both attentions' rounding.)
FUSED_VS_GENERIC = (5.8e-2, 3.1e-2)


def _stages(dims, patches, locals_, ks, depths):
    return G._stages(dims, patches, locals_, ks, depths)


D64 = (64, 64, 64, 64)
# bf16 against the restatement, emb_dim 64: ((H, W), kwargs); (queries, keys) of the global attention per stage in the comments
BF16_SHAPES = {
    # 144/16, 36/9, 36/4, 36/1: 36 queries are no multiple of a 16- or 32-row tile
    "m16_9_4_1": ((12, 12), dict(num_classes=5, **_stages(D64, (1, 2, 1, 1), (2, 3, 2, 1), (3, 2, 3, 6), (0, 0, 0, 0)))),
    # 64/64 (as many keys as queries), 64/16, 16/4, 4/1; stage 2 has a second transformer
    "m64_16_4_1": ((16, 16), dict(num_classes=5, **_stages(D64, (2, 1, 2, 2), (2, 2, 2, 1), (1, 2, 2, 2), (0, 1, 0, 0)))),
    # 49 queries: 49/1 with one 7 x 7 window, 49/49 with one-token windows, 49/1, 49/1
    "n49": ((14, 14), dict(num_classes=4, **_stages(D64, (2, 1, 1, 1), (7, 1, 7, 1), (7, 1, 7, 7), (0, 0, 0, 0)))),
    # 324/81 (more than 64 keys), 81/9, 81/1 with one 81-token window, 9/9
    "n324_m81": ((18, 18), dict(num_classes=4, **_stages(D64, (1, 2, 1, 3), (2, 3, 9, 1), (2, 3, 9, 1), (0, 0, 0, 0)))),
}


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.twins_svt import TwinsSVT
    m = TwinsSVT(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
    if P is not None:
        m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    return m


def _params(kw, seed=3):
    return R.init_params(R.table_of(kw), seed=seed)


def _inputs(kw, hw, b, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((b, hw[0], hw[1], 3)).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    return img, dl


_REF = {}


def _reference(tag, kw, P, img, dl):
    """float64 (logits, gradients, d(img)): computed once per tag and shared."""
    if tag not in _REF:
        _REF[tag] = R.forward_backward(kw, P, img, dl)
    return _REF[tag]


def _errors(m, img, dl, rg, rd):
    """(logits, gradients, d(img), {tensor: error relative to its reference's max}); a reference that is exactly zero is measured against the
    largest gradient of the model instead."""
    logits = m(img)
    grads, dimg = m.backward(dl, want_dimg=True)
    top = max(float(np.abs(v).max()) for v in rg.values())
    errs = {}
    for n in rg:
        if np.abs(rg[n]).max() == 0:
            errs[n] = float(np.abs(grads[n]).max()) / top
        else:
            errs[n] = rel_max_err(grads[n], rg[n])
    errs["dimg"] = rel_max_err(dimg, rd)
    return logits, grads, dimg, errs


def _check(tag, compute, m, img, dl, rl, rg, rd):
    logits, grads, dimg, errs = _errors(m, img, dl, rg, rd)
    bf16 = compute == "bf16"
    le = float(np.abs(logits - rl).max()) / (max(1.0, float(rl.std())) if bf16 else 1.0)
    worst = max(errs, key=errs.get)
    print(f"[twins:{tag} {compute}] logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), dimg {errs['dimg']:.3e}")
    gates = {"fp32": FP32_GATES, "bf16x3": X3_GATES, "bf16": BF16_GATES}[compute]
    gate(le, gates[0], f"{tag} {compute} logits", f"twins {compute} logits")
    for n, e in errs.items():
        gate(e, gates[1], f"{tag} {compute} grad {n}", f"twins {compute} gradients")
    return logits, grads, dimg


@functools.lru_cache(maxsize=None)
def _fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    return G.kwargs_of(case), P, z["img"].astype(np.float32), z["dlogits"].astype(np.float32), z["logits"], {n: z["grad/" + n] for n in P}, z["dimg"]


def _profile_step(m, img, dl):
    return m.profile(lambda: (m(img), m.backward(dl, want_dimg=True)))


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    kw, P, img, dl, rl, rg, rd = _fixture(case)
    _check(case, compute, _model(kw, compute, 2, P), img, dl, rl, rg, rd)


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_bf16_matches_restatement(shape):
    hw, kw = BF16_SHAPES[shape]
    P = _params(kw)
    img, dl = _inputs(kw, hw, 2, 1)
    rl, rg, rd = _reference(shape, kw, P, img, dl)
    m = _model(kw, "bf16", 2, P)
    _check(shape, "bf16", m, img, dl, rl, rg, rd)
    prof = _profile_step(m, img, dl)
    assert prof["global_kv_unfold"][0] == sum(1 + d for (_, _, _, _, d, _) in R.stages_of(kw)), prof   # one per global block
    assert prof["global_kv_fold"][0] == prof["global_kv_unfold"][0] and prof["twins_peg_fwd"][0] == 4 and prof["twins_peg_bwd"][0] == 4, prof
    fused = _fewkey_blocks(hw, kw)
    assert prof.get("attn_fewkey_fwd", (0,))[0] == fused and prof.get("attn_fewkey_bwd", (0,))[0] == fused, prof   # the default in bf16: on


def _fewkey_blocks(hw, kw):
    """Global blocks whose key count the few-key kernels take (at most 64): one attn_fewkey_fwd and one _bwd scope per such block and step."""
    H, W = hw
    n = 0
    for (_, p, _, gk, depth, _) in R.stages_of(kw):
        H, W = H // p, W // p
        if (H // gk) * (W // gk) <= 64:
            n += 1 + depth
    return n


@contextlib.contextmanager
def _generic_attention():
    """VITX_GENERIC_ATTN=1 around the construction of a handle: the materialised attention path, i.e. what runs without the few-key kernels."""
    old = os.environ.get("VITX_GENERIC_ATTN")
    os.environ["VITX_GENERIC_ATTN"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VITX_GENERIC_ATTN"]
        else:
            os.environ["VITX_GENERIC_ATTN"] = old


def test_dispatch_bound():
    """64 keys take the few-key kernels, 65 do not (a 5 x 13 map with global_k 1), on both sides against the restatement; fused_global_attn=False
    and VITX_GENERIC_ATTN=1 keep the materialised path at 64 keys too, and the fp32 modes never take the kernels."""
    hw64, kw64 = BF16_SHAPES["m64_16_4_1"]
    hw65, kw65 = (5, 13), dict(num_classes=3, **_stages(D64, (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1), (0, 0, 0, 0)))
    for tag, hw, kw, want in (("64 keys", hw64, kw64, 5), ("65 keys", hw65, kw65, 0)):
        assert _fewkey_blocks(hw, kw) == want
        P = _params(kw)
        img, dl = _inputs(kw, hw, 2, 1)
        rl, rg, rd = _reference("m64_16_4_1" if want else "m65", kw, P, img, dl)
        m = _model(kw, "bf16", 2, P, fused_global_attn=True)
        _check(tag, "bf16", m, img, dl, rl, rg, rd)
        prof = _profile_step(m, img, dl)
        assert prof.get("attn_fewkey_fwd", (0,))[0] == want and prof.get("attn_fewkey_bwd", (0,))[0] == want, prof
    P = _params(kw64)
    img, dl = _inputs(kw64, hw64, 2, 1)
    off = _model(kw64, "bf16", 2, P, fused_global_attn=False, image_size=hw64)
    assert not any(k.startswith("attn_fewkey") for k in _profile_step(off, img, dl))
    with _generic_attention():
        g = _model(kw64, "bf16", 2, P, fused_global_attn=True, image_size=hw64)
    assert not any(k.startswith("attn_fewkey") for k in _profile_step(g, img, dl))
    x3 = _model(kw64, "bf16x3", 2, P, fused_global_attn=True, image_size=hw64)
    assert not any(k.startswith("attn_fewkey") for k in _profile_step(x3, img, dl))


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
def test_fewkey_against_materialised(shape):
    """The same bf16 handle with the few-key kernels and on the materialised path (VITX_GENERIC_ATTN=1 around construction): logits and every
    gradient, relative to the materialised path's tensor max.  Both paths' errors against float64 are printed by _check and listed in DESIGN.md
    section 21, so that this gate cannot hide a kernel that is worse than the path it replaces."""
    hw, kw = BF16_SHAPES[shape]
    P = _params(kw)
    img, dl = _inputs(kw, hw, 2, 1)
    rl, rg, rd = _reference(shape, kw, P, img, dl)
    f = _model(kw, "bf16", 2, P, fused_global_attn=True, image_size=hw)
    with _generic_attention():
        g = _model(kw, "bf16", 2, P, fused_global_attn=True, image_size=hw)
    lf, gf, df = _check(f"{shape} few-key", "bf16", f, img, dl, rl, rg, rd)
    lg, gg, dg = _check(f"{shape} materialised", "bf16", g, img, dl, rl, rg, rd)
    top = max(float(np.abs(v).max()) for v in gg.values())
    le = float(np.abs(lf - lg).max()) / max(1.0, float(np.asarray(lg).std()))
    errs = {n: (rel_max_err(gf[n], gg[n].astype(np.float64)) if np.abs(gg[n]).max() > 0 else float(np.abs(gf[n]).max()) / top) for n in gg}
    errs["dimg"] = rel_max_err(df, dg.astype(np.float64))
    worst = max(errs, key=errs.get)
    print(f"[twins:{shape} few-key against materialised] logits {le:.3e}, worst {errs[worst]:.3e} ({worst})")
    gate(le, FUSED_VS_GENERIC[0], f"{shape} few-key vs materialised logits", "twins few-key vs materialised logits")
    for n, e in errs.items():
        gate(e, FUSED_VS_GENERIC[1], f"{shape} few-key vs materialised {n}", "twins few-key vs materialised gradients")


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
def test_global_k_7_with_7x7_windows(compute):
    """The usage's reduction and window size: a 14 x 14 map (4 keys, four windows), then 7 x 7 maps (1 key, one window)."""
    hw, kw = (14, 14), dict(num_classes=3, **_stages((8, 8, 4, 4), (1, 2, 1, 1), (7, 7, 7, 1), (7, 7, 7, 7), (0, 0, 0, 0)))
    P = _params(kw)
    img, dl = _inputs(kw, hw, 2, 5)
    rl, rg, rd = _reference("k7", kw, P, img, dl)
    _check("k7", compute, _model(kw, compute, 2, P), img, dl, rl, rg, rd)


@pytest.mark.parametrize("kp", [3, 5])
@pytest.mark.parametrize("hw", [(4, 4), (4, 12)])
def test_peg(kp, hw):
    """PEG with a 3- and a 5-tap kernel on 2 x 2 maps (kernel 5 is larger than the map) and on 2 x 6 / 1 x 3 ones, read back against the
    restatement; with a zero kernel and bias the residual path is the identity, bit for bit."""
    kw = dict(num_classes=3, peg_kernel_size=kp, **_stages((4, 8, 4, 4), (2, 1, 1, 2), (2, 1, 2, 1), (2, 1, 1, 1), (0, 0, 0, 0)))
    P = _params(kw)
    img, dl = _inputs(kw, hw, 2, 6)
    m = _model(kw, "fp32", 2, P)
    m(img)
    taps = {}
    R.forward(kw, {n: torch.tensor(v) for n, v in P.items()}, torch.tensor(img.astype(np.float64)), taps)
    for s in range(4):
        for name in (f"embedded.{s}", f"pre_peg.{s}", f"peg.{s}", f"stage.{s}"):
            got, want = m.read(name), taps[name].numpy()
            assert got.shape == want.shape, name
            gate(rel_max_err(got, want), FP32_GATES[1], f"read {name}")
    gate(rel_max_err(m.read("pooled"), taps["pooled"].numpy()), FP32_GATES[1], "read pooled")
    with pytest.raises(Exception, match="unknown tensor name"):
        m.read("peg.4")
    rl, rg, rd = _reference(f"peg{kp}{hw}", kw, P, img, dl)
    _check(f"peg {kp} on {hw}", "fp32", m, img, dl, rl, rg, rd)
    for s in range(4):
        P[f"svt_layers.{s}.peg.kernel"] = np.zeros_like(P[f"svt_layers.{s}.peg.kernel"])
        P[f"svt_layers.{s}.peg.bias"] = np.zeros_like(P[f"svt_layers.{s}.peg.bias"])
    m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    m(img)
    for s in range(4):
        pre = m.read(f"pre_peg.{s}")
        assert np.abs(pre).max() > 0 and np.array_equal(m.read(f"peg.{s}"), pre), s


@pytest.mark.parametrize("dim", [8, 6])
@pytest.mark.parametrize("hw", [(8, 8), (4, 12)])
def test_window_partition_round_trip_is_bit_exact(hw, dim):
    """With to_out and fc2 of every pair zeroed each branch adds exact zeros, so what is left between 'embedded' and 'pre_peg' is the window
    partition and its inverse (and the copies through the two engines): the same bits, on square and rectangular window grids (dim 8: the
    float4 path, dim 6: the scalar one)."""
    kw = dict(num_classes=3, **_stages((dim, dim, dim, dim), (2, 1, 1, 1), (2, 1, 2, 1), (2, 1, 2, 1), (0, 0, 0, 0)))
    P = _params(kw)
    for n in P:
        if n.endswith((".to_out.kernel", ".to_out.bias", ".fc2.kernel", ".fc2.bias")):
            P[n] = np.zeros_like(P[n])
    img, _ = _inputs(kw, hw, 3, 7)
    m = _model(kw, "fp32", 3, P)
    m(img)
    for s in range(3):
        emb = m.read(f"embedded.{s}")
        assert np.abs(emb).max() > 0 and np.array_equal(m.read(f"pre_peg.{s}"), emb), s


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_call_sequences_on_one_object(compute):
    """Batch 3 -> 1 -> 3 on one object, a second backward, then an image of another size (the handle is created again, the weights are kept):
    every gradient against the restatement each time."""
    d = (64, 64, 64, 64) if compute == "bf16" else (8, 4, 8, 4)
    kw = dict(num_classes=4, **_stages(d, (2, 1, 2, 1), (2, 2, 1, 1), (2, 2, 1, 2), (0, 1, 0, 0)))
    P = _params(kw)
    m = _model(kw, compute, 3, P)
    for step, (hw, b) in enumerate([((8, 8), 3), ((8, 8), 1), ((8, 8), 3), ((8, 16), 2), ((8, 8), 1)]):
        img, dl = _inputs(kw, hw, b, 20 + step)
        rl, rg, rd = _reference(f"seq {compute} {step}", kw, P, img, dl)
        l1, g1, d1 = _check(f"step {step}: {hw} x {b}", compute, m, img, dl, rl, rg, rd)
        g2, d2 = m.backward(dl, want_dimg=True)
        assert np.array_equal(d1, d2)
        for n in g1:
            assert np.array_equal(g1[n], g2[n]), n
        assert (m._cfg.image_h, m._cfg.image_w) == hw
    for n, v in m.state_dict().items():
        assert np.array_equal(v, np.asarray(P[n], np.float32)), n


def test_global_k_engine_refuses_the_image_entry_points():
    from vit_tensorflow import _native as N
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h = c.image_w = 4
    c.patch_h = c.patch_w = 1
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 1, 1, 8, 1, 2, 16, 32
    c.pool, c.ln_eps, c.max_batch, c.nest_block, c.global_k = N.POOL_CLS, 1e-5, 1, 1, 2
    l, h = N.lib(), C.c_void_p()
    N.check(l.vitx_create(C.byref(c), C.byref(h)))
    try:
        img, out = np.zeros((1, 4, 4, 1), np.float32), np.zeros(18 * 8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert l.vitx_forward(h, p(img), 1, 4, 4, 0, 0, p(out)) == N.ERR_UNSUPPORTED
        assert l.vitx_embed_forward(h, p(img), 1, 4, 4, p(out)) == N.ERR_UNSUPPORTED
        tok = np.zeros((1, 9, 8), np.float32)      # the transformer entry takes image_h * image_w = 16 tokens per sequence, nothing else
        assert l.vitx_transformer_forward(h, p(tok), 1, 9, 0, 0, p(out)) == N.ERR_INVALID
    finally:
        l.vitx_destroy(h)


def test_training_with_dropout_is_refused():
    kw = G.kwargs_of("twins_tiny")
    m = _model(kw, "fp32", 1)
    img = np.zeros((1, 8, 8, 3), np.float32)
    assert m(img, training=True).shape == (1, 5) and np.array_equal(m(img, training=True), m(img, training=False))
    from vit_tensorflow.twins_svt import TwinsSVT
    d = TwinsSVT(**kw, dropout=0.2, max_batch=1)
    with pytest.raises(NotImplementedError, match="dropout"):
        d(img)
    assert d(img, training=False).shape == (1, 5)
