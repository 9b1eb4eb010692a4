"""pit.PiT and pit.Pool on the MI355X through the Python drop-in, against fixtures produced by the reference's own pit.py
(tests/golden/ref_pit_*.npz) and against the float64 torch restatement (tests/pit_ref.py) where no fixture exists.

Every error is relative to the reference tensor's max (logits: absolute in the fp32 modes, over max(1, std) in bf16).  pos_embedding rows an
image does not use have a true gradient of exactly zero and are compared with == 0 in every mode.  The gates are 2x the worst value of each
kind observed on the MI355X (profiles/pit/test_gpu_pit_observed_errors.log); the figures stand beside the constants
below.  An fp32 figure of 1.7e-4 (ten times the worst fp32 figure DESIGN.md section 22 records for CvT, 1.69e-5) would be a defect, not a
gate; every fp32 figure here is far below it.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pit_ref as R  # noqa: E402
import gen_pit_fixtures as G  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

# (logits, worst gradient or d(img)) observed on the MI355X, and the gates at 2x
OBSERVED_FP32 = (7.607e-7, 3.521e-6)     # pit_w64; pit_small, stage.2.0.ff.fc1.bias (the taps: 4.736e-7)
OBSERVED_X3 = (5.573e-6, 2.319e-5)       # pit_w64; pit_w64, stage.0.0.ff.fc2.kernel
OBSERVED_BF16 = (1.004e-2, 1.559e-2)     # pit_w64; pit_w64, pool.0.downsample.dw.kernel (the 325-token cases: 3.6e-3, 9.0e-3)
FP32_GATES = (1.6e-6, 7.1e-6)
X3_GATES = (1.2e-5, 4.7e-5)
BF16_GATES = (2.1e-2, 3.2e-2)
OBSERVED_TAPS = 4.736e-7                 # fp32 `read` taps against the restatement: pit_pooled, tokens
TAPS_GATE = 9.5e-7
# Pool alone: (output, worst gradient or d(tokens)), fp32 and bf16x3
OBSERVED_POOL_FP32 = (4.745e-7, 9.404e-7)   # 31 x 31, d = 64, batch 1; 31 x 31, d = 64, batch 3, downsample.pw.kernel
OBSERVED_POOL_X3 = (4.939e-6, 5.023e-6)     # 16 x 16, d = 64, batch 3; 7 x 7, d = 64, batch 3, downsample.pw.kernel
POOL_FP32_GATES = (9.5e-7, 1.9e-6)
POOL_X3_GATES = (9.9e-6, 1.1e-5)
# the streamed-key attention against the materialised path, both bf16: (logits over max(1, std), worst gradient or d(img) over the tensor's max)
OBSERVED_LONG_VS_MAT = (3.166e-3, 8.634e-3)   # depth (1, 1); depth (1, 1, 1), patch_embedding.kernel
LONG_VS_MAT = (6.4e-3, 1.8e-2)


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.pit import PiT
    m = PiT(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
    if P is not None:
        m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    return m


def _inputs(kw, hw, b, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((b, hw[0], hw[1], 3)).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    return img, dl


_REF = {}


def _reference(tag, kw, P, img, dl):
    """float64 (logits, gradients, d(img)): computed once per tag and shared."""
    if tag not in _REF:
        _REF[tag] = R.run(kw, P, img, dl)
    return _REF[tag]


def _errors(grads, dimg, rg, rd, truth=None):
    """{tensor: error relative to its reference's max}; where a row of the true gradient is exactly zero (pos_embedding rows the image does
    not use) the result must be exact zeros.  truth: the float64 gradients that say which those are, where rg itself is a rounded result."""
    truth = truth or rg
    errs = {}
    for n in rg:
        dead = ~np.any(np.asarray(truth[n]).reshape(-1, truth[n].shape[-1]), axis=1)
        if dead.any():
            got = np.asarray(grads[n]).reshape(-1, truth[n].shape[-1])[dead]
            assert np.all(got == 0), f"{n}: {int(dead.sum())} rows of the true gradient are exactly zero, got max |g| = {np.abs(got).max():.3e}"
        errs[n] = rel_max_err(grads[n], rg[n])
    errs["dimg"] = rel_max_err(dimg, rd)
    return errs


def _check(tag, compute, m, img, dl, rl, rg, rd):
    logits = m(img)
    grads, dimg = m.backward(dl, want_dimg=True)
    errs = _errors(grads, dimg, rg, rd)
    le = float(np.abs(logits - rl).max()) / (max(1.0, float(rl.std())) if compute == "bf16" else 1.0)
    worst = max(errs, key=errs.get)
    print(f"[pit:{tag} {compute}] logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), dimg {errs['dimg']:.3e}")
    gates = {"fp32": FP32_GATES, "bf16x3": X3_GATES, "bf16": BF16_GATES}[compute]
    gate(le, gates[0], f"{tag} {compute} logits", f"pit {compute} logits")
    for n, e in errs.items():
        gate(e, gates[1], f"{tag} {compute} grad {n}", f"pit {compute} gradients")
    return logits, grads, dimg


@functools.lru_cache(maxsize=None)
def _fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    return G.kwargs_of(case), P, z["img"].astype(np.float32), z["dlogits"].astype(np.float32), z["logits"], {n: z["grad/" + n] for n in P}, z["dimg"]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    kw, P, img, dl, rl, rg, rd = _fixture(case)
    m = _model(kw, compute, 2, P)
    _, g1, d1 = _check(case, compute, m, img, dl, rl, rg, rd)
    g2, d2 = m.backward(dl, want_dimg=True)   # no atomics anywhere: a second backward on one forward gives the same bits
    assert _same_bits(d1, d2) and all(_same_bits(g1[n], g2[n]) for n in g1)
    if compute == "fp32":   # the taps against the restatement
        import torch
        taps = {}
        R.forward(kw, {n: torch.tensor(v) for n, v in P.items()}, torch.tensor(img.astype(np.float64)), taps)
        for name, t in taps.items():
            e = rel_max_err(m.read(name), t.numpy())
            print(f"[pit:{case} fp32] read {name}: {e:.3e}")
            gate(e, TAPS_GATE, f"{case} read {name}", "pit fp32 taps")


def test_bf16_matches_float64():
    """pit_w64 (widths 64 -> 128, heads of 64, one Pool) in the bf16 mode against the reference's float64 fixture."""
    kw, P, img, dl, rl, rg, rd = _fixture("pit_w64")
    m = _model(kw, "bf16", 2, P)
    _, g1, d1 = _check("pit_w64", "bf16", m, img, dl, rl, rg, rd)
    g2, d2 = m.backward(dl, want_dimg=True)
    assert _same_bits(d1, d2) and all(_same_bits(g1[n], g2[n]) for n in g1)
    prof = m.profile(lambda: (m(img), m.backward(dl, want_dimg=True)))
    for cls in ("pit_unfold", "pit_embed", "pit_pool_fwd", "pit_pool_bwd", "pit_head"):
        assert cls in prof and prof[cls][0] >= 1, (cls, prof)
    assert prof["pit_pool_fwd"][0] == 1 and prof["pit_pool_bwd"][0] == 1, prof


# ------------------------------------------------------------------------------------------------ Pool alone
def _pool_check(tag, compute, pool, P, tokens, dout, want):
    out = pool(tokens)
    grads, dx = pool.backward(dout)
    ro, rg, rdx = want
    eo = rel_max_err(out, ro)
    errs = {n: rel_max_err(grads[n], rg[n]) for n in rg}
    errs["dtokens"] = rel_max_err(dx, rdx)
    worst = max(errs, key=errs.get)
    print(f"[pit-pool:{tag} {compute}] out {eo:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), dtokens {errs['dtokens']:.3e}")
    gates = POOL_FP32_GATES if compute == "fp32" else POOL_X3_GATES
    gate(eo, gates[0], f"pool {tag} {compute} out", f"pit pool {compute} out")
    for n, e in errs.items():
        gate(e, gates[1], f"pool {tag} {compute} grad {n}", f"pit pool {compute} gradients")
    g2, dx2 = pool.backward(dout)
    assert _same_bits(dx, dx2) and all(_same_bits(grads[n], g2[n]) for n in grads)


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
def test_pool_matches_reference_source(compute):
    """The reference's own Pool(8) on maps 7 x 7 (pads 1 | 1), 6 x 6 (0 | 1), 2 x 2 and 1 x 1 through the Python Pool, one object for all four."""
    from vit_tensorflow.pit import Pool
    z = G.load("pit_pool_layer")
    P = G.params_of(z)
    pool = Pool(G.POOL_DIM, compute=compute, seed=0)
    pool.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    for hw in G.POOL_MAPS:
        want = (z[f"out_{hw}"], {n: z[f"grad_{hw}/{n}"] for n in P}, z[f"dtokens_{hw}"])
        _pool_check(f"fixture {hw}x{hw}", compute, pool, P, z[f"tokens_{hw}"].astype(np.float32), z[f"dout_{hw}"].astype(np.float32), want)


@functools.lru_cache(maxsize=None)
def _pool_of(d, compute):
    from vit_tensorflow.pit import Pool
    P = R.init_params([(n, s, 0) for n, s in R.pool_table(d, "")], seed=5)
    pool = Pool(d, compute=compute, max_batch=3, seed=0)
    pool.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
    pool(np.zeros((3, 1 + 31 * 31, d), np.float32))   # the handle at its largest map and batch: made once
    return pool, P


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("d", [4, 64])
@pytest.mark.parametrize("hw", [1, 2, 7, 16, 31])
def test_pool_kernels(hw, d, b):
    """vitx_pit_pool_forward / _backward against the restatement: every padding case, widths on the vector (64, 4) path, one and several
    images; a 31 x 31 map at batch 3 is more than one slice of every sum."""
    pool, P = _pool_of(d, "fp32")
    rng = np.random.default_rng(100 * hw + d + b)
    tokens = rng.standard_normal((b, 1 + hw * hw, d)).astype(np.float32)
    dout = (rng.standard_normal((b, 1 + (-(-hw // 2)) ** 2, 2 * d)) / b).astype(np.float32)
    _pool_check(f"{hw}x{hw} d={d} b={b}", "fp32", pool, P, tokens, dout, R.run_pool(P, tokens, dout))


@pytest.mark.parametrize("d", [3, 64])
def test_pool_kernels_other_paths(d):
    """d = 3: the scalar form of the kernels (2 d = 6 is no multiple of 4); d = 64 in bf16x3: the Dense products on the split-operand kernel."""
    compute = "fp32" if d == 3 else "bf16x3"
    pool, P = _pool_of(d, compute)
    rng = np.random.default_rng(d)
    for hw in (7, 16):
        tokens = rng.standard_normal((3, 1 + hw * hw, d)).astype(np.float32)
        dout = (rng.standard_normal((3, 1 + (-(-hw // 2)) ** 2, 2 * d)) / 3).astype(np.float32)
        _pool_check(f"{hw}x{hw} d={d} b=3", compute, pool, P, tokens, dout, R.run_pool(P, tokens, dout))


def test_pool_refusals():
    from vit_tensorflow.pit import Pool
    pool = Pool(4)
    with pytest.raises(ValueError, match="square"):
        pool(np.zeros((1, 7, 4), np.float32))
    with pytest.raises(ValueError, match="tokens"):
        pool(np.zeros((1, 5, 3), np.float32))
    assert pool(np.zeros((2, 10, 4), np.float32)).shape == (2, 5, 8)
    with pytest.raises(ValueError, match="cotangent"):   # a cotangent of another size would be read past its end
        pool.backward(np.zeros((2, 4, 8), np.float32))
    assert pool.backward(np.zeros((2, 5, 8), np.float32))[1].shape == (2, 10, 4)


# ------------------------------------------------------------------------------------------------ one handle, many calls
def test_call_sequence_on_one_model():
    """Batch 2, then 3 (the handle is made again), then a smaller image (25 -> 9 -> 4 patch tokens: pos_embedding rows 26 .. 49 unused), then
    new weights -- each against the restatement."""
    kw = G.kwargs_of("pit_pooled")
    P = R.init_params(R.table_of(kw), seed=2)
    m = _model(kw, "fp32", None, P)
    for step, (b, hw) in enumerate([(2, (32, 32)), (3, (32, 32)), (3, (24, 24)), (1, (24, 24))]):
        if step == 3:
            P = R.init_params(R.table_of(kw), seed=9)
            m.load_state_dict({k: np.asarray(v, np.float32) for k, v in P.items()})
        img, dl = _inputs(kw, hw, b, 40 + step)
        rl, rg, rd = _reference(f"seq{step}", kw, P, img, dl)
        if hw == (24, 24):
            assert not np.any(rg["pos_embedding"][0, 26:]) and np.any(rg["pos_embedding"][0, 25])
        _check(f"call sequence step {step} (b={b}, {hw[0]}x{hw[1]})", "fp32", m, img, dl, rl, rg, rd)


# ------------------------------------------------------------------------------------------------ the long path
@pytest.mark.parametrize("depth", [(1, 1), (1, 1, 1)])
def test_long_attn_takes_the_streamed_kernels(depth):
    """Image 76, patch 8: 18 x 18 + 1 = 325 tokens (over 288) at width 64 with heads of 64, pooled, bf16.  (76 is no multiple of 8 and the
    reference's assertion is kept, so the model is constructed with image_size=80 -- 362 position rows -- and the handle follows the 76 x 76
    image of the call.)  depth=(1, 1) pools 18 -> 9 (pads 0 | 1); depth=(1, 1, 1) goes on 9 -> 5 (pads 1 | 1).  long_attn=True and
    long_attn=False are each held to the float64 restatement, then to each other; the streamed classes show up with long_attn=True only, and
    only for the 325-token stage."""
    kw = dict(image_size=80, patch_size=8, num_classes=5, dim=64, depth=depth, heads=2, dim_head=64, mlp_dim=128, pool_stages=True)
    P = R.init_params(R.table_of(kw), seed=4)
    img, dl = _inputs(kw, (76, 76), 2, 77)
    rl, rg, rd = _reference(f"long{len(depth)}", kw, P, img, dl)
    res = {}
    for long_attn in (True, False):
        m = _model(kw, "bf16", 2, P, long_attn=long_attn)
        res[long_attn] = _check(f"325 tokens depth={depth} long_attn={long_attn}", "bf16", m, img, dl, rl, rg, rd)
        prof = m.profile(lambda: (m(img), m.backward(dl, want_dimg=True)))
        streamed = {k: v[0] for k, v in prof.items() if k.startswith("attn_stream")}
        if long_attn:
            assert streamed == {"attn_stream_fwd": 1, "attn_stream_bwd": 1}, prof
        else:
            assert not streamed, prof
    (ll, gl, dl_), (lm, gm, dm) = res[True], res[False]
    errs = _errors(gl, dl_, {n: np.asarray(v, np.float64) for n, v in gm.items()}, np.asarray(dm, np.float64), truth=rg)
    le = float(np.abs(ll - lm).max()) / max(1.0, float(lm.std()))
    worst = max(errs, key=errs.get)
    print(f"[pit:325 tokens depth={depth} streamed vs materialised] logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst})")
    gate(le, LONG_VS_MAT[0], f"streamed vs materialised logits depth={depth}", "pit streamed vs materialised logits")
    for n, e in errs.items():
        gate(e, LONG_VS_MAT[1], f"streamed vs materialised grad {n} depth={depth}", "pit streamed vs materialised gradients")


# ------------------------------------------------------------------------------------------------ the refusals
def test_refusals():
    kw = dict(image_size=40, patch_size=8, num_classes=3, dim=8, depth=(1, 1), heads=1, mlp_dim=8, dim_head=8)
    img = np.zeros((1, 40, 40, 3), np.float32)
    m = _model(dict(kw, dropout=0.1), "fp32", 1)
    with pytest.raises(NotImplementedError, match="Dropout"):
        m(img)
    assert m(img, training=False).shape == (1, 3)
    with pytest.raises(NotImplementedError, match="Dropout"):
        _model(dict(kw, emb_dropout=0.1), "fp32", 1)(img, training=True)
    m = _model(kw, "fp32", 1)
    assert m(img).shape == (1, 3)
    with pytest.raises(ValueError, match="pos_embedding has 82 rows"):   # 11 x 11 + 1 tokens
        m(np.zeros((1, 48, 48, 3), np.float32))
    assert m(np.zeros((1, 32, 40, 3), np.float32)).shape == (1, 3)       # 7 x 9: fine without Pool
    with pytest.raises(ValueError, match="7 x 9"):
        _model(dict(kw, pool_stages=True), "fp32", 1)(np.zeros((1, 32, 40, 3), np.float32))
    for refused in (m.comm_init, m.capture_graph, m.optimizer_step, m.apply_gradients):
        with pytest.raises(NotImplementedError):
            refused()
    with pytest.raises(ValueError, match="long_attn"):
        m.set_long_attn(True)
