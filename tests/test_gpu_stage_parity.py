"""Per-stage parity of the bf16 ViT block on the GPU, forward and backward, from the engine's own saved activations.

One block (dim 128, 2 heads of 64, mlp_dim 256, depth 1) is run through `m.transformer(tokens)` / `m.transformer.backward(d_out)`; every stage is
then recomputed in float64 from the input of that stage AS THE ENGINE STORED IT (`vitx_debug_read`) and compared per element with the worst-case
rounding bound of that one stage (tests/stage_ref.py: about 2^-8 of the value where the output is bf16, about K 2^-24 where it is fp32).  The
bounds are derived, not fitted; tests/test_stage_bounds_host.py proves on the CPU that they accept a correctly rounded emulation and reject planted
defects, and that the inputs make every key matter.  A ratio err / bound above 1 is a finding.

Stages (forward): LayerNorm 1 / 2 with their statistics, to_qkv, attention and its lse, to_out + residual, fc1 + GELU (act and the stored gelu'),
fc2 + residual.  Links (backward): d_hpre, the fc2 / fc1 / to_qkv weight gradients and the fc2 / fc1 bias gradients, attention backward (d_qkv),
d_y1, the LayerNorm 1 parameter gradients.

Left to the whole-model tests (tests/test_gpu_parity.py and the fixtures), because the input of the link cannot be read once the backward has
finished: the to_out weight and bias gradients (the branch gradient is a ring slot that the next pass overwrites), the LayerNorm 2 VJP and its
parameter gradients (d(y2) is overwritten by d(y1)), and the final d(tokens).
"""
from __future__ import annotations

import numpy as np
import pytest

import stage_ref as sr
from util import gate

pytestmark = pytest.mark.gpu

KW = dict(image_size=272, patch_size=16, num_classes=4, dim=sr.DIM, depth=1, heads=sr.HEADS, mlp_dim=sr.MLP, dim_head=sr.DH)   # up to 291 tokens
FWD = ("x_in", "y1", "qkv", "attn_out", "x_mid", "y2", "hpre", "act", "x_out", "mean1", "rstd1", "mean2", "rstd2")
BWD = ("d_hpre", "d_attn_out", "d_qkv", "d_y1")


def make_model(params, compute="bf16", max_batch=3, **over):
    from vit_tensorflow import ViT
    kw = dict(KW)
    kw.update(over)
    m = ViT(**kw, compute=compute, max_batch=max_batch, seed=0)
    sd = m.state_dict()
    sd.update({k: np.asarray(v, np.float32) for k, v in params.items()})
    m.load_state_dict(sd)
    return m


def run_block(m, x, d_out=None, lse=True):
    out = m.transformer(x, training=False)
    reads = {k: m.debug_read(k, 0) for k in FWD + (("lse",) if lse else ())}
    grads = None
    if d_out is not None:
        grads, _ = m.transformer.backward(d_out)
        reads.update({k: m.debug_read(k, 0) for k in BWD})
    assert np.array_equal(np.asarray(out, np.float32).ravel(), reads["x_out"]), "x_out read differs from the call's result"
    return reads, grads


_RUNS = {}


def case(b, n, regime, long_attn=False):
    key = (b, n, regime, long_attn)
    if key not in _RUNS:
        P = sr.make_params(regime, n)
        x, d = sr.make_tokens(b, n, params=P, regime=regime)
        m = make_model(P, long_attn=long_attn)
        _RUNS[key] = (P, x, d) + run_block(m, x, d)
    return _RUNS[key]


def check(tag, P, d, reads, grads, b, n, form="either", gelu_rows=None, backward=True, only=None, weights_bf16=True):
    ch, ln32 = sr.block_checks(reads, grads, P, d, b, n, sr.HEADS, sr.DH, sr.EPS, form, gelu_rows, backward=backward, weights_bf16=weights_bf16)
    r = {nm: sr.worst_ratio(g, w, bd) for nm, g, w, bd in ch if only is None or nm.startswith(only)}
    print(f"[stage] gpu {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    print(f"[stage] ln32 {tag}: " + " ".join(f"{s}.{k}={v:.3e}" for s, mm in ln32.items() for k, v in mm.items()))
    for nm, v in r.items():
        assert np.isfinite(v), (tag, nm)
    for nm, v in r.items():
        gate(v, 1.0, f"{nm} ({tag})", f"stage {nm}")
    return r


# ------------------------------------------------------------------------------------------------ the debug hook itself
def test_debug_read_follows_the_geometry_of_a_transformer_call():
    """A full forward at one geometry, then transformer(tokens) at another b and n: every name returns b n rows, bit for bit what a fresh handle reads"""
    P = sr.make_params("random", 9)
    x, _ = sr.make_tokens(3, 9)
    names = FWD[:9]
    cols = dict(zip(names, (sr.DIM, sr.DIM, 3 * sr.DIM, sr.DIM, sr.DIM, sr.DIM, sr.MLP, sr.MLP, sr.DIM)))
    fresh = make_model(P, image_size=64)
    fresh.transformer(x, training=False)
    want = {k: fresh.debug_read(k, 0) for k in names + ("lse", "mean1", "rstd2")}
    used = make_model(P, image_size=64)
    used(np.random.default_rng(0).standard_normal((2, 64, 64, 3)).astype(np.float32), training=False)   # 2 x 17 rows
    used.transformer(x, training=False)
    for k in names:
        got = used.debug_read(k, 0)
        assert got.size == 3 * 9 * cols[k], (k, got.size)
        assert np.array_equal(got, want[k]), k
    for k, size in (("lse", 3 * sr.HEADS * 9), ("mean1", 27), ("rstd2", 27)):
        got = used.debug_read(k, 0)
        assert got.size == size and np.array_equal(got, want[k]), k


def test_backward_names_exist_only_between_a_backward_and_the_next_forward():
    from vit_tensorflow import _native as N
    b, n = 2, 9
    P = sr.make_params("random", n)
    x, d = sr.make_tokens(b, n)
    m = make_model(P, image_size=64)
    m.transformer(x, training=False)
    for k in BWD:
        with pytest.raises(N.VitxError):
            m.debug_read(k, 0)
    m.transformer.backward(d)
    sizes = dict(zip(BWD, (sr.MLP, sr.DIM, 3 * sr.DIM, sr.DIM)))
    for k in BWD:
        assert m.debug_read(k, 0).size == b * n * sizes[k], k
    m.transformer(x, training=False)
    with pytest.raises(N.VitxError):
        m.debug_read("d_qkv", 0)
    f = make_model(P, compute="fp32", image_size=64)   # the materialised attention keeps no [b, heads, n] lse
    f.transformer(x, training=False)
    with pytest.raises(N.VitxError):
        f.debug_read("lse", 0)


# ------------------------------------------------------------------------------------------------ every stage and link
@pytest.mark.parametrize("regime", ["random", "sharp"])
@pytest.mark.parametrize("b,n", sr.CASES)
def test_every_stage_forward_and_backward(b, n, regime):
    P, x, d, reads, grads = case(b, n, regime)
    check(f"b={b} n={n} {regime}", P, d, reads, grads, b, n)


@pytest.mark.parametrize("n", [65, 288])
def test_saturated_softmax_is_finite_and_inside_the_bounds(n):
    P, x, d, reads, grads = case(2, n, "saturated")
    for k, v in reads.items():
        assert np.isfinite(v).all(), k
    for k, v in grads.items():
        assert np.isfinite(v).all(), k
    check(f"b=2 n={n} saturated", P, d, reads, grads, 2, n)


def test_streamed_keys():
    """long_attn past 288 tokens: attn_stream.hip, same saved state, same gates"""
    P, x, d, reads, grads = case(1, 289, "sharp", long_attn=True)
    check("b=1 n=289 sharp streamed", P, d, reads, grads, 1, 289)


# interior tiles of the 256-row pipelined variant (13, with either epilogue bit) read GELU from the LDS table, every other tile and variant evaluates
# the polynomial (gemm_bf16_pipe.hip: GTAB = MODE == EPI_BIAS_GELU && BM == 256, use_tab inside the wave-private epilogue of interior tiles)
VARIANTS = [("13", "table"), ("11", "poly"), ("2", "poly"), ("9", "poly"), (str(13 + 256), "table"), (str(2 + 512), "poly")]


@pytest.mark.parametrize("kernel,form", VARIANTS)
def test_gemm_variants(monkeypatch, kernel, form):
    b, n = 3, 97   # 291 rows: one full 256-row tile and a tail
    monkeypatch.setenv("VITX_GEMM_KERNEL", kernel)
    P = sr.make_params("random", n)
    x, d = sr.make_tokens(b, n)
    reads, grads = run_block(make_model(P), x, d)
    check(f"b=3 n=97 random VITX_GEMM_KERNEL={kernel}", P, d, reads, grads, b, n, form, (b * n) // 256 * 256 if form == "table" else None)


def test_generic_gemm(monkeypatch):
    """the k-ordered fp32-FMA kernel on every Dense: bf16 activations against the fp32 parameters themselves (no bf16 operand copy on this path)"""
    b, n = 3, 97
    monkeypatch.setenv("VITX_GENERIC_GEMM", "1")
    P = sr.make_params("random", n)
    x, d = sr.make_tokens(b, n)
    reads, grads = run_block(make_model(P), x, d)
    check("b=3 n=97 random VITX_GENERIC_GEMM=1", P, d, reads, grads, b, n, "poly", weights_bf16=False)


@pytest.mark.parametrize("kernel,form", [("13", "table"), ("11", "poly")])
def test_gelu_sweep_against_erf(monkeypatch, kernel, form):
    """act and the stored gelu' against erf on a ramp of bf16 patterns: every binade from 2^-13 to 2^4 in both signs, both sides of the polynomial
    clamp at 3.96 and of the table ends at 2^-12 and 8 (the patterns are asserted in tests/test_stage_bounds_host.py)"""
    b, n = 3, 97
    monkeypatch.setenv("VITX_GEMM_KERNEL", kernel)
    P = sr.make_sweep_params()
    x, _ = sr.make_tokens(b, n)
    reads, _ = run_block(make_model(P, mlp_dim=sr.SWEEP_MLP), x)
    check(f"gelu sweep VITX_GEMM_KERNEL={kernel}", P, None, reads, None, b, n, form, 256 if form == "table" else None, backward=False, only="fc1")


# ------------------------------------------------------------------------------------------------ LayerNorm edges
@pytest.mark.parametrize("compute,dim", [("bf16", sr.DIM), ("fp32", sr.DIM), ("fp32", 132)])
def test_layernorm_edge_rows(compute, dim):
    """rows with a common offset of 30 sigma, rows of variance exactly 0, rows with one 1e4 outlier (one kind per image); in fp32 mode y1 is stored in
    fp32 and the bound is ln32 alone.  dim = 132 takes the guarded tail of the vector path (33 of the 64 lanes hold a float4)."""
    kinds = sr.ln_edge_inputs(dim)
    x = np.stack(list(kinds.values()), 0)
    r = np.random.default_rng(11)
    P = {sr.PFX + "attn.norm.gamma": (1.0 + 0.1 * r.standard_normal(dim)).astype(np.float32),
         sr.PFX + "attn.norm.beta": (0.1 * r.standard_normal(dim)).astype(np.float32)}
    m = make_model(P, compute=compute, image_size=64, dim=dim)
    m.transformer(x, training=False)
    y, mean, rstd = (m.debug_read(k, 0) for k in ("y1", "mean1", "rstd1"))
    assert np.array_equal(m.debug_read("x_in", 0), x.ravel())
    rows = x.shape[1]
    for i, kind in enumerate(kinds):
        sl = slice(i * rows, (i + 1) * rows)
        ln, ln32 = sr.layernorm_ref(x[i], P[sr.PFX + "attn.norm.gamma"], P[sr.PFX + "attn.norm.beta"], sr.EPS, compute == "bf16")
        got = {"y": y.reshape(-1, dim)[sl], "mean": mean[sl], "rstd": rstd[sl]}
        rr = {k: sr.worst_ratio(got[k], *ln[k]) for k in got}
        print(f"[stage] gpu layernorm {compute} dim={dim} '{kind}': " + " ".join(f"{k}={v:.3f}" for k, v in rr.items()))
        print(f"[stage] ln32 layernorm {compute} dim={dim} '{kind}': " + " ".join(f"{k}={v:.3e}" for k, v in ln32.items()))
        for k, v in rr.items():
            gate(v, 1.0, f"ln1.{k} {compute} dim={dim} '{kind}'", f"stage layernorm edge {k}")


# ------------------------------------------------------------------------------------------------ the gates bite on hardware data
@pytest.mark.parametrize("n", [65, 288])
def test_gate_rejects_a_wrong_reference_on_gpu_output(n):
    """The GPU's own output against deliberately wrong references (no extra GPU work: the runs above are reused): last key dropped, two keys of one
    32-key group swapped, last K element of a Dense dropped.  Each must fail the gate the right reference passes."""
    b = 2
    P, x, d, reads, grads = case(b, n, "sharp")
    got = reads["attn_out"].reshape(b * n, -1)
    right, _ = sr.attn_fwd_ref(reads["qkv"], b, n, sr.HEADS, sr.DH, 0.125)
    assert sr.worst_ratio(got, *right["attn_out"]) <= 1.0
    wrong, _ = sr.attn_fwd_ref(reads["qkv"], b, n, sr.HEADS, sr.DH, 0.125, drop_key=n - 1)
    r1 = sr.worst_ratio(got, *wrong["attn_out"])
    wrong, _ = sr.attn_fwd_ref(reads["qkv"], b, n, sr.HEADS, sr.DH, 0.125, swap_keys=(34, 35))
    r2 = sr.worst_ratio(got, *wrong["attn_out"])
    wb = sr.f64(sr.bf16_rne(P[sr.PFX + "attn.to_qkv.kernel"]))
    y1 = sr.f64(reads["y1"]).reshape(b * n, sr.DIM)
    assert sr.worst_ratio(reads["qkv"].reshape(b * n, -1), *sr.dense_ref(y1, wb)) <= 1.0
    r3 = sr.worst_ratio(reads["qkv"].reshape(b * n, -1), *sr.dense_ref(y1[:, :-1], wb[:-1]))
    print(f"[stage] gpu wrong references n={n}: last key dropped {r1:.1f}, keys 34 / 35 swapped {r2:.1f}, last K element dropped {r3:.1f}")
    assert r1 > 1.0 and r2 > 1.0 and r3 > 1.0
