"""crossformer.CrossFormer on the MI355X through the Python drop-in, against fixtures produced by the reference's own crossformer.py
(tests/golden/ref_cf_*.npz) and against the float64 torch restatement (tests/crossformer_ref.py) where no fixture exists.

Every error is relative to the reference tensor's max (logits: absolute in the fp32 modes, over max(1, std) in bf16).  The dpb.* gradients are
compared with == 0.  The q and k thirds of to_qkv of a one-token window have a true gradient of zero (softmax == 1 whatever q and k are): they
are gated against the largest gradient of the model, the v third against its own max.  The gates are 2x the worst value of each kind observed
on the MI355X (profiles/crossformer/test_gpu_crossformer_observed_errors.log):

                                    logits      worst gradient or d(img) (case, tensor)
    fp32, fixtures + restatement    2.452e-6    4.803e-6 (cf_usage_windows, crossformer_layers.0.transformer.0.short_ff.fc2.kernel)
    bf16x3                          2.741e-5    1.995e-5 (cf_bf16_w64, crossformer_layers.0.transformer.0.short_attn.to_qkv.kernel, q and k thirds)
    bf16, fixtures + restatement    1.204e-2    1.781e-2 (call sequence, batch 1, crossformer_layers.1.transformer.0.long_attn.to_qkv.kernel, q and k thirds)
    position bias, fp32 network     1.689e-7 of the bias's max (bias.2.0.long)
    window kernels / small BIAS     3.238e-5    4.167e-3 (cf_bf16, crossformer_layers.0.transformer.0.short_attn.to_qkv.kernel, q and k thirds)
    one attention alone, bf16       o 2.817e-3 (n = 16), d(q, k, v) 6.130e-3 (n = 4); the two kernel families give the same figures

The fp32 figures are an order of magnitude under TwinsSVT's: heads of 32 behind widths of 32 .. 128 sum far fewer products per output than
TwinsSVT's 512-wide to_out into a width of 4 or 8.  In bf16 the two attention forms give the same worst values to three digits (the window
kernels' error is storage rounding, as the small-head form's is).
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import crossformer_ref as R  # noqa: E402
import gen_crossformer_fixtures as G  # noqa: E402
from util import gate, rel_max_err  # noqa: E402

pytestmark = pytest.mark.gpu

# (logits, worst gradient or d(img)), observed on the MI355X and the gates at 2x
OBSERVED_FP32 = (2.452e-6, 4.803e-6)
OBSERVED_X3 = (2.741e-5, 1.995e-5)
OBSERVED_BF16 = (1.204e-2, 1.781e-2)
OBSERVED_BIAS = 1.689e-7
FP32_GATES = (4.9e-6, 9.6e-6)
X3_GATES = (5.5e-5, 4.0e-5)
BF16_GATES = (2.4e-2, 3.6e-2)
BIAS_GATE = 3.4e-7
# the window kernels against the BIAS form of the small-head kernels, both bf16: (logits over max(1, std), worst gradient or d(img) over the tensor's max)
# observed 3.238e-5 (cf_bf16_w64) and 4.167e-3 (cf_bf16); gates at 2x
WINDOW_VS_SMALL = (6.5e-5, 8.4e-3)
# one attention alone on bf16 inputs against float64: (o, worst of d(q), d(k), d(v)), relative to the tensor's max.  Storage alone costs 2^-9 per
# rounding: o and P are rounded once each, dS, P and the outputs once each on the way to d(q, k, v).  Observed 2.817e-3 and 6.130e-3; gates at 2x
KERNEL_GATES = (5.7e-3, 1.3e-2)
BF16_CASES = ("cf_bf16", "cf_bf16_w64")


def _model(kw, compute, max_batch, P=None, **extra):
    from vit_tensorflow.crossformer import CrossFormer
    m = CrossFormer(**kw, compute=compute, max_batch=max_batch, seed=0, **extra)
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
        _REF[tag] = R.forward_backward(kw, P, img, dl)
    return _REF[tag]


def _errors(grads, dimg, rg, rd, truth=None):
    """{tensor: error relative to its reference's max}; the dpb gradients must be exact zeros; a part of a tensor whose true gradient is zero is
    measured against the largest gradient of the model instead.  truth: the float64 gradients that say which parts those are, where rg itself
    is a rounded result (one bf16 form against another: both hold rounding noise there)."""
    truth = truth or rg
    top = max(float(np.abs(v).max()) for v in rg.values())
    errs = {}
    for n in rg:
        if R.is_dpb(n):
            assert np.all(rg[n] == 0) and np.all(grads[n] == 0), n
            continue
        if n.endswith(".to_qkv.kernel"):
            inner = rg[n].shape[-1] // 3
            qk, v = (Ellipsis, slice(0, 2 * inner)), (Ellipsis, slice(2 * inner, None))
            parts = {n + "[q,k]": (grads[n][qk], rg[n][qk], truth[n][qk]), n + "[v]": (grads[n][v], rg[n][v], truth[n][v])}
        else:
            parts = {n: (grads[n], rg[n], truth[n])}
        for pn, (got, ref, tr) in parts.items():
            errs[pn] = float(np.abs(got - ref).max()) / top if np.abs(tr).max() <= 1e-13 * top else rel_max_err(got, ref)
    errs["dimg"] = rel_max_err(dimg, rd)
    return errs


def _check(tag, compute, m, img, dl, rl, rg, rd):
    logits = m(img)
    grads, dimg = m.backward(dl, want_dimg=True)
    errs = _errors(grads, dimg, rg, rd)
    bf16 = compute == "bf16"
    le = float(np.abs(logits - rl).max()) / (max(1.0, float(rl.std())) if bf16 else 1.0)
    worst = max(errs, key=errs.get)
    print(f"[crossformer:{tag} {compute}] logits {le:.3e}, worst grad rel err {errs[worst]:.3e} ({worst}), dimg {errs['dimg']:.3e}")
    gates = {"fp32": FP32_GATES, "bf16x3": X3_GATES, "bf16": BF16_GATES}[compute]
    gate(le, gates[0], f"{tag} {compute} logits", f"crossformer {compute} logits")
    for n, e in errs.items():
        gate(e, gates[1], f"{tag} {compute} grad {n}", f"crossformer {compute} gradients")
    return logits, grads, dimg


@functools.lru_cache(maxsize=None)
def _fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    return G.kwargs_of(case), P, z["img"].astype(np.float32), z["dlogits"].astype(np.float32), z["logits"], {n: z["grad/" + n] for n in P}, z["dimg"]


def _profile_step(m, img, dl):
    return m.profile(lambda: (m(img), m.backward(dl, want_dimg=True)))


def _attentions(kw):
    return 2 * sum(depth for (_, depth, *_rest) in R.stages_of(kw))


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_matches_reference_source(case, compute):
    kw, P, img, dl, rl, rg, rd = _fixture(case)
    _check(case, compute, _model(kw, compute, 2, P), img, dl, rl, rg, rd)


@pytest.mark.parametrize("window", [True, False])
@pytest.mark.parametrize("case", BF16_CASES)
def test_bf16_matches_float64(case, window):
    """bf16 against the float64 fixtures: windows of 1, 4 and 16 tokens with two and four heads (cf_bf16), 49 and 64 tokens (cf_bf16_w64); with
    the window kernels (attn_window.hip) and with the BIAS form of the small-head kernels on bf16 storage (window_attn=False).  Every
    attention of the step runs the class asked for."""
    kw, P, img, dl, rl, rg, rd = _fixture(case)
    m = _model(kw, "bf16", 2, P, window_attn=window)
    _check(f"{case} {'window' if window else 'small BIAS'}", "bf16", m, img, dl, rl, rg, rd)
    prof = _profile_step(m, img, dl)
    on, off = ("attn_window", "attn_small") if window else ("attn_small", "attn_window")
    assert prof[on + "_fwd"][0] == _attentions(kw) and prof[on + "_bwd"][0] == _attentions(kw), prof
    assert not any(k.startswith(off) for k in prof), prof


@pytest.mark.parametrize("case", BF16_CASES)
def test_window_kernels_against_small_bias_form(case):
    """The same bf16 handle with the window kernels and with the BIAS form of the small-head kernels: logits and every gradient, relative to
    the small-head form's tensor max.  Both forms' errors against float64 are gated by test_bf16_matches_float64, so this gate cannot hide a
    kernel that is worse than the form it replaces."""
    kw, P, img, dl, rl, rg, rd = _fixture(case)
    lw, gw, dw = (lambda m: (m(img),) + m.backward(dl, want_dimg=True))(_model(kw, "bf16", 2, P, window_attn=True))
    ls, gs, dsm = (lambda m: (m(img),) + m.backward(dl, want_dimg=True))(_model(kw, "bf16", 2, P, window_attn=False))
    errs = _errors(gw, dw, {n: np.asarray(v, np.float64) for n, v in gs.items()}, np.asarray(dsm, np.float64), truth=rg)
    le = float(np.abs(lw - ls).max()) / max(1.0, float(np.asarray(ls).std()))
    worst = max(errs, key=errs.get)
    print(f"[crossformer:{case} window against small BIAS] logits {le:.3e}, worst {errs[worst]:.3e} ({worst})")
    gate(le, WINDOW_VS_SMALL[0], f"{case} window vs small logits", "crossformer window vs small logits")
    for n, e in errs.items():
        gate(e, WINDOW_VS_SMALL[1], f"{case} window vs small {n}", "crossformer window vs small gradients")


def _attention_f64(qkv, d_o, bias):
    """float64 softmax(q k^T / sqrt(32) + bias) v and its VJP on [b, n, 3, h, 32] / [b, n, h * 32]."""
    q, k, v = (torch.tensor(qkv[:, :, i].astype(np.float64)).permute(0, 2, 1, 3).requires_grad_(True) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * 32 ** -0.5 + torch.tensor(bias.astype(np.float64)), -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(d_o.shape)
    g = torch.autograd.grad((o * torch.tensor(d_o.astype(np.float64))).sum(), [q, k, v])
    return o.detach().numpy(), np.stack([t.permute(0, 2, 1, 3).numpy() for t in g], axis=2)


def _bf16_round(a):
    return torch.tensor(a).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("n", [1, 4, 9, 16, 49, 64])
def test_window_kernel_masks_instead_of_padding(n):
    """The window kernels at every tile count and fill, with the activation buffers pre-filled with NaN beyond the live rows (every access stays
    inside the allocation): the outputs are finite and have the bits of the run on zero-filled buffers, the tails of the output buffers are
    untouched, and the results agree with float64 on the same bf16 inputs and with the BIAS form of the small-head kernels.  5 windows x 2 heads:
    more problems than a workgroup has waves, and no multiple of it."""
    m = _model(G.kwargs_of("cf_bf16"), "bf16", 1, image_size=(16, 16))
    rng = np.random.default_rng(100 + n)
    b, h = 5, 2
    qkv = _bf16_round(rng.standard_normal((b, n, 3, h, 32)).astype(np.float32))
    d_o = _bf16_round(rng.standard_normal((b, n, h * 32)).astype(np.float32))
    bias = rng.standard_normal((n, n)).astype(np.float32)
    o0, l0, d0, ot0, dt0 = m.window_attention(qkv, d_o, bias, tail_rows=64, tail_value=0.0)
    o1, l1, d1, ot1, dt1 = m.window_attention(qkv, d_o, bias, tail_rows=64, tail_value=float("nan"))
    assert np.isfinite(o1).all() and np.isfinite(l1).all() and np.isfinite(d1).all()
    assert np.array_equal(o0, o1) and np.array_equal(l0, l1) and np.array_equal(d0, d1)
    assert np.all(ot0 == 0) and np.all(dt0 == 0) and np.isnan(ot1).all() and np.isnan(dt1).all()
    ro, rd = _attention_f64(qkv, d_o, bias)
    so, sl, sd, _, _ = m.window_attention(qkv, d_o, bias, window_kernel=False)
    eo, ed = rel_max_err(o1, ro), max(rel_max_err(d1[:, :, i], rd[:, :, i]) if np.abs(rd[:, :, i]).max() > 1e-12 else float(np.abs(d1[:, :, i]).max())
                                      for i in range(3))
    so_e, sd_e = rel_max_err(so, ro), max(rel_max_err(sd[:, :, i], rd[:, :, i]) if np.abs(rd[:, :, i]).max() > 1e-12 else float(np.abs(sd[:, :, i]).max())
                                          for i in range(3))
    print(f"[crossformer:window kernel n={n}] o {eo:.3e} d(qkv) {ed:.3e}; small BIAS form o {so_e:.3e} d(qkv) {sd_e:.3e}; lse diff {np.abs(l1 - sl).max():.3e}")
    gate(eo, KERNEL_GATES[0], f"window kernel n={n} o", "crossformer window kernel o")
    gate(ed, KERNEL_GATES[1], f"window kernel n={n} d(qkv)", "crossformer window kernel d(qkv)")
    gate(so_e, KERNEL_GATES[0], f"small BIAS kernel n={n} o", "crossformer small BIAS kernel o")
    gate(sd_e, KERNEL_GATES[1], f"small BIAS kernel n={n} d(qkv)", "crossformer small BIAS kernel d(qkv)")


def test_position_bias_buffers():
    """The [n, n] bias of a short and of two long attentions of cf_rect, read back against the restatement's: window sizes 3 and 2 are where
    the reference's row stride 2 wsz - 1 differs from a symmetric one."""
    kw, P, img, dl, *_ = _fixture("cf_rect")
    m = _model(kw, "fp32", 2, P)
    m(img)
    taps = {}
    R.forward(kw, {n: torch.tensor(v) for n, v in P.items()}, torch.tensor(img.astype(np.float64)), taps)
    for which, pre, n in (("bias.0.0.short", "crossformer_layers.0.transformer.0.short_attn", 9),
                          ("bias.0.0.long", "crossformer_layers.0.transformer.0.long_attn", 4),
                          ("bias.1.1.short", "crossformer_layers.1.transformer.1.short_attn", 4),
                          ("bias.2.0.long", "crossformer_layers.2.transformer.0.long_attn", 9),
                          ("bias.3.0.long", "crossformer_layers.3.transformer.0.long_attn", 1)):
        got, want = m.read(which), taps["bias." + pre].numpy()
        assert got.shape == want.shape == (n, n), which
        e = rel_max_err(got, want)
        print(f"[crossformer:bias {which}] rel err {e:.3e} (max |bias| {np.abs(want).max():.3f})")
        assert np.abs(want).max() > 1e-2
        gate(e, BIAS_GATE, f"read {which}", "crossformer position bias")
        if n > 1:   # the symmetric index arithmetic would give another matrix
            wsz = int(round(np.sqrt(n)))
            i, j = np.divmod(np.arange(n), wsz)
            sym = (i[:, None] - i[None, :] + wsz) * (2 * wsz + 1) + j[:, None] - j[None, :] + wsz
            assert not np.array_equal(sym, R.rel_pos_indices(wsz))
    for name in ("embedded.0", "stage.0", "embedded.3", "stage.3", "pooled"):
        got, want = m.read(name), taps[name].numpy()
        assert got.shape == want.shape, name
        e = rel_max_err(got, want)
        print(f"[crossformer:read {name}] rel err {e:.3e}")
        gate(e, FP32_GATES[1], f"read {name}")
    with pytest.raises(Exception, match="unknown tensor name"):
        m.read("bias.0.1.short")           # stage 1 has one layer


@contextlib.contextmanager
def _generic_attention():
    old = os.environ.get("VITX_GENERIC_ATTN")
    os.environ["VITX_GENERIC_ATTN"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VITX_GENERIC_ATTN"]
        else:
            os.environ["VITX_GENERIC_ATTN"] = old


def test_dispatch():
    """81 tokens (a 9 x 9 window on a 9 x 9 map) run the BIAS form of the small-head kernels whatever window_attn says, in bf16 and fp32; 64 and
    49 tokens (cf_bf16_w64) run the window kernels with window_attn=True, the small-head ones with False, and the fp32 modes never take the
    window kernels.  Under VITX_GENERIC_ATTN a biased engine is refused: the materialised path has no bias."""
    from vit_tensorflow import _native as N
    kw81 = dict(dim=64, depth=(1, 0, 0, 0), global_window_size=(9, 1, 1, 1), local_window_size=(9, 1, 1, 1),
                cross_embed_kernel_sizes=((1, 2), (1,), (1,), (1,)), cross_embed_strides=1, num_classes=3)
    P = R.init_params(R.table_of(kw81), seed=3)
    img, dl = _inputs(kw81, (9, 9), 2, 1)
    rl, rg, rd = _reference("n81", kw81, P, img, dl)
    for compute in ("bf16", "fp32"):
        m = _model(kw81, compute, 2, P, window_attn=True)
        _check("81 tokens", compute, m, img, dl, rl, rg, rd)
        prof = _profile_step(m, img, dl)
        assert prof["attn_small_fwd"][0] == 2 and prof["attn_small_bwd"][0] == 2, prof
        assert prof["cf_windows"][0] > 0 and prof["cf_head"][0] == 2 and not any(k.startswith("attn_window") for k in prof), prof
    kw, P, img, dl, *_ = _fixture("cf_bf16_w64")
    for compute, window, want in (("bf16", True, "attn_window"), ("bf16", False, "attn_small"), ("bf16x3", True, "attn_small")):
        prof = _profile_step(_model(kw, compute, 2, P, window_attn=window, image_size=(56, 56)), img, dl)
        assert prof[want + "_fwd"][0] == 2 and prof[want + "_bwd"][0] == 2, (compute, window, prof)
        assert not any(k.startswith("attn_small" if want == "attn_window" else "attn_window") for k in prof), (compute, window, prof)
    with _generic_attention():
        g = _model(kw, "bf16", 2, P, image_size=(56, 56))
    with pytest.raises(N.VitxError, match="VITX_GENERIC_ATTN: the materialised attention path has no additive score bias") as ei:
        g(img)
    assert ei.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("c", [8, 6])
@pytest.mark.parametrize("hwg", [(8, 8, 4), (6, 12, 3), (6, 9, 1), (4, 4, 4)])
def test_dilated_partition_is_bit_exact(hwg, c):
    """to_dilated / from_dilated against einops on square and rectangular maps (c 8: the float4 path, c 6: the scalar one); the round trip is
    the identity."""
    from einops import rearrange
    H, W, g = hwg
    m = _model(G.kwargs_of("cf_rect"), "fp32", 1, image_size=(24, 48))
    x = np.random.default_rng(H * 100 + W + c).standard_normal((3, H, W, c)).astype(np.float32)
    tok = m.partition(x, g)
    want = rearrange(x, "b (l1 h) (l2 w) d -> (b h w) (l1 l2) d", l1=g, l2=g)
    assert tok.shape == want.shape and np.array_equal(tok, want)
    back = m.partition(tok.reshape(x.shape), g, inverse=True)
    assert np.array_equal(back, x)
    if g > 1 and (H // g > 1 or W // g > 1):
        assert not np.array_equal(tok, rearrange(x, "b (h s1) (w s2) d -> (b h w) (s1 s2) d", s1=g, s2=g))


@pytest.mark.parametrize("dim", [32, 48])
def test_window_round_trips_are_bit_exact_in_the_model(dim):
    """With to_out and fc2 of every pair zeroed each branch adds exact zeros, so what is left between 'embedded' and 'stage' is the two window
    partitions, their inverses and the copies through the engines: the same bits, on rectangular maps."""
    kw = {**G.kwargs_of("cf_rect"), "dim": dim}
    P = R.init_params(R.table_of(kw), seed=3)
    for n in P:
        if n.endswith((".to_out.kernel", ".to_out.bias", ".fc2.kernel", ".fc2.bias")):
            P[n] = np.zeros_like(P[n])
    img, _ = _inputs(kw, (24, 48), 3, 7)
    m = _model(kw, "fp32", 3, P)
    m(img)
    for s in range(4):
        emb = m.read(f"embedded.{s}")
        assert np.abs(emb).max() > 0 and np.array_equal(m.read(f"stage.{s}"), emb), s


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_call_sequences_on_one_object(compute):
    """Batch 3 -> 1 -> 3 on one object, a second backward, then an image of another size (the handle is created again, the weights are kept)
    and batch 1: every gradient against the restatement each time, and the second backward gives the bits of the first."""
    kw = G.kwargs_of("cf_bf16" if compute == "bf16" else "cf_rect")
    hw0, hw1 = ((16, 16), (16, 32)) if compute == "bf16" else ((24, 48), (24, 24))
    P = R.init_params(R.table_of(kw), seed=3)
    m = _model(kw, compute, 3, P)
    for step, (hw, b) in enumerate([(hw0, 3), (hw0, 1), (hw0, 3), (hw1, 2), (hw1, 1)]):
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


def test_new_dpb_weights_change_the_logits():
    """set_weights with new dpb weights: the bias is rebuilt on a parameter change, and the logits follow the restatement's."""
    kw, P, img, dl, rl, *_ = _fixture("cf_rect")
    m = _model(kw, "fp32", 2, P)
    before = m(img)
    gate(float(np.abs(before - rl).max()), FP32_GATES[0], "cf_rect logits before")
    P2 = dict(P)
    rng = np.random.default_rng(11)
    for n in P:
        if R.is_dpb(n) and n.endswith("kernel"):
            P2[n] = (P[n] + 0.5 * rng.standard_normal(P[n].shape)).astype(np.float32).astype(np.float64)
    names = [t[0] for t in m._table]
    m.set_weights([np.asarray(P2[n], np.float32) for n in names])
    after = m(img)
    want = R.forward(kw, {n: torch.tensor(v) for n, v in P2.items()}, torch.tensor(img.astype(np.float64))).numpy()
    spread = float(rl.max() - rl.min())
    assert np.abs(after - before).max() > 1e-3 * spread
    print(f"[crossformer:new dpb weights] logits moved {np.abs(after - before).max():.3e} of a spread of {spread:.3e}; against float64 {np.abs(after - want).max():.3e}")
    gate(float(np.abs(after - want).max()), FP32_GATES[0], "cf_rect logits after new dpb weights")
    grads, _ = m.backward(dl)
    for n in names:
        if R.is_dpb(n):
            assert np.all(grads[n] == 0), n


def test_training_with_dropout_is_refused():
    kw = G.kwargs_of("cf_rect")
    m = _model(kw, "fp32", 1)
    img = np.zeros((1, 24, 48, 3), np.float32)
    assert m(img, training=True).shape == (1, 4) and np.array_equal(m(img, training=True), m(img, training=False))
    from vit_tensorflow.crossformer import CrossFormer
    d = CrossFormer(**kw, ff_dropout=0.2, attn_dropout=0.1, max_batch=1)
    with pytest.raises(NotImplementedError, match="ff_dropout"):
        d(img)
    assert d(img, training=False).shape == (1, 4)
