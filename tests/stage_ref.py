"""Float64 references of the single stages of the bf16 ViT block, each with the worst-case rounding bound of that one stage.

Every function takes its inputs exactly as the engine stored them (`vitx_debug_read`), recomputes ONE stage in float64 and returns
`(want, bound)` per element, so the errors of earlier stages do not accumulate and the gate of a stage is the rounding of that stage alone.
The same checks run on a numpy emulation of the kernels (tests/test_stage_bounds_host.py: a correctly rounded computation must pass,
planted defects must fail) and on the GPU's reads (tests/test_gpu_stage_parity.py).

Notation
  U = 2^-8           worst relative error of one round-to-nearest-even bf16 store
  a32(K, S)          4 K 2^-24 S: K-term fp32 accumulation in any order, S = the same sum over absolute values.  The factor 4 is an allowance
                     (the internal rounding of the MFMA unit is not documented), not a fit.
  Wb                 a parameter rounded to bf16 (RNE): the operand copy the engine keeps
Every term of a bound names the rounding point in the kernel source it accounts for.  Terms that the issue's table did not list are marked
"(added)": they were found reading the kernels and are all far below the bf16 terms.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -8
F32 = 2.0 ** -24          # half an fp32 ulp, relative
BF16_TINY = 2.0 ** -126   # (added) a bf16 store below the normal range is rounded on the subnormal grid or flushed to zero: absolute, not relative
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794

try:                      # vectorised erf: scipy when present, else math.erf
    from scipy.special import erf as _erf
except Exception:         # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def erf(x):
    return _erf(np.asarray(x, np.float64))


def a32(K, S):
    return 4.0 * K * F32 * np.asarray(S, np.float64)


def ustore(want):
    """one bf16 store of `want`: U |want|, or the subnormal spacing where that is larger"""
    return U * np.abs(want) + BF16_TINY


# ------------------------------------------------------------------------------------------------ number formats
def bf16_rne(x) -> np.ndarray:
    """float32 -> bf16 (round to nearest even) -> float32, the conversion of `(bf16_t)v` on gfx950."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def bf16_trunc(x) -> np.ndarray:
    a = np.ascontiguousarray(x, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(a.shape)


def bf16_bits(x) -> np.ndarray:
    """the 16-bit pattern of a value that is exactly representable in bf16"""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return (a.view(np.uint32) >> 16).astype(np.uint16).reshape(a.shape)


def bf16_from_bits(b) -> np.ndarray:
    return (np.asarray(b, np.uint32) << 16).astype(np.uint32).view(np.float32)


def f64(x) -> np.ndarray:
    return np.asarray(x, np.float64)


# ------------------------------------------------------------------------------------------------ GELU
def phi(x):
    return 0.5 * (1.0 + erf(f64(x) * SQRT1_2))


def gelu(x):
    x = f64(x)
    return x * phi(x)


def gelu_grad(x):
    x = f64(x)
    return phi(x) + x * INV_SQRT_2PI * np.exp(-0.5 * x * x)


GELU_SUP_D1 = 1.13   # >= sup |gelu'|  (1.1289 at x = sqrt 2)
GELU_SUP_D2 = 0.80   # >= sup |gelu''| (0.7979 at x = 0)

# the LDS table of the fc1 epilogue (gemm_bf16_pipe.hip:28-64): binades 2^-12 .. 2^3 of the bf16 pattern, both ends clamped
GT_LO = (127 - 12) << 7
GT_NE = ((127 + 3) << 7) - GT_LO


def _table_clamp(x):
    """the value whose table entry a pre-activation x reads (gemm_bf16_pipe.hip:430: the index is clamped to the table's binades)"""
    x = f64(x)
    lo, hi = 2.0 ** -12, float(bf16_from_bits(np.array([GT_LO + GT_NE - 1]))[0])
    return np.sign(x) * np.clip(np.abs(x), lo, hi) + (x == 0) * lo


def gelu_apx(x, form: str):
    """Approximation error of gelu as the fc1 epilogue evaluates it, from the figures the source states.
    poly   common.h:77-78: |erf error| <= 4.2e-5 on |x| <= 3.96, 7.5e-5 beyond the clamp, so |gelu error| <= |x| / 2 * that, and <= 1.5e-4 as stated
           (the smaller of two valid bounds; common.h:108 adds one fma rounding, 2^-24 |x|)
    table  gemm_bf16_pipe.hip:31-33: gelu = x * Phi with Phi stored as fp16: relative 2.4e-4 as stated plus the fp16 store (2^-11 relative, 2^-25
           absolute in the subnormal range), and (added) the two clamped ends of the table: |x| |Phi(x) - Phi(clamp x)|
    either the larger of the two (a launch whose tile variant is chosen by the library may take either form per tile)"""
    x = f64(x)
    ax = np.abs(x)
    if form == "poly":
        return np.minimum(1.5e-4, 0.5 * ax * np.where(ax <= 3.96, 4.2e-5, 7.5e-5)) + F32 * ax
    if form == "table":
        return ax * (phi(x) * (2.4e-4 + 2.0 ** -11) + 2.0 ** -25) + ax * np.abs(phi(x) - phi(_table_clamp(x)))
    return np.maximum(gelu_apx(x, "poly"), gelu_apx(x, "table"))


def gelu_grad_apx(x, form: str):
    """poly   half the stated erf error (common.h:113: phi = 1/2 + erf / 2) plus x pdf(x) times one fp32 ulp of the hardware exp2 (common.h:114) and
           (added) the three fp32 roundings of its argument x^2 / 2 * -log2 e, each 2^-24 of the argument
    table  the entry is gelu' of the pattern rounded to bf16 once (covered by the store term); (added) the clamped ends: |gelu'(x) - gelu'(clamp x)|"""
    x = f64(x)
    ax = np.abs(x)
    if form == "poly":
        pdf = ax * INV_SQRT_2PI * np.exp(-0.5 * x * x)
        return 0.5 * np.where(ax <= 3.96, 4.2e-5, 7.5e-5) + pdf * (2.0 ** -23 + 3.0 * F32 * 0.5 * x * x)
    if form == "table":
        return np.abs(gelu_grad(x) - gelu_grad(_table_clamp(x)))
    return np.maximum(gelu_grad_apx(x, "poly"), gelu_grad_apx(x, "table"))


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_f32(x, gamma, beta, eps):
    """float32 two-pass LayerNorm in numpy: what `ln32` is measured against float64 with"""
    x = np.asarray(x, np.float32)
    d = np.float32(x.shape[-1])
    mu = (x.sum(-1, dtype=np.float32) / d).astype(np.float32)
    c = x - mu[:, None]
    var = ((c * c).sum(-1, dtype=np.float32) / d).astype(np.float32)
    rs = (np.float32(1.0) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = c * rs[:, None] * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)
    return y.astype(np.float32), mu, rs


def layernorm_ref(x, gamma, beta, eps, out_bf16: bool):
    """layernorm_fwd_kernel (elementwise.hip:88-129): two-pass statistics in fp32, y = (x - mu) rs gamma + beta stored in T.
    Returns {'y': (want, bound), 'mean': (...), 'rstd': (...)} and the measured ln32 values.
    ln32 is MEASURED, not derived: 4 x the largest error of the float32 numpy LayerNorm above against float64 on the same rows (per case; the
    margin of 4 allows for another reduction order and rsqrtf).  bf16 output adds U |y| for the store (elementwise.hip:125, st4<bf16_t>)."""
    x64, g64, b64 = f64(x), f64(gamma), f64(beta)
    mu = x64.mean(-1)
    var = ((x64 - mu[:, None]) ** 2).mean(-1)
    rs = 1.0 / np.sqrt(var + eps)
    y = (x64 - mu[:, None]) * rs[:, None] * g64 + b64
    y32, mu32, rs32 = layernorm_f32(x, gamma, beta, eps)
    ln32 = {"y": 4.0 * float(np.abs(y32 - y).max()), "mean": 4.0 * float(np.abs(mu32 - mu).max()), "rstd": 4.0 * float(np.abs(rs32 - rs).max())}
    yb = np.full(y.shape, ln32["y"]) + (ustore(y) if out_bf16 else 0.0)
    return {"y": (y, yb), "mean": (mu, np.full(mu.shape, ln32["mean"])), "rstd": (rs, np.full(rs.shape, ln32["rstd"]))}, ln32


# ------------------------------------------------------------------------------------------------ Dense
def dense_ref(a, wb, bias=None, resid=None, out_bf16=True):
    """a [M, K] as stored, wb [K, N] the bf16 operand copy.  Accumulation: fp32 over K in the MFMA units (gemm_bf16*.hip), bias and residual added
    in fp32 (epilogue.h:64-66,104): a32(K + 2, sum |a| |wb| + |bias| + |resid|).  A T output adds U |want| (epilogue.h:71, st4<bf16_t>)."""
    a, wb = f64(a), f64(wb)
    want = a @ wb
    mag = np.abs(a) @ np.abs(wb)
    extra = 0
    if bias is not None:
        want = want + f64(bias)
        mag = mag + np.abs(f64(bias))
        extra += 1
    if resid is not None:
        want = want + f64(resid)
        mag = mag + np.abs(f64(resid))
        extra += 1
    bound = a32(a.shape[1] + extra, mag)
    if out_bf16:
        bound = bound + ustore(want)
    return want, bound


def bf16_round_reach(h, e):
    """h is a float64 value that the kernel holds in fp32 within +-e and then rounds to bf16 (RNE): the farthest the stored value can lie from h.
    Rounding is monotone, so the extremes are the roundings of the two ends of the interval; never more than U |h| + e (+ the ends' own fp32
    conversion here), and far less where h sits on a bf16 value, as in the GELU sweep."""
    h, e = f64(h), f64(e) + 2.0 * F32 * np.abs(f64(h))
    lo, hi = f64(bf16_rne((h - e).astype(np.float32))), f64(bf16_rne((h + e).astype(np.float32)))
    return np.maximum(np.abs(lo - h), np.abs(hi - h))


def fc1_gelu_ref(y2, wb, bias, form: str):
    """EPI_BIAS_GELU (epilogue.h:78-90, gemm_bf16_pipe.hip:400-473): h = acc + bias is rounded to bf16 BEFORE the activation (epilogue.h:85,171,228),
    so the stored h lies within dh = bf16_round_reach(h, a32(dim + 1, ...)) <= U |h| + a32 of the float64 h; act = bf16(gelu(h)), hpre = bf16(gelu'(h))
    in the bf16 mode.  Returns {'act': ..., 'hpre': ...} and h."""
    y2, wb, bias = f64(y2), f64(wb), f64(bias)
    h = y2 @ wb + bias
    dh = bf16_round_reach(h, a32(y2.shape[1] + 1, np.abs(y2) @ np.abs(wb) + np.abs(bias)))
    hs = np.sign(h) * (np.abs(h) + dh)     # the approximation terms are taken at both ends of h's own interval
    g, gd = gelu(h), gelu_grad(h)
    gb = ustore(g) + GELU_SUP_D1 * dh + np.maximum(gelu_apx(hs, form), gelu_apx(h, form))
    gdb = ustore(gd) + GELU_SUP_D2 * dh + np.maximum(gelu_grad_apx(hs, form), gelu_grad_apx(h, form))
    return {"act": (g, gb), "hpre": (gd, gdb)}, h


# ------------------------------------------------------------------------------------------------ attention
def split_qkv(qkv, b, n, heads, dh):
    """packed [b n, 3 h dh] as the to_qkv Dense emits it -> q, k, v [b, h, n, dh]"""
    t = f64(qkv).reshape(b, n, 3, heads, dh).transpose(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def merge_heads(x):
    b, h, n, dh = x.shape
    return x.transpose(0, 2, 1, 3).reshape(b * n, h * dh)


def attn_scores(q, k, scale):
    s = scale * np.einsum("bhid,bhjd->bhij", q, k)
    sabs = scale * np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k))
    # (added) relative error of one p = 2^(s log2e - m): the fp32 score (a32 over the 64 products, attn_bf16.hip:109-113), the fp32 roundings of
    # the scaled, shifted exponent (attn_bf16.hip:120, :290, :406 -- each 2^-24 of |s| or of |lse|) and the hardware exp2 (fast_exp2), 2^-22 together
    return s, a32(64, sabs)


def attn_fwd_ref(qkv, b, n, heads, dh, scale, drop_key=None, swap_keys=None):
    """attn_fwd_kernel (attn_bf16.hip:168-257) and attn_stream_fwd: o = sum_j bf16(p_j) v_j / sum_j p_j, o stored as bf16.
      U |want|                      the bf16 store of o (attn_bf16.hip:249)
      2U(1+U) M                     p rounded to bf16 for the PV product (pack8, attn_bf16.hip:129) while the row sum takes the unrounded p (:127);
                                    M = sum_j P_ij |v_jd|.  2U covers a kernel that sums either the rounded or the unrounded p
      a32(n + 64, M)                fp32 accumulation of PV over the keys, the row sum, the 1 / l multiply (:241-249), the streamed form's rescaling
      2 ds_i M  (added)             the relative error ds of p itself (attn_scores), which does not cancel between numerator and row sum
    lse: a32(64, sum |q| |k|) scale + 2^-20  (:242: m + log2f(l), two fp32 roundings of a value of a few units)
    drop_key / swap_keys: deliberately wrong references (the tests show that the gate rejects them)."""
    q, k, v = split_qkv(qkv, b, n, heads, dh)
    s, serr = attn_scores(q, k, scale)
    if drop_key is not None:
        s = s.copy()
        s[..., drop_key] = -np.inf
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    P = p / l
    lse = (m + np.log(l))[..., 0]
    vv = v
    if swap_keys is not None:
        j0, j1 = swap_keys
        vv = v.copy()
        vv[:, :, [j0, j1]] = v[:, :, [j1, j0]]
    o = np.einsum("bhij,bhjd->bhid", P, vv)
    M = np.einsum("bhij,bhjd->bhid", P, np.abs(v))
    ds = serr.max(-1, keepdims=True) + 2.0 ** -22 * (1.0 + np.where(np.isfinite(s), np.abs(s), 0.0).max(-1, keepdims=True))
    bound = ustore(o) + 2.0 * U * (1.0 + U) * M + a32(n + 64, M) + 2.0 * ds * M
    lse_b = serr.max(-1) + 2.0 ** -20
    aux = {"P": P, "v": v, "M": M, "bound_bhid": bound}
    return {"attn_out": (merge_heads(o), merge_heads(bound)), "lse": (lse.reshape(b * heads, n), lse_b.reshape(b * heads, n))}, aux


def attn_bwd_ref(qkv, o, d_o, lse, b, n, heads, dh, scale, no_D=False):
    """attn_bwd_dq_kernel / attn_bwd_dkv_kernel (attn_bf16.hip:259-509), attn_stream_bwd.  P is recomputed from the STORED lse, D from the STORED o:
      D = sum_d dO o (:326-332, fp32)   dP = dO v^T (:280-285, fp32 MFMA)   dS = P (dP - D) scale rounded to bf16 (:296-299, :408-411)
      dV = bf16(P)^T dO (:411-415)      dQ = dS k (:301)                   dK = dS^T q (:416), each stored as bf16 (:347, :426)
    bounds  dV: U |want| + U sum_i P_ij |dO_id|  (store; P rounded)
            dQ: U |want| + 2U scale sum_j P_ij (|dP_ij| + |D_i|) |k_jd|   (store; 2U for P and dS both rounded -- these kernels round dS only)
            dK: likewise over i with |q_id|
            each plus the fp32 terms: a32 over the contraction, and (added) the fp32 errors of P (attn_scores + the stored lse's own rounding),
            of dP (a32 over 64 products) and of D (a32 over 64 products) carried through dS."""
    q, k, v = split_qkv(qkv, b, n, heads, dh)
    O = f64(o).reshape(b, n, heads, dh).transpose(0, 2, 1, 3)
    dO = f64(d_o).reshape(b, n, heads, dh).transpose(0, 2, 1, 3)
    L = f64(lse).reshape(b, heads, n)[..., None]
    s, serr = attn_scores(q, k, scale)
    P = np.exp(s - L)
    relP = serr + 2.0 ** -22 * (1.0 + np.abs(s) + np.abs(L))
    D = (dO * O).sum(-1, keepdims=True)
    eD = a32(64, (np.abs(dO) * np.abs(O)).sum(-1, keepdims=True))
    dP = np.einsum("bhid,bhjd->bhij", dO, v)
    edP = a32(64, np.einsum("bhid,bhjd->bhij", np.abs(dO), np.abs(v)))
    dS = P * (dP - (0.0 if no_D else D))
    # fp32-level error of one dS element, and its bf16 rounding budget
    dS_f32 = relP * np.abs(dS) + P * (edP + eD) + 3.0 * F32 * np.abs(dS)
    dS_mag = P * (np.abs(dP) + np.abs(D))
    dV = np.einsum("bhij,bhid->bhjd", P, dO)
    MV = np.einsum("bhij,bhid->bhjd", P, np.abs(dO))
    dVb = ustore(dV) + U * MV + a32(n, MV) + np.einsum("bhij,bhid->bhjd", relP * P, np.abs(dO))
    dQ = scale * np.einsum("bhij,bhjd->bhid", dS, k)
    dQb = (ustore(dQ) + 2.0 * U * scale * np.einsum("bhij,bhjd->bhid", dS_mag, np.abs(k))
           + scale * np.einsum("bhij,bhjd->bhid", dS_f32, np.abs(k)) + a32(n, scale * np.einsum("bhij,bhjd->bhid", np.abs(dS), np.abs(k))))
    dK = scale * np.einsum("bhij,bhid->bhjd", dS, q)
    dKb = (ustore(dK) + 2.0 * U * scale * np.einsum("bhij,bhid->bhjd", dS_mag, np.abs(q))
           + scale * np.einsum("bhij,bhid->bhjd", dS_f32, np.abs(q)) + a32(n, scale * np.einsum("bhij,bhid->bhjd", np.abs(dS), np.abs(q))))

    def pack(a, c, e):
        return np.stack([a, c, e], 0).transpose(1, 3, 0, 2, 4).reshape(b * n, 3 * heads * dh)
    aux = {"P": P, "dP": dP, "D": D, "k": k, "dQb": dQb, "scale": scale}
    return (pack(dQ, dK, dV), pack(dQb, dKb, dVb)), aux


# ------------------------------------------------------------------------------------------------ weight and parameter gradients
def wgrad_ref(x, dy):
    """dW [in, out] = x^T dy (gemm_bf16_tn.hip: both operands as stored, fp32 accumulation over the rows, fp32 output, possibly as split partial sums
    added in fp32): a32(rows, |x|^T |dy|)"""
    x, dy = f64(x), f64(dy)
    return x.T @ dy, a32(x.shape[0], np.abs(x).T @ np.abs(dy))


def colsum_ref(dy):
    """bias gradients: fp32 column sums over the rows (epilogue.h:137-138 / colsum_kernel / layernorm_bwd_kernel's `as`): a32(rows, sum |dy|)"""
    dy = f64(dy)
    return dy.sum(0), a32(dy.shape[0], np.abs(dy).sum(0))


def ln_param_grad_ref(dy, x, mean, rstd):
    """layernorm_bwd_kernel (elementwise.hip:261-263): xhat = (x - mean) rstd from the STORED statistics (two fp32 roundings), dgamma = sum dy xhat,
    dbeta = sum dy, per-wave fp32 sums combined in fixed order: a32(rows + 2, ...)"""
    dy, x = f64(dy), f64(x)
    xh = (x - f64(mean)[:, None]) * f64(rstd)[:, None]
    r = dy.shape[0]
    return ((dy * xh).sum(0), a32(r + 2, (np.abs(dy) * np.abs(xh)).sum(0))), (dy.sum(0), a32(r, np.abs(dy).sum(0)))


# ------------------------------------------------------------------------------------------------ the whole block, stage by stage
PFX = "transformer.0."


def block_checks(reads: dict, grads, params: dict, d_out, b: int, n: int, heads: int, dh: int, eps: float, gelu_form="either", gelu_rows=None,
                 backward=True, ln_out_bf16=True, weights_bf16=True):
    """Every stage and link of one block from the engine's own reads: a list of (name, got, want, bound) and the measured ln32 values.
    gelu_form: 'poly' | 'table' | 'either'; gelu_rows: with 'table', the number of leading rows that take the table (the interior tiles), the rest
    take the polynomial.  weights_bf16=False: the Dense operand is the fp32 parameter itself (VITX_GENERIC_GEMM=1: engine.hip, dense_fwd /
    dense_dgrad hand the fp32-FMA kernel `dense_w`, not the bf16 operand copy)."""
    P = {k[len(PFX):]: np.asarray(v, np.float32) for k, v in params.items() if k.startswith(PFX)}
    Wb = {k: f64(bf16_rne(v) if weights_bf16 else v) for k, v in P.items() if k.endswith("kernel")}
    rows, dim = b * n, P["attn.norm.gamma"].shape[0]
    inner, mlp = heads * dh, P["mlp.fc1.bias"].shape[0]
    R = {k: f64(v) for k, v in reads.items()}
    shp = {"x_in": dim, "y1": dim, "qkv": 3 * inner, "attn_out": inner, "x_mid": dim, "y2": dim, "hpre": mlp, "act": mlp, "x_out": dim,
           "d_hpre": mlp, "d_attn_out": inner, "d_qkv": 3 * inner, "d_y1": dim}
    for k, c in shp.items():
        if k in R:
            R[k] = R[k].reshape(rows, c)
    scale = 1.0 / math.sqrt(dh)
    out, ln32 = [], {}

    def add(name, got, wb):
        out.append((name, f64(got).reshape(wb[0].shape), wb[0], wb[1]))

    for i, (src, y, pre) in enumerate((("x_in", "y1", "attn.norm."), ("x_mid", "y2", "mlp.norm.")), 1):
        ln, m = layernorm_ref(reads[src].reshape(rows, dim), P[pre + "gamma"], P[pre + "beta"], eps, ln_out_bf16)
        ln32[f"ln{i}"] = m
        add(f"ln{i}.y", R[y], ln["y"])
        add(f"ln{i}.mean", R[f"mean{i}"], ln["mean"])
        add(f"ln{i}.rstd", R[f"rstd{i}"], ln["rstd"])
    add("to_qkv", R["qkv"], dense_ref(R["y1"], Wb["attn.to_qkv.kernel"]))
    at, _ = attn_fwd_ref(R["qkv"], b, n, heads, dh, scale)
    add("attn", R["attn_out"], at["attn_out"])
    if "lse" in R:
        add("lse", R["lse"].reshape(b * heads, n), at["lse"])
    add("to_out+resid", R["x_mid"], dense_ref(R["attn_out"], Wb["attn.to_out.kernel"], P["attn.to_out.bias"], R["x_in"], out_bf16=False))
    if gelu_form == "table" and gelu_rows is not None and gelu_rows < rows:
        top, _ = fc1_gelu_ref(R["y2"][:gelu_rows], Wb["mlp.fc1.kernel"], P["mlp.fc1.bias"], "table")
        bot, _ = fc1_gelu_ref(R["y2"][gelu_rows:], Wb["mlp.fc1.kernel"], P["mlp.fc1.bias"], "poly")
        fc1 = {k: (np.concatenate([top[k][0], bot[k][0]]), np.concatenate([top[k][1], bot[k][1]])) for k in top} if gelu_rows else bot
    else:
        fc1, _ = fc1_gelu_ref(R["y2"], Wb["mlp.fc1.kernel"], P["mlp.fc1.bias"], gelu_form)
    add("fc1+gelu.act", R["act"], fc1["act"])
    add("fc1+gelu.gelu'", R["hpre"], fc1["hpre"])
    add("fc2+resid", R["x_out"], dense_ref(R["act"], Wb["mlp.fc2.kernel"], P["mlp.fc2.bias"], R["x_mid"], out_bf16=False))
    if not backward:
        return out, ln32

    G = {k[len(PFX):]: f64(v) for k, v in grads.items() if k.startswith(PFX)}
    dout = np.asarray(d_out, np.float32).reshape(rows, dim)
    g = f64(bf16_rne(dout))     # the bf16 copy of the residual gradient every GEMM of the backward reads (engine.hip, launch_convert into g_lp)
    # fc2 input gradient + EPI_GELU_BWD (epilogue.h:116-138, :193-197, :235-240): acc * stored gelu'(h), one bf16 store
    da = g @ Wb["mlp.fc2.kernel"].T
    want = da * R["hpre"]
    add("d_hpre", R["d_hpre"], (want, ustore(want) + a32(dim, np.abs(g) @ np.abs(Wb["mlp.fc2.kernel"]).T) * np.abs(R["hpre"])))
    add("dW fc2", G["mlp.fc2.kernel"], wgrad_ref(R["act"], g))
    add("db fc2", G["mlp.fc2.bias"], colsum_ref(dout))   # column sums of the fp32 residual gradient, taken on the LayerNorm 2 VJP pass (engine.hip, fc2_bias_in_ln)
    add("dW fc1", G["mlp.fc1.kernel"], wgrad_ref(R["y2"], R["d_hpre"]))
    add("db fc1", G["mlp.fc1.bias"], colsum_ref(R["d_hpre"]))   # of the values as stored (epilogue.h:137)
    ab, _ = attn_bwd_ref(R["qkv"], R["attn_out"], R["d_attn_out"], R["lse"], b, n, heads, dh, scale)
    add("attn_bwd.d_qkv", R["d_qkv"], ab)
    add("dW to_qkv", G["attn.to_qkv.kernel"], wgrad_ref(R["y1"], R["d_qkv"]))
    add("d_y1", R["d_y1"], dense_ref(R["d_qkv"], Wb["attn.to_qkv.kernel"].T))
    (dg, db_) = ln_param_grad_ref(R["d_y1"], R["x_in"], R["mean1"], R["rstd1"])
    add("dgamma ln1", G["attn.norm.gamma"], dg)
    add("dbeta ln1", G["attn.norm.beta"], db_)
    return out, ln32


def worst_ratio(got, want, bound):
    """largest err / bound over the elements; inf where a value is not finite"""
    got, want, bound = f64(got), f64(want), f64(bound)
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs shared by the host and the GPU tests
DIM, HEADS, DH, MLP, EPS = 128, 2, 64, 256, 1e-3
NS = (1, 2, 63, 64, 65, 96, 97, 224, 225, 288)          # both sides of every padded-key instance of attn_bf16.hip (64, 96, 224, 288)
CASES = [(2, n) for n in NS] + [(3, 97)]


def tau_for(n: int) -> float:
    """Sharp regime: W_q = tau W_k makes token i its own strongest key.  With keys of squared norm about 64 per head the diagonal logit is about
    8 tau and the others about N(0, tau^2), so P_ii ~ e^(8 tau) / (e^(8 tau) + (n - 1) e^(tau^2 / 2)); tau solves 8 tau - tau^2 / 2 = ln(0.82 (n - 1)),
    i.e. P_ii ~ 0.45: peaked enough that each key matters, far from saturated."""
    if n <= 2:
        return 0.05
    return 8.0 - math.sqrt(64.0 - 2.0 * math.log(0.82 * (n - 1.0)))


def _orth(r, m):
    q, _ = np.linalg.qr(r.standard_normal((m, m)))
    return q


def make_params(regime: str, n: int, seed: int = 0, dim=DIM, heads=HEADS, dh=DH, mlp=MLP) -> dict:
    """transformer.0.* parameters.
    'random'     N(0,1) kernels scaled by 1 / sqrt(fan_in) (unit-variance pre-activations), random LayerNorm and bias vectors.
    'sharp'      W_k, W_v and W_out orthogonal (every key, value and output-gradient row keeps the norm of its LayerNorm row, so the rows of the
                 softmax are evenly peaked), W_q = tau_for(n) W_k, and a quarter-size fc2 kernel so that the output gradient chosen by
                 make_tokens reaches the attention mostly through the residual.
    'saturated'  'sharp' with tau four times larger."""
    r = np.random.default_rng(1000 + seed)
    inner = heads * dh
    p = {
        "attn.norm.gamma": 1.0 + 0.1 * r.standard_normal(dim), "attn.norm.beta": 0.1 * r.standard_normal(dim),
        "attn.to_qkv.kernel": r.standard_normal((dim, 3 * inner)) / math.sqrt(dim),
        "attn.to_out.kernel": r.standard_normal((inner, dim)) / math.sqrt(inner), "attn.to_out.bias": 0.1 * r.standard_normal(dim),
        "mlp.norm.gamma": 1.0 + 0.1 * r.standard_normal(dim), "mlp.norm.beta": 0.1 * r.standard_normal(dim),
        "mlp.fc1.kernel": r.standard_normal((dim, mlp)) / math.sqrt(dim), "mlp.fc1.bias": 0.5 * r.standard_normal(mlp),
        "mlp.fc2.kernel": r.standard_normal((mlp, dim)) / math.sqrt(mlp), "mlp.fc2.bias": 0.1 * r.standard_normal(dim),
    }
    if regime in ("sharp", "saturated"):
        assert inner == dim
        tau = tau_for(n) * (4.0 if regime == "saturated" else 1.0)
        w = p["attn.to_qkv.kernel"]
        w[:, inner:2 * inner] = _orth(r, dim)
        w[:, 2 * inner:] = _orth(r, dim)
        w[:, :inner] = tau * w[:, inner:2 * inner]
        p["attn.to_out.kernel"] = _orth(r, dim)
        p["mlp.fc2.kernel"] *= 0.25
    else:
        assert regime == "random"
    return {PFX + k: v.astype(np.float32) for k, v in p.items()}


def make_tokens(b: int, n: int, seed: int = 0, dim=DIM, params=None, regime="random", dh=DH):
    """tokens and d(out).  'random': both N(0,1).
    Sharp regimes: token i is (a_i | b_i) W_k^T with a_i, b_i random directions of norm sqrt(dh), so that after LayerNorm 1 the key of every head has
    nearly the same norm and P_ii sits close to the value tau_for aims at in every row; d(out) row i is v_i W_out plus a quarter of noise (v from
    the float64 LayerNorm and Dense of the tokens), so that d(attn_out)_i = d(out)_i W_out^T points along v_i and dP_ii = |v_i|^2 stands out of
    dP_ij and of D_i = sum_j P_ij dP_ij -- which is what lets EVERY key carry a dQ term far above the bound of some element."""
    r = np.random.default_rng(2000 + 17 * seed + 1000 * b + n)
    x = r.standard_normal((b, n, dim)).astype(np.float32)
    d = r.standard_normal((b, n, dim))
    if regime in ("sharp", "saturated"):
        wqkv, wout = f64(params[PFX + "attn.to_qkv.kernel"]), f64(params[PFX + "attn.to_out.kernel"])
        ab = r.standard_normal((b * n, dim // dh, dh))
        ab *= math.sqrt(dh) / np.linalg.norm(ab, axis=-1, keepdims=True)
        x = (ab.reshape(b * n, dim) @ wqkv[:, dim:2 * dim].T).astype(np.float32).reshape(b, n, dim)
        g, be = f64(params[PFX + "attn.norm.gamma"]), f64(params[PFX + "attn.norm.beta"])
        x64 = f64(x).reshape(b * n, dim)
        mu = x64.mean(-1, keepdims=True)
        y1 = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + EPS) * g + be
        d = ((y1 @ wqkv[:, 2 * dim:]) @ wout).reshape(b, n, dim) + 0.25 * d
    return x, d.astype(np.float32)


# the GELU sweep: a tiny fc1 kernel and a ramp of bf16 patterns in fc1.bias, so that the pre-activation of column c is the pattern c
SWEEP_MLP = 1024


def gelu_sweep_bias(mlp=SWEEP_MLP) -> np.ndarray:
    """bf16 patterns covering every binade from 2^-13 to 2^4 in both signs (mantissas 0, 1, 2, 31, 63, 64, 65, 96, 126, 127 of each), the values
    adjacent to 3.96 (the polynomial clamp), to 8 and to 2^-12 (the table ends), and 0; the rest of the columns repeat the ramp with other mantissas."""
    pats = []
    mans = (0, 1, 2, 31, 63, 64, 65, 96, 126, 127)
    for e in range(127 - 13, 127 + 5):
        for mnt in mans:
            pats.append((e << 7) | mnt)
    near = []
    for v in (3.96, 8.0, 2.0 ** -12):
        c = int(bf16_bits(bf16_rne(np.array([v], np.float32)))[0])
        near += [c - 2, c - 1, c, c + 1, c + 2]
    pats += near
    pats = sorted(set(pats))
    both = pats + [p | 0x8000 for p in pats] + [0]
    extra = np.random.default_rng(7)
    while len(both) < mlp:
        e = int(extra.integers(127 - 13, 127 + 5))
        both.append((e << 7) | int(extra.integers(0, 128)) | (int(extra.integers(0, 2)) << 15))
    assert len(both) == mlp, len(both)
    return bf16_from_bits(np.array(both, np.uint32)).astype(np.float32)


def make_sweep_params(seed: int = 0) -> dict:
    p = make_params("random", 97, seed, mlp=SWEEP_MLP)
    r = np.random.default_rng(3000 + seed)
    p[PFX + "mlp.fc1.kernel"] = (r.standard_normal((DIM, SWEEP_MLP)) * 2.0 ** -33).astype(np.float32)   # |y2 W| ~ 1e-9: far below half an ulp of 2^-13
    p[PFX + "mlp.fc1.bias"] = gelu_sweep_bias()
    return p


def ln_edge_inputs(dim, rows=8) -> dict:
    """LayerNorm edge rows, one kind per image: a common offset of 30 sigma, rows of variance exactly 0, rows with one 1e4 outlier"""
    r = np.random.default_rng(5)
    off = (30.0 + r.standard_normal((rows, dim))).astype(np.float32)
    const = np.repeat(np.arange(rows, dtype=np.float32)[:, None] * 0.5 + 3.0, dim, 1)
    outl = r.standard_normal((rows, dim)).astype(np.float32)
    outl[np.arange(rows), r.integers(0, dim, rows)] = 1e4
    return {"offset 30 sigma": off, "variance 0": const, "one 1e4 outlier": outl}
