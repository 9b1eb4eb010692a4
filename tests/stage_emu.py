"""A numpy emulation of the bf16 ViT block: float32 accumulation, bf16 round-to-nearest-even at the points the kernels round (stage_ref.py names
them).  It stands in for the GPU in tests/test_stage_bounds_host.py: a correctly rounded computation must pass every gate of stage_ref.block_checks,
and each planted `defect` must break the gate of the stage it sits in."""
from __future__ import annotations

import math

import numpy as np

import stage_ref as sr
from stage_ref import PFX, bf16_rne, bf16_trunc

f32 = np.float32
LOG2E = f32(1.44269504088896340736)

ERF_COEF = (-4.356138932e-07, 1.643961321e-05, -2.719887553e-04, 2.634852515e-03, -1.693103523e-02, 7.756211587e-02, -2.648631880e-01,
            7.977257765e-01)   # common.h:94-101


def erf_poly(x, coef=ERF_COEF):
    x = np.asarray(x, f32)
    u0 = x * x * f32(0.5)
    u = np.minimum(u0, f32(7.84))
    p = np.full(x.shape, f32(coef[0]), f32)
    for c in coef[1:]:
        p = p * u + f32(c)
    return np.clip(p * x, f32(-1), f32(1)), u0


def gelu_poly(h, coef=ERF_COEF):
    """gelu_both_fast (common.h:119-127) on the bf16-rounded pre-activation"""
    e, u0 = erf_poly(h, coef)
    hx = h * f32(0.5)
    g = hx * e + hx
    ph = e * f32(0.5) + f32(0.5)
    gd = (h * f32(0.39894228040143267794)) * np.exp2(u0 * f32(-1.44269504088896340736)).astype(f32) + ph
    return g.astype(f32), gd.astype(f32)


_TABLE = None


def gelu_table():
    """the table as gemm_bf16_pipe.hip:45-54 builds it: (Phi as fp16, gelu' as bf16) per bf16 pattern of 2^-12 <= |x| < 8"""
    global _TABLE
    if _TABLE is None:
        bits = np.concatenate([np.arange(sr.GT_NE, dtype=np.uint32) + sr.GT_LO, (np.arange(sr.GT_NE, dtype=np.uint32) + sr.GT_LO) | 0x8000])
        x = sr.bf16_from_bits(bits).astype(np.float64)
        ph = sr.phi(x).astype(f32).astype(np.float16).astype(f32)
        gd = bf16_rne(sr.gelu_grad(x).astype(f32))
        _TABLE = (ph, gd)
    return _TABLE


def gelu_tab(h, off=0):
    """the table form (gemm_bf16_pipe.hip:426-442); off: the planted defect, every read one entry off"""
    ph, gd = gelu_table()
    bits = sr.bf16_bits(h).astype(np.int64)
    t = np.clip((bits & 0x7FFF) - sr.GT_LO, 0, sr.GT_NE - 1)
    t = np.clip(t + off, 0, sr.GT_NE - 1) + (bits >> 15) * sr.GT_NE
    return (np.asarray(h, f32) * ph[t]).astype(f32), gd[t]


def emulate_block(params, x, d_out, b, n, heads=sr.HEADS, dh=sr.DH, eps=sr.EPS, gelu_form="poly", gelu_rows=None, defect=None, defect_arg=None):
    """-> (reads, grads) in the form of vitx_debug_read / transformer.backward"""
    P = {k[len(PFX):]: np.asarray(v, f32) for k, v in params.items() if k.startswith(PFX)}
    Wb = {k: bf16_rne(v) for k, v in P.items() if k.endswith("kernel")}
    dim = P["attn.norm.gamma"].shape[0]
    rows, inner = b * n, heads * dh
    scale = f32(1.0 / math.sqrt(dh))
    R, G = {}, {}

    def ln(xin, pre, dm1=False):
        d = f32(xin.shape[1])
        mu = (xin.sum(1, dtype=f32) / d).astype(f32)
        c = xin - mu[:, None]
        var = ((c * c).sum(1, dtype=f32) / (d - f32(1) if dm1 else d)).astype(f32)
        rs = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
        return bf16_rne(c * rs[:, None] * P[pre + "gamma"] + P[pre + "beta"]), mu, rs

    x = np.asarray(x, f32).reshape(rows, dim)
    R["x_in"] = x
    R["y1"], R["mean1"], R["rstd1"] = ln(x, "attn.norm.", dm1=defect == "var_dm1")
    acc = R["y1"] @ Wb["attn.to_qkv.kernel"]
    if defect == "dense_drop_k":
        acc = R["y1"][:, :-1] @ Wb["attn.to_qkv.kernel"][:-1]
    R["qkv"] = bf16_trunc(acc) if defect == "trunc" else bf16_rne(acc)

    t = R["qkv"].reshape(b, n, 3, heads, dh).transpose(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    s = np.einsum("bhid,bhjd->bhij", q, k).astype(f32)
    sv = s.copy()
    if defect == "drop_last_key":
        sv[..., n - 1] = -np.inf
    if defect == "drop_key":
        sv[..., defect_arg] = -np.inf
    m = sv.max(-1, keepdims=True) * (scale * LOG2E)
    p = np.exp2(sv * (scale * LOG2E) - m).astype(f32)
    l = p.sum(-1, keepdims=True, dtype=f32)
    pb = bf16_rne(p)
    vv = v
    if defect == "swap_keys":
        j = defect_arg
        vv = v.copy()
        vv[:, :, [j, j + 1]] = v[:, :, [j + 1, j]]
    o = (np.einsum("bhij,bhjd->bhid", pb, vv).astype(f32) * (f32(1) / l)).astype(f32)
    R["attn_out"] = bf16_rne(o.transpose(0, 2, 1, 3).reshape(rows, inner))
    R["lse"] = ((m + np.log2(l)) * f32(0.69314718055994530942)).astype(f32)[..., 0].reshape(b * heads, n)

    R["x_mid"] = (x + (R["attn_out"] @ Wb["attn.to_out.kernel"] + P["attn.to_out.bias"])).astype(f32)
    R["y2"], R["mean2"], R["rstd2"] = ln(R["x_mid"], "mlp.norm.")
    h = bf16_rne(R["y2"] @ Wb["mlp.fc1.kernel"] + P["mlp.fc1.bias"])
    coef = ERF_COEF
    if defect == "erf_coef":
        i, c = defect_arg
        coef = tuple(c if j == i else cj for j, cj in enumerate(ERF_COEF))
    gp, gdp = gelu_poly(h, coef)
    if gelu_form == "table":
        gt, gdt = gelu_tab(h, 1 if defect == "table_off" else 0)
        top = rows if gelu_rows is None else gelu_rows
        sel = (np.arange(rows) < top)[:, None]
        gp, gdp = np.where(sel, gt, gp), np.where(sel, gdt, gdp)
    R["act"], R["hpre"] = bf16_rne(gp), bf16_rne(gdp)
    R["x_out"] = (R["x_mid"] + (R["act"] @ Wb["mlp.fc2.kernel"] + P["mlp.fc2.bias"])).astype(f32)
    if d_out is None:
        return R, G

    # ---- backward
    dout = np.asarray(d_out, f32).reshape(rows, dim)
    g = bf16_rne(dout)
    R["d_hpre"] = bf16_rne((g @ Wb["mlp.fc2.kernel"].T) * R["hpre"])
    act_w, g_w = (R["act"][:-1], g[:-1]) if defect == "wgrad_drop_row" else (R["act"], g)
    G["mlp.fc2.kernel"] = (act_w.T @ g_w).astype(f32)
    G["mlp.fc2.bias"] = dout.sum(0, dtype=f32)
    G["mlp.fc1.kernel"] = (R["y2"].T @ R["d_hpre"]).astype(f32)
    G["mlp.fc1.bias"] = R["d_hpre"].sum(0, dtype=f32)
    d_y2 = bf16_rne(R["d_hpre"] @ Wb["mlp.fc1.kernel"].T)

    def ln_vjp(dy, xin, mu, rs, gamma):
        xh = (xin - mu[:, None]) * rs[:, None]
        gg = dy * gamma
        s1 = gg.mean(1, dtype=f32)[:, None]
        s2 = (gg * xh).mean(1, dtype=f32)[:, None]
        return (rs[:, None] * (gg - s1 - xh * s2)).astype(f32), (dy * xh).sum(0, dtype=f32), dy.sum(0, dtype=f32)

    dx, _, _ = ln_vjp(d_y2, R["x_mid"], R["mean2"], R["rstd2"], P["mlp.norm.gamma"])
    g_mid = (dout + dx).astype(f32)
    g_lp = bf16_rne(g_mid)
    R["d_attn_out"] = bf16_rne(g_lp @ Wb["attn.to_out.kernel"].T)

    O = R["attn_out"].reshape(b, n, heads, dh).transpose(0, 2, 1, 3)
    dO = R["d_attn_out"].reshape(b, n, heads, dh).transpose(0, 2, 1, 3)
    lse2 = (R["lse"].reshape(b, heads, n)[..., None] * LOG2E).astype(f32)
    Pm = np.exp2(s * (scale * LOG2E) - lse2).astype(f32)
    D = (dO * O).sum(-1, keepdims=True, dtype=f32)
    dP = np.einsum("bhid,bhjd->bhij", dO, v).astype(f32)
    dS = bf16_rne(Pm * ((dP - (f32(0) if defect == "no_D" else D)) * scale))
    dq = np.einsum("bhij,bhjd->bhid", dS, k).astype(f32)
    dk = np.einsum("bhij,bhid->bhjd", dS, q).astype(f32)
    if defect == "no_scale_dk":
        dk = (dk / scale).astype(f32)
    dv = np.einsum("bhij,bhid->bhjd", bf16_rne(Pm), dO).astype(f32)
    R["d_qkv"] = bf16_rne(np.stack([dq, dk, dv], 0).transpose(1, 3, 0, 2, 4).reshape(rows, 3 * inner))
    G["attn.to_qkv.kernel"] = (R["y1"].T @ R["d_qkv"]).astype(f32)
    R["d_y1"] = bf16_rne(R["d_qkv"] @ Wb["attn.to_qkv.kernel"].T)
    _, G["attn.norm.gamma"], G["attn.norm.beta"] = ln_vjp(R["d_y1"], x, R["mean1"], R["rstd1"], P["attn.norm.gamma"])
    return R, {PFX + k: a for k, a in G.items()}
