"""CPU proof of the per-stage gates of tests/test_gpu_stage_parity.py, before the GPU sees them (stage_ref.py holds the references and bounds).

  * a correctly rounded emulation of the block (stage_emu.py: float32 accumulation, bf16 RNE at the kernels' rounding points) is inside every bound
    on every input set the GPU tests use; the largest err / bound per stage is printed;
  * each planted defect in that emulation breaks the gate of its stage;
  * the inputs meet the conditions that make the attention and GELU gates bite (asserted on the float64 reference).

Conditions that cannot hold by arithmetic, and are therefore not asserted:
  * random regime: a near-flat softmax over n keys gives every key a share of about 1 / n of an output, below 20 bounds (20 * 3 U = 0.23) as soon as
    n > 4; the every-key condition is asserted for the sharp, saturated and streamed cases, which exist for that purpose;
  * n = 1: one key, P = 1 and dS = P (dP - D) = 0 exactly, so no dQ term exists; max P = 1 is outside [0.2, 0.95] for the same reason;
  * saturated cases: dS vanishes by construction (the issue asks them to be finite and inside the bounds only).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import stage_emu as se
import stage_ref as sr

ALL = [(b, n, r) for (b, n) in sr.CASES for r in ("random", "sharp")] + [(2, 65, "saturated"), (2, 288, "saturated"), (1, 289, "sharp")]


@functools.lru_cache(maxsize=None)
def emulated(b, n, regime, form="poly", gelu_rows=None):
    P = sr.make_params(regime, n)
    x, d = sr.make_tokens(b, n, params=P, regime=regime)
    R, G = se.emulate_block(P, x, d, b, n, gelu_form=form, gelu_rows=gelu_rows)
    return P, x, d, R, G


def ratios(P, d, R, G, b, n, form="poly", gelu_rows=None, backward=True):
    ch, ln32 = sr.block_checks(R, G, P, d, b, n, sr.HEADS, sr.DH, sr.EPS, form, gelu_rows, backward=backward)
    return {nm: sr.worst_ratio(g, w, bd) for nm, g, w, bd in ch}, ln32


@pytest.mark.parametrize("b,n,regime", ALL)
def test_correctly_rounded_emulation_is_inside_every_bound(b, n, regime):
    P, x, d, R, G = emulated(b, n, regime)
    r, ln32 = ratios(P, d, R, G, b, n)
    print(f"[stage] emulation b={b} n={n} {regime}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("form,rows", [("table", 256), ("table", None), ("poly", None)])
def test_emulation_of_both_gelu_forms_is_inside_the_bounds(form, rows):
    """b = 3, n = 97: with the table the first 256 rows are interior tiles of the 256-row variant, the last 35 take the polynomial"""
    P, x, d, R, G = emulated(3, 97, "random", form, rows)
    r, _ = ratios(P, d, R, G, 3, 97, form, rows, backward=False)
    assert r["fc1+gelu.act"] <= 1.0 and r["fc1+gelu.gelu'"] <= 1.0, r
    r2, _ = ratios(P, d, R, G, 3, 97, "either", None, backward=False)
    assert r2["fc1+gelu.act"] <= 1.0 and r2["fc1+gelu.gelu'"] <= 1.0, r2


# ------------------------------------------------------------------------------------------------ planted defects
def defect_ratio(defect, stage, b=2, n=65, regime="sharp", arg=None, form="poly", params=None):
    P = params or sr.make_params(regime, n)
    x, d = sr.make_tokens(b, n, params=P, regime="random" if params else regime)
    R, G = se.emulate_block(P, x, d, b, n, gelu_form=form, defect=defect, defect_arg=arg)
    r, _ = ratios(P, d, R, G, b, n, form)
    good, _ = ratios(P, d, *se.emulate_block(P, x, d, b, n, gelu_form=form), b, n, form)
    assert all(v <= 1.0 for v in good.values()), good   # the same inputs without the defect pass
    print(f"[stage] defect {defect}: {stage} err / bound = {r[stage]:.2f}")
    return r[stage]


@pytest.mark.parametrize("n", [65, 288])
def test_defect_last_key_dropped(n):
    assert defect_ratio("drop_last_key", "attn", n=n) > 1.0


@pytest.mark.parametrize("j", [2, 34, 62])
def test_defect_two_keys_swapped_inside_a_32_key_group(j):
    assert j // 32 == (j + 1) // 32
    assert defect_ratio("swap_keys", "attn", arg=j) > 1.0


def test_defect_last_k_element_of_a_dense_dropped():
    assert defect_ratio("dense_drop_k", "to_qkv") > 1.0


def test_defect_last_row_of_a_weight_gradient_dropped():
    assert defect_ratio("wgrad_drop_row", "dW fc2") > 1.0


def test_defect_variance_over_d_minus_1():
    assert defect_ratio("var_dm1", "ln1.y") > 1.0
    assert defect_ratio("var_dm1", "ln1.rstd") > 1.0


def test_defect_bf16_truncation_on_a_dense_output():
    assert defect_ratio("trunc", "to_qkv") > 1.0


@pytest.mark.parametrize("i,c", [(7, 7.978257765e-01), (6, -2.649631880e-01), (4, -1.694103523e-02)])
def test_defect_erf_coefficient_changed_in_its_fourth_digit(i, c):
    P = sr.make_sweep_params()
    a = defect_ratio("erf_coef", "fc1+gelu.act", b=3, n=97, arg=(i, c), params=P)
    g = defect_ratio("erf_coef", "fc1+gelu.gelu'", b=3, n=97, arg=(i, c), params=P)
    assert a > 1.0 and g > 1.0, (a, g)


def test_defect_table_read_one_entry_off():
    P = sr.make_sweep_params()
    a = defect_ratio("table_off", "fc1+gelu.act", b=3, n=97, form="table", params=P)
    g = defect_ratio("table_off", "fc1+gelu.gelu'", b=3, n=97, form="table", params=P)
    assert a > 1.0 and g > 1.0, (a, g)


def test_defect_D_missing_from_dS():
    assert defect_ratio("no_D", "attn_bwd.d_qkv") > 1.0


def test_defect_scale_missing_from_dK():
    assert defect_ratio("no_scale_dk", "attn_bwd.d_qkv") > 1.0


# ------------------------------------------------------------------------------------------------ input conditions (on the float64 reference)
SHARP = [(b, n, r) for (b, n, r) in ALL if r != "random"]


@pytest.mark.parametrize("b,n,regime", SHARP)
def test_every_key_matters_in_the_forward(b, n, regime):
    """for every key j there is an output element where key j's own term P_ij |v_jd| is at least 20 bounds of that element"""
    P, x, d, R, G = emulated(b, n, regime)
    _, aux = sr.attn_fwd_ref(R["qkv"], b, n, sr.HEADS, sr.DH, 0.125)
    term = np.einsum("bhij,bhjd->bhijd", aux["P"], np.abs(aux["v"])) / aux["bound_bhid"][:, :, :, None, :]
    best = term.max(axis=(2, 4))                      # [b, h, j]
    print(f"[stage] forward key condition b={b} n={n} {regime}: weakest key has {best.min():.1f} bounds")
    assert best.min() >= 20.0


@pytest.mark.parametrize("b,n,regime", [c for c in SHARP if c[2] == "sharp" and c[1] > 1])
def test_every_key_matters_in_dq_and_rows_are_peaked_not_saturated(b, n, regime):
    P, x, d, R, G = emulated(b, n, regime)
    (_, _), aux = sr.attn_bwd_ref(R["qkv"], R["attn_out"], R["d_attn_out"], R["lse"], b, n, sr.HEADS, sr.DH, 0.125)
    dS = aux["P"] * np.abs(aux["dP"] - aux["D"])
    term = aux["scale"] * np.einsum("bhij,bhjd->bhijd", dS, np.abs(aux["k"])) / aux["dQb"][:, :, :, None, :]
    best = term.max(axis=(2, 4))
    mx = aux["P"].max(-1)
    frac = float(((mx >= 0.2) & (mx <= 0.95)).mean())
    print(f"[stage] dQ key condition b={b} n={n}: weakest key has {best.min():.1f} bounds; rows with max P in [0.2, 0.95]: {frac:.3f}")
    assert best.min() >= 20.0
    assert frac >= 0.9


def test_gelu_sweep_covers_the_binades_the_clamp_and_the_table_ends():
    P = sr.make_sweep_params()
    x, _ = sr.make_tokens(3, 97)
    R, _ = se.emulate_block(P, x, None, 3, 97)
    Wb = sr.f64(sr.bf16_rne(P[sr.PFX + "mlp.fc1.kernel"]))
    _, h = sr.fc1_gelu_ref(R["y2"], Wb, P[sr.PFX + "mlp.fc1.bias"], "poly")
    bias = sr.gelu_sweep_bias()
    nz = bias != 0                                    # (the one zero column holds whatever tiny value the kernel product has)
    hb = sr.bf16_rne(h.astype(np.float32))
    assert (hb[:, nz] == bias[None, nz]).all(), "the tiny kernel moved a pre-activation off its pattern"
    pats = set(int(v) for v in sr.bf16_bits(bias[nz]))
    for sign in (0, 0x8000):
        for e in range(127 - 13, 127 + 5):            # every binade from 2^-13 to 2^4
            assert any((p & 0x8000) == sign and ((p & 0x7FFF) >> 7) == e for p in pats), (sign, e)
        for v in (3.96, 8.0, 2.0 ** -12):             # the bf16 values on both sides of the polynomial clamp and of both table ends
            c = int(sr.bf16_bits(sr.bf16_rne(np.array([v], np.float32)))[0])
            assert {sign | (c - 1), sign | c, sign | (c + 1)} <= pats, (sign, v)


def test_gelu_sweep_emulation_is_inside_the_bounds_in_both_forms():
    P = sr.make_sweep_params()
    x, _ = sr.make_tokens(3, 97)
    for form, rows in (("poly", None), ("table", 256)):
        R, _ = se.emulate_block(P, x, None, 3, 97, gelu_form=form, gelu_rows=rows)
        r, _ = ratios(P, None, R, None, 3, 97, form, rows, backward=False)
        ra, rg = r["fc1+gelu.act"], r["fc1+gelu.gelu'"]
        print(f"[stage] gelu sweep emulation {form}: act {ra:.3f} gelu' {rg:.3f}")
        assert r["fc1+gelu.act"] <= 1.0 and r["fc1+gelu.gelu'"] <= 1.0, (form, r)


def test_fp16_phi_table_error_against_the_figure_in_the_source():
    """gemm_bf16_pipe.hip states the error of the stored Phi; the table is rebuilt here as the host code builds it and compared with erf"""
    ph, _ = se.gelu_table()
    bits = np.concatenate([np.arange(sr.GT_NE, dtype=np.uint32) + sr.GT_LO, (np.arange(sr.GT_NE, dtype=np.uint32) + sr.GT_LO) | 0x8000])
    x = sr.bf16_from_bits(bits).astype(np.float64)
    want = sr.phi(x)
    err = np.abs(ph - want)
    print(f"[stage] fp16 Phi table: max abs error {err.max():.3e}, max relative error where Phi >= 2^-14: {(err / want)[want >= 2.0 ** -14].max():.3e}")
    assert err.max() <= 2.0 ** -12                                               # half an fp16 ulp below 1
    assert (err <= want * 2.0 ** -11 + 2.0 ** -25).all()                         # what gelu_apx('table') allows for the store


def test_layernorm_edge_rows():
    """the LayerNorm edge inputs of the GPU test through the float32 LayerNorm: common offset of 30 sigma, variance exactly 0, one 1e4 outlier"""
    g, be = np.linspace(0.5, 1.5, sr.DIM).astype(np.float32), np.linspace(-0.2, 0.2, sr.DIM).astype(np.float32)
    for kind, x in sr.ln_edge_inputs(sr.DIM).items():
        for bf16 in (True, False):
            ln, ln32 = sr.layernorm_ref(x, g, be, sr.EPS, bf16)
            y32, mu32, rs32 = sr.layernorm_f32(x, g, be, sr.EPS)
            assert sr.worst_ratio(sr.bf16_rne(y32) if bf16 else y32, *ln["y"]) <= 1.0, kind
            assert sr.worst_ratio(mu32, *ln["mean"]) <= 1.0 and sr.worst_ratio(rs32, *ln["rstd"]) <= 1.0, kind
        print(f"[stage] ln32 of '{kind}': " + " ".join(f"{k}={v:.3e}" for k, v in ln32.items()))
