"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_crossvit_*.npz by EXECUTING THE REFERENCE'S OWN cross_vit.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  Seeded weights (tests/crossvit_ref.py:init_params)
are loaded into the reference's layers by table name; the fixture holds the inputs, the logits, d(sum(logits * dlogits)) for every
variable, d(img), and the table (names in order, shapes) that the name -> attribute map below produced.

    python tools/gen_crossvit_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import tf_shim  # noqa: E402
from oracle.gen_ref_fixtures import _import_reference  # noqa: E402
import crossvit_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = {
    # sm_dim != lg_dim: project_in / project_out present
    "crossvit_small": dict(image_size=32, num_classes=7, sm_dim=32, lg_dim=48, sm_patch_size=8, sm_enc_depth=1, sm_enc_heads=2, sm_enc_mlp_dim=64,
                           sm_enc_dim_head=16, lg_patch_size=16, lg_enc_depth=2, lg_enc_heads=2, lg_enc_mlp_dim=96, lg_enc_dim_head=16,
                           cross_attn_depth=1, cross_attn_heads=2, cross_attn_dim_head=16, depth=1, dropout=0.0, emb_dropout=0.0),
    # sm_dim == lg_dim: no projections
    "crossvit_same_dim": dict(image_size=32, num_classes=5, sm_dim=32, lg_dim=32, sm_patch_size=4, sm_enc_depth=1, sm_enc_heads=2, sm_enc_mlp_dim=64,
                              sm_enc_dim_head=16, lg_patch_size=8, lg_enc_depth=1, lg_enc_heads=4, lg_enc_mlp_dim=48, lg_enc_dim_head=8,
                              cross_attn_depth=1, cross_attn_heads=2, cross_attn_dim_head=32, depth=1, dropout=0.0, emb_dropout=0.0),
    # depth 2 x cross_attn_depth 2
    "crossvit_deep": dict(image_size=16, num_classes=6, sm_dim=24, lg_dim=40, sm_patch_size=4, sm_enc_depth=1, sm_enc_heads=2, sm_enc_mlp_dim=48,
                          sm_enc_dim_head=12, lg_patch_size=8, lg_enc_depth=1, lg_enc_heads=2, lg_enc_mlp_dim=80, lg_enc_dim_head=20,
                          cross_attn_depth=2, cross_attn_heads=2, cross_attn_dim_head=16, depth=2, dropout=0.0, emb_dropout=0.0),
}


def _dense(out, name, layer, bias=True):
    out[name + ".kernel"] = layer.kernel
    if bias:
        out[name + ".bias"] = layer.bias


def _ln(out, name, layer):
    out[name + ".gamma"] = layer.gamma
    out[name + ".beta"] = layer.beta


def _attn(out, pre, attn):
    _dense(out, pre + ".to_q", attn.to_q, bias=False)      # cross_vit.py:61
    _dense(out, pre + ".to_kv", attn.to_kv, bias=False)    # cross_vit.py:62
    _dense(out, pre + ".to_out", attn.to_out.layers[0])    # cross_vit.py:64-69


def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    for br in ("sm", "lg"):
        e = getattr(model, br + "_image_embedder")
        out[br + "_image_embedder.pos_embedding"] = e.pos_embedding
        out[br + "_image_embedder.cls_token"] = e.cls_token
        _dense(out, br + "_image_embedder.patch_embedding", e.patch_embedding.layers[1])
    for i, (sm_enc, lg_enc, cross) in enumerate(model.multi_scale_encoder.layers):
        L = f"multi_scale_encoder.{i}"
        for br, enc in (("sm", sm_enc), ("lg", lg_enc)):
            for j, (attn, mlp) in enumerate(enc.layers):
                p = f"{L}.{br}_enc.{j}"
                _ln(out, p + ".attn.norm", attn.norm)
                _attn(out, p + ".attn", attn.fn)
                _ln(out, p + ".mlp.norm", mlp.norm)
                _dense(out, p + ".mlp.fc1", mlp.fn.net.layers[0])
                _dense(out, p + ".mlp.fc2", mlp.fn.net.layers[3])
            _ln(out, f"{L}.{br}_enc.norm", enc.norm)
        for k, pair in enumerate(cross.layers):
            for nm, pio in zip(("sm_attend_lg", "lg_attend_sm"), pair):
                p = f"{L}.cross.{k}.{nm}"
                if pio.need_projection:
                    _dense(out, p + ".project_in", pio.project_in)
                _ln(out, p + ".norm", pio.fn.norm)
                _attn(out, p, pio.fn.fn)
                if pio.need_projection:
                    _dense(out, p + ".project_out", pio.project_out)
    for br in ("sm", "lg"):
        h = getattr(model, br + "_mlp_head").layers
        _ln(out, br + "_mlp_head.norm", h[0])
        _dense(out, br + "_mlp_head", h[1])
    return out


def make(case: str, b: int = 2) -> dict:
    kw = CASES[case]
    mod = _import_reference("cross_vit")
    tf_shim.seed(1234)
    model = mod.CrossViT(**kw)
    rng = np.random.Generator(np.random.PCG64(7))
    H = kw["image_size"]
    img = rng.standard_normal((b, H, H, 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    model(x, training=False)                                   # Keras builds the layers on the first call
    ref_vars = reference_variables(model)
    table = [(n, tuple(v.shape), 0) for n, v in ref_vars.items()]
    P = crossvit_ref.init_params(table, seed=1)
    for n, v in ref_vars.items():
        tf_shim.assign(v, P[n])
    logits = model(x, training=True)                           # the reference's default; dropout rates are 0
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
    grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()))
    out = {"img": img, "dlogits": dlogits, "logits": logits.numpy().astype(np.float64), "dimg": grads[0].numpy().astype(np.float64),
           "param_seed": np.int64(1), "names": np.array(list(ref_vars)),
           "shapes": np.array([",".join(str(s) for s in v.shape) for v in ref_vars.values()])}
    for n, t in zip(ref_vars, grads[1:]):
        out["grad/" + n] = t.numpy().astype(np.float64)
    return out


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return crossvit_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case])


def main(argv):
    for case in (argv or list(CASES)):
        out = make(case)
        path = os.path.join(GOLDEN, f"ref_{case}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:])
