"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_sd_*.npz by EXECUTING THE REFERENCE'S OWN vit_for_small_dataset.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  The shim lacks five things that file needs; they are
installed on the shim module here, at run time (install_shim_extras).  Seeded weights (tests/small_dataset_ref.py:init_params) are loaded into
the reference's layers by table name; the fixture holds the inputs, the logits, d(sum(logits * dlogits)) for every variable, d(img), and the
table (names in order, shapes) that the name -> attribute map below produced.

    python tools/gen_small_dataset_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import small_dataset_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = {
    "sd_small": dict(image_size=16, patch_size=4, num_classes=5, dim=32, depth=2, heads=2, dim_head=16, mlp_dim=48, pool="cls"),        # 17 tokens
    "sd_rect_mean": dict(image_size=(8, 24), patch_size=8, num_classes=4, dim=24, depth=1, heads=3, dim_head=32, mlp_dim=40, pool="mean"),   # 4 tokens
    # 2 tokens: each attends only to the other; every patch pixel is an image-border pixel
    "sd_2tok": dict(image_size=4, patch_size=4, num_classes=3, dim=16, depth=1, heads=1, dim_head=16, mlp_dim=16, pool="cls"),
    "sd_dh64": dict(image_size=32, patch_size=4, num_classes=6, dim=48, depth=1, heads=2, dim_head=64, mlp_dim=64, pool="cls"),          # 65 tokens
    # widths the engine's bf16 mode accepts (dim, heads * dim_head and mlp_dim multiples of 64): the bf16 check against reference-produced data
    "sd_bf16": dict(image_size=16, patch_size=4, num_classes=5, dim=64, depth=2, heads=2, dim_head=32, mlp_dim=64, pool="cls"),
}


class _DtypeProxy:
    """A torch dtype that also answers `.as_numpy_dtype` (vit_for_small_dataset.py:112 reads it off dots.dtype)."""
    as_numpy_dtype = np.float32

    def __init__(self, d):
        self._d = d

    def __getattr__(self, n):
        return getattr(self._d, n)

    def __eq__(self, o):
        return self._d == (o._d if isinstance(o, _DtypeProxy) else o)

    def __hash__(self):
        return hash(self._d)


class _TD(tf_shim._T):
    @property
    def dtype(self):
        return _DtypeProxy(torch.Tensor.dtype.__get__(self))


def install_shim_extras():
    """tf.roll, tf.eye, tf.math.log, tf.math.exp (its result carries the dtype proxy, so that `dots` does between the multiply and the where)
    and a tf.where that hands back a plain shim tensor."""
    tf_shim.install()
    import tensorflow as tf
    if getattr(tf, "_vitx_sd_extras", False):
        return
    t = tf_shim._t
    tf.roll = lambda x, shift, axis: torch.roll(t(x), int(shift), dims=int(axis))

    def eye(n, dtype=None):
        e = torch.eye(int(n))
        return t(e.bool() if dtype in (bool, torch.bool, getattr(tf, "bool", None)) else e.double())
    tf.eye = eye
    tf.math.log = lambda x: torch.log(t(x))
    tf.math.exp = lambda x: torch.exp(t(x)).as_subclass(_TD)
    where = tf.where
    tf.where = lambda c, x=None, y=None, name=None: where(c, x, y).as_subclass(tf_shim._T)
    tf._vitx_sd_extras = True


def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {"pos_embedding": model.pos_embedding, "cls_token": model.cls_token}
    seq = model.patch_embedding.to_patch_tokens.layers
    out["patch_embedding.norm.gamma"] = seq[1].gamma
    out["patch_embedding.norm.beta"] = seq[1].beta
    out["patch_embedding.kernel"] = seq[2].kernel
    out["patch_embedding.bias"] = seq[2].bias
    for l, (attn, ff) in enumerate(model.transformer.layers):
        p = f"transformer.{l}"
        out[p + ".attn.norm.gamma"] = attn.norm.gamma
        out[p + ".attn.norm.beta"] = attn.norm.beta
        out[p + ".attn.temperature"] = attn.fn.temperature
        out[p + ".attn.to_qkv.kernel"] = attn.fn.to_qkv.kernel
        out[p + ".attn.to_out.kernel"] = attn.fn.to_out.layers[0].kernel
        out[p + ".attn.to_out.bias"] = attn.fn.to_out.layers[0].bias
        out[p + ".mlp.norm.gamma"] = ff.norm.gamma
        out[p + ".mlp.norm.beta"] = ff.norm.beta
        out[p + ".mlp.fc1.kernel"] = ff.fn.net.layers[0].kernel
        out[p + ".mlp.fc1.bias"] = ff.fn.net.layers[0].bias
        out[p + ".mlp.fc2.kernel"] = ff.fn.net.layers[3].kernel
        out[p + ".mlp.fc2.bias"] = ff.fn.net.layers[3].bias
    h = model.mlp_head.layers
    out["mlp_head.norm.gamma"] = h[0].gamma
    out["mlp_head.norm.beta"] = h[0].beta
    out["mlp_head.kernel"] = h[1].kernel
    out["mlp_head.bias"] = h[1].bias
    return out


def _shape(v):
    s = tuple(int(d) for d in v.shape)
    return s if s else (1,)       # the reference's temperature is a rank-0 variable; the library's table holds it as [1]


def make(case: str, b: int = 2) -> dict:
    kw = CASES[case]
    install_shim_extras()
    mod = _import_reference("vit_for_small_dataset")
    tf_shim.seed(1234)
    model = mod.ViT(**kw)
    rng = np.random.Generator(np.random.PCG64(7))
    H, W = kw["image_size"] if isinstance(kw["image_size"], tuple) else (kw["image_size"], kw["image_size"])
    img = rng.standard_normal((b, H, W, 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    model(x, training=False)                                   # Keras builds the layers on the first call
    ref_vars = reference_variables(model)
    table = [(n, _shape(v), 0) for n, v in ref_vars.items()]
    P = small_dataset_ref.init_params(table, seed=1, dim_head=kw["dim_head"])
    for n, v in ref_vars.items():
        tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
    logits = model(x, training=True)                           # the reference's default; dropout rates are 0
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
    grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()))
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": logits.numpy().astype(np.float64),
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1), "names": np.array(list(ref_vars)),
           "shapes": np.array([",".join(str(s) for s in _shape(v)) for v in ref_vars.values()])}
    for (n, v), g in zip(ref_vars.items(), grads[1:]):
        out["grad/" + n] = g.numpy().astype(np.float64).reshape(_shape(v))
    return out


def params_of(z, case: str) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return small_dataset_ref.init_params(table, seed=int(z["param_seed"]), dim_head=CASES[case]["dim_head"])


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
