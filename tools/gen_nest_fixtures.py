"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_nest_*.npz by EXECUTING THE REFERENCE'S OWN nest.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  The names that file needs beyond what the shim and
tools/gen_cct_fixtures.py provide are installed on the shim module here, at run time (install_shim_extras), under the CCT generator's two rules:

  * Conv2D IS the shim's own tf.image.extract_patches(..., 'SAME') (pinned to TensorFlow through the T2T fixtures) followed by a matmul with the
    kernel reshaped to [k*k*Cin, Cout], plus the bias (a 1x1 'valid' convolution is the same thing: no padding either way);
  * MaxPool2D IS the same extract_patches followed by a max over the window axis.  NesT pools a LayerNorm output, which is signed, so the input
    is shifted to be non-negative first (x - min(x)) and shifted back after: the zero fill of extract_patches then equals TensorFlow's "padding
    never wins", and a shift commutes with max.

tests/test_nest_oracle.py checks both against torch's conv2d / max_pool2d on explicitly padded tensors.

nest.py's own defaults run the model with training=True; with dropout 0.0 every Dropout is the identity, so that is the deterministic path and
the fixtures are generated that way.

Seeded weights (tests/nest_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img, dlogits, logits,
dimg, every gradient and the name / shape table, in files of at most PART_BYTES of arrays (ref_<case>.npz, ref_<case>.part1.npz, ...; an array
larger than that is cut along its first axis); load() puts them together.

    python tools/gen_nest_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
"""
from __future__ import annotations

import contextlib
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import tf_shim  # noqa: E402
import gen_cct_fixtures as cct_gen  # noqa: E402
import nest_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 480 * 1024

CASES = {
    # 8 x 8 map, blocks 4 / 2 / 1 of 2 x 2 = 4 tokens; heads 1 with dim_head == dim at level 0 (to_out kept), dim_head 8: generic attention
    "nest_small": dict(image_size=16, patch_size=2, num_classes=5, dim=8, heads=1, num_hierarchies=3, block_repeats=(1, 1, 2), mlp_mult=2),
    # 6 x 6 map, 2 x 2 blocks of 3 x 3 = 9 tokens (under one row tile), dim_head 32
    "nest_dh32_9tok": dict(image_size=12, patch_size=2, num_classes=4, dim=32, heads=1, num_hierarchies=2, block_repeats=2, mlp_mult=2),
    # one level: no aggregation, no blocking; its single pos_emb is the last level's
    "nest_1level": dict(image_size=8, patch_size=4, num_classes=3, dim=16, heads=2, num_hierarchies=1, block_repeats=1, mlp_mult=1),
    # 28 x 28 map, 2 x 2 blocks of 14 x 14 = 196 tokens (the usage's count: four row tiles, no multiple of 16), dim_head 16
    "nest_196tok": dict(image_size=28, patch_size=1, num_classes=4, dim=32, heads=2, num_hierarchies=2, block_repeats=1, mlp_mult=1),
    # dim // heads truncates: inner 9 != dim 10 (and 18 != 20), widths that are no multiples of 4
    "nest_inner9": dict(image_size=8, patch_size=2, num_classes=3, dim=10, heads=3, num_hierarchies=2, block_repeats=1, mlp_mult=2),
    # widths the bf16 mode accepts; dim_head 64 with heads 1: to_out kept on the existing fused kernels
    "nest_bf16": dict(image_size=12, patch_size=2, num_classes=5, dim=64, heads=1, num_hierarchies=2, block_repeats=1, mlp_mult=1),
}


# ------------------------------------------------------------------------------------------------ shim extras
class Conv2D(tf_shim.Layer):
    """nn.Conv2D(filters, kernel_size, strides, padding, use_bias) as extract_patches + matmul + bias."""

    def __init__(self, filters, kernel_size, strides=1, padding="valid", use_bias=True, **kw):
        super().__init__(**kw)
        self.filters, self.k, self.s, self.use_bias = int(filters), int(kernel_size), int(strides), bool(use_bias)
        assert str(padding).upper() == "SAME" or self.k == 1, "'valid' only where it equals 'SAME' (1x1)"
        self.kernel = self.bias = None

    def build(self, input_shape):
        cin = int(input_shape[-1])
        lim = np.sqrt(6.0 / (self.k * self.k * (cin + self.filters)))   # glorot_uniform
        self.kernel = tf_shim.Variable(tf_shim._random_uniform([self.k, self.k, cin, self.filters], -lim, lim))
        self._weights = [self.kernel]
        if self.use_bias:
            self.bias = tf_shim.Variable(torch.zeros(self.filters, dtype=tf_shim.DTYPE))
            self._weights.append(self.bias)

    def call(self, inputs):
        rows = tf_shim.extract_patches(inputs, [1, self.k, self.k, 1], [1, self.s, self.s, 1], [1, 1, 1, 1], "SAME")
        y = torch.matmul(rows, self.kernel.reshape(-1, self.filters))
        return y + self.bias if self.use_bias else y


class MaxPool2D(tf_shim.Layer):
    """nn.MaxPool2D(pool_size, strides, padding='SAME') on a signed input: the CCT generator's extract_patches + max on x - min(x), shifted back."""

    def __init__(self, pool_size=2, strides=None, padding="valid", **kw):
        super().__init__(**kw)
        assert str(padding).upper() == "SAME"
        self.pool = cct_gen.MaxPool2D(pool_size=pool_size, strides=strides, padding=padding)

    def call(self, inputs):
        x = tf_shim._t(inputs)
        lo = x.detach().min()
        return self.pool(x - lo) + lo


@contextlib.contextmanager
def nest_layers_installed():
    """nn.Conv2D / nn.MaxPool2D are this file's while a NesT is constructed, and the CCT generator's again afterwards."""
    install_shim_extras()
    import tensorflow.keras.layers as nn
    saved = nn.Conv2D, nn.MaxPool2D
    nn.Conv2D, nn.MaxPool2D = Conv2D, MaxPool2D
    try:
        yield
    finally:
        nn.Conv2D, nn.MaxPool2D = saved


def install_shim_extras():
    cct_gen.install_shim_extras()
    import tensorflow as tf
    if getattr(tf, "_vitx_nest_extras", False):
        return
    t = tf_shim._t
    tf.ones = lambda shape, dtype=None, name=None: t(torch.ones([int(s) for s in shape], dtype=tf_shim.DTYPE))
    tf.zeros = tf_shim.zeros

    def reduce_variance(x, axis=None, keepdims=False, name=None):   # the biased variance
        x = t(x)
        mean = x.mean(dim=axis, keepdim=True)
        return ((x - mean) ** 2).mean(dim=axis, keepdim=keepdims)
    tf.math.reduce_variance = reduce_variance
    tf._vitx_nest_extras = True


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    pe = model.patch_embedding.layers[1]
    out["patch_embedding.kernel"], out["patch_embedding.bias"] = pe.kernel, pe.bias
    for i, (tr, agg) in enumerate(model.nest_layers):
        pre = f"nest_layers.{i}"
        out[pre + ".transformer.pos_emb"] = tr.pos_emb
        for l, (attn, ff) in enumerate(tr.layers):
            q = f"{pre}.transformer.{l}"
            out[q + ".attn.norm.g"], out[q + ".attn.norm.b"] = attn.norm.g, attn.norm.b
            out[q + ".attn.to_qkv.kernel"] = attn.fn.to_qkv.kernel
            out[q + ".attn.to_out.kernel"], out[q + ".attn.to_out.bias"] = attn.fn.to_out.layers[0].kernel, attn.fn.to_out.layers[0].bias
            out[q + ".ff.norm.g"], out[q + ".ff.norm.b"] = ff.norm.g, ff.norm.b
            fc1, fc2 = ff.fn.net.layers[0], ff.fn.net.layers[3]
            out[q + ".ff.fc1.kernel"], out[q + ".ff.fc1.bias"] = fc1.kernel, fc1.bias
            out[q + ".ff.fc2.kernel"], out[q + ".ff.fc2.bias"] = fc2.kernel, fc2.bias
        if hasattr(agg, "ag_layers"):
            conv, norm = agg.ag_layers.layers[0], agg.ag_layers.layers[1]
            out[pre + ".aggregate.conv.kernel"], out[pre + ".aggregate.conv.bias"] = conv.kernel, conv.bias
            out[pre + ".aggregate.norm.g"], out[pre + ".aggregate.norm.b"] = norm.g, norm.b
    head = model.mlp_head.layers
    out["mlp_head.norm.g"], out["mlp_head.norm.b"] = head[0].g, head[0].b
    out["mlp_head.kernel"], out["mlp_head.bias"] = head[2].kernel, head[2].bias
    return out


def make(case: str, b: int = 2) -> dict:
    from oracle.gen_ref_fixtures import _import_reference
    kw = CASES[case]
    install_shim_extras()
    mod = _import_reference("nest")
    tf_shim.seed(1234)
    with nest_layers_installed():
        model = mod.NesT(**kw)
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.standard_normal((b, kw["image_size"], kw["image_size"], 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    model(x)                                                   # Keras builds the layers on the first call
    ref_vars = reference_variables(model)
    table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
    P = nest_ref.init_params(table, seed=1)
    for n, v in ref_vars.items():
        tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
    logits = model(x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
    grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()))
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": logits.numpy().astype(np.float64),
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1),
           "names": np.array(list(ref_vars)), "shapes": np.array([",".join(str(s) for s in t[1]) for t in table])}
    for (n, v), g in zip(ref_vars.items(), grads[1:]):
        out["grad/" + n] = g.numpy().astype(np.float64).reshape(tuple(v.shape))
    return out


def load(case: str) -> dict:
    """A fixture with its parts (and the pieces of its cut arrays) put together."""
    raw = {}
    for path in [os.path.join(GOLDEN, f"ref_{case}.npz")] + sorted(glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz"))):
        with np.load(path) as z:
            raw.update({k: z[k] for k in z.files})
    out, pieces = {}, {}
    for k, v in raw.items():
        if "@" in k:
            name, i = k.rsplit("@", 1)
            pieces.setdefault(name, {})[int(i)] = v
        else:
            out[k] = v
    for name, d in pieces.items():
        out[name] = np.concatenate([d[i] for i in sorted(d)], axis=0)
    return out


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return nest_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case])


def main(argv):
    for case in (argv or list(CASES)):
        out = make(case)
        for old in glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz")):
            os.remove(old)
        items = []
        for k, v in out.items():
            if v.nbytes > PART_BYTES:     # cut along the first axis
                n = -(-v.nbytes // PART_BYTES)
                assert v.shape[0] >= n, k
                items += [(f"{k}@{i}", piece) for i, piece in enumerate(np.array_split(v, n, axis=0))]
            else:
                items.append((k, v))
        parts, size = [{}], 0
        for k, v in items:
            if size and size + v.nbytes > PART_BYTES:
                parts.append({})
                size = 0
            parts[-1][k] = v
            size += v.nbytes
        for i, part in enumerate(parts):
            path = os.path.join(GOLDEN, f"ref_{case}.npz" if i == 0 else f"ref_{case}.part{i}.npz")
            np.savez_compressed(path, **part)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:])
