"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_cct_*.npz by EXECUTING THE REFERENCE'S OWN cct.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  The shim lacks the names that file needs beyond the
other models'; they are installed on the shim module here, at run time (install_shim_extras).  Two rules keep those extras from sharing a
mistake with the library or with tests/cct_ref.py:

  * Conv2D IS the shim's own tf.image.extract_patches(..., 'SAME') (pinned to TensorFlow through the T2T fixtures) followed by a matmul with the
    kernel reshaped to [k*k*Cin, Cout];
  * MaxPool2D IS the same extract_patches followed by a max over the window axis, and asserts that its input is non-negative, so that the zero
    fill of extract_patches equals TensorFlow's "padding never wins".

tests/test_cct_oracle.py checks both against torch's conv2d / max_pool2d on explicitly padded tensors.

Keras hands `training` down: a layer called without it receives the enclosing call's value.  The shim does not, and cct.py:161 calls
self_attn and drop_path without it -- under the plain shim an "inference" run would apply attention dropout at rate 0.1.  training_inherited()
adds the Keras behaviour for the duration of a run.  The fixtures are generated with training=False.

Seeded weights (tests/cct_ref.py:init_params) are loaded into the reference's layers by table name; a fixture holds img, dlogits, logits, dimg,
every gradient and the name / shape table.  A fixture whose arrays exceed the size the other fixtures have is written as several files
(ref_<case>.npz, ref_<case>.part1.npz, ...); load() puts them together.

positional_embedding='sine' has no fixture: the reference raises there under TensorFlow (cct.py:271-272 assigns into a tensor), so a run under
the shim -- whose tensors do allow the assignment -- would record the shim's behaviour, not the reference's.  The tests check that mode against
tests/cct_ref.py:sine_table.

    python tools/gen_cct_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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

from oracle import tf_shim  # noqa: E402
import cct_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 480 * 1024   # the largest of the other models' fixtures is 547 kB

CASES = {
    # 16 x 16 -> conv k3 s1 16 x 16 -> pool 3/2 8 x 8 = 64 tokens
    "cct_small": dict(img_size=16, embedding_dim=32, n_conv_layers=1, kernel_size=3, stride=1, pooling_kernel_size=3, pooling_stride=2,
                      num_layers=2, num_heads=2, mlp_ratio=2, num_classes=5, positional_embedding="learnable"),
    # 12 x 20 -> 6 x 10 -> 3 x 5 -> 2 x 3 -> 1 x 2 = 2 tokens: rectangular, both pad parities, 64 intermediate planes (K = 147 and 3136)
    "cct_rect_2conv": dict(img_size=(12, 20), embedding_dim=24, n_conv_layers=2, kernel_size=7, stride=2, pooling_kernel_size=3, pooling_stride=2,
                           num_layers=1, num_heads=3, mlp_ratio=2, num_classes=4, positional_embedding="none"),
    # 4 x 4 -> 2 x 2 -> 1 token: softmax over one token, attention over one key
    "cct_1tok": dict(img_size=4, embedding_dim=16, n_conv_layers=1, kernel_size=3, stride=2, pooling_kernel_size=3, pooling_stride=2,
                     num_layers=1, num_heads=1, mlp_ratio=1, num_classes=3, positional_embedding="none"),
    # widths the engine's bf16 mode accepts (embedding_dim and int(embedding_dim * mlp_ratio) multiples of 64, head_dim 64)
    "cct_bf16": dict(img_size=16, embedding_dim=128, n_conv_layers=1, kernel_size=3, stride=1, pooling_kernel_size=3, pooling_stride=2,
                     num_layers=2, num_heads=2, mlp_ratio=1, num_classes=5, positional_embedding="learnable"),
}


# ------------------------------------------------------------------------------------------------ shim extras
class Conv2D(tf_shim.Layer):
    """nn.Conv2D(filters, kernel_size, strides, padding='SAME', use_bias=False) as extract_patches + matmul."""

    def __init__(self, filters, kernel_size, strides=1, padding="valid", use_bias=True, **kw):
        super().__init__(**kw)
        assert str(padding).upper() == "SAME" and not use_bias
        self.filters, self.k, self.s = int(filters), int(kernel_size), int(strides)
        self.kernel = None

    def build(self, input_shape):
        cin = int(input_shape[-1])
        lim = np.sqrt(6.0 / (self.k * self.k * (cin + self.filters)))   # glorot_uniform
        self.kernel = tf_shim.Variable(tf_shim._random_uniform([self.k, self.k, cin, self.filters], -lim, lim))
        self._weights = [self.kernel]

    def call(self, inputs):
        rows = tf_shim.extract_patches(inputs, [1, self.k, self.k, 1], [1, self.s, self.s, 1], [1, 1, 1, 1], "SAME")
        return torch.matmul(rows, self.kernel.reshape(-1, self.filters))


class MaxPool2D(tf_shim.Layer):
    """nn.MaxPool2D(pool_size, strides, padding='SAME') as extract_patches + max over the window axis (non-negative input only)."""

    def __init__(self, pool_size=2, strides=None, padding="valid", **kw):
        super().__init__(**kw)
        assert str(padding).upper() == "SAME"
        self.k, self.s = int(pool_size), int(strides if strides is not None else pool_size)

    def call(self, inputs):
        x = tf_shim._t(inputs)
        assert bool((x >= 0).all()), "MaxPool2D extra: zero fill stands for TF's -inf padding only on non-negative input"
        b, _, _, c = x.shape
        rows = tf_shim.extract_patches(x, [1, self.k, self.k, 1], [1, self.s, self.s, 1], [1, 1, 1, 1], "SAME")
        return rows.reshape(b, rows.shape[1], rows.shape[2], self.k * self.k, c).max(dim=3).values


class ReLU(tf_shim.Layer):
    def call(self, inputs):
        return torch.relu(tf_shim._t(inputs))


def install_shim_extras():
    tf_shim.install()
    import tensorflow as tf
    import tensorflow.keras.layers as nn
    if getattr(tf, "_vitx_cct_extras", False):
        return
    t = tf_shim._t
    nn.Conv2D, nn.MaxPool2D, nn.ReLU = Conv2D, MaxPool2D, ReLU
    tf.pad = lambda x, paddings, **_: torch.nn.functional.pad(t(x), [int(v) for pr in reversed([list(p) for p in paddings]) for v in pr])
    tf.tile = lambda x, multiples: t(x).repeat(*[int(m) for m in multiples])
    tf.squeeze = lambda x, axis=None: t(x).squeeze() if axis is None else t(x).squeeze(int(axis))
    tf.linspace = lambda start, stop, num: torch.linspace(float(start), float(stop), int(num), dtype=tf_shim.DTYPE).as_subclass(tf_shim._T)
    tf.floor = lambda x: torch.floor(t(x))
    tf.divide = lambda x, y: t(x) / y
    tf.rank = lambda x: torch.tensor(t(x).dim()).as_subclass(tf_shim._T)

    def truncated_normal(shape, mean=0.0, stddev=1.0, dtype=None, seed=None, name=None):
        v = tf_shim._random_normal(shape)
        for _ in range(64):   # redraw what lies beyond two standard deviations
            bad = v.abs() > 2.0
            if not bool(bad.any()):
                break
            v = torch.where(bad, tf_shim._random_normal(shape), v)
        return (v.clamp(-2.0, 2.0) * stddev + mean).as_subclass(tf_shim._T)
    tf.random.truncated_normal = truncated_normal
    tf._vitx_cct_extras = True


@contextlib.contextmanager
def training_inherited():
    """Keras' propagation of `training`: a layer whose call() takes it and that is called without it receives the enclosing call's value."""
    stack = [None]
    layer_call, model_call = tf_shim.Layer.__call__, tf_shim.Model.__call__

    def wrap(orig):
        def call(self, *args, **kwargs):
            if "training" not in kwargs and tf_shim._accepts(self.call, "training"):
                kwargs["training"] = stack[-1]
            stack.append(kwargs.get("training", stack[-1]))
            try:
                return orig(self, *args, **kwargs)
            finally:
                stack.pop()
        return call
    tf_shim.Layer.__call__, tf_shim.Model.__call__ = wrap(layer_call), wrap(model_call)
    try:
        yield
    finally:
        tf_shim.Layer.__call__, tf_shim.Model.__call__ = layer_call, model_call


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    convs = [l for l in model.tokenizer.conv_layers.layers if isinstance(l, Conv2D)]
    for i, l in enumerate(convs):
        out[f"tokenizer.conv_layers.{i}.kernel"] = l.kernel
    c = model.classifier
    out["classifier.attention_pool.kernel"] = c.attention_pool.kernel
    out["classifier.attention_pool.bias"] = c.attention_pool.bias
    if c.positional_emb is not None:
        out["classifier.positional_emb"] = c.positional_emb
    for l, blk in enumerate(c.blocks.layers):
        p = f"classifier.blocks.{l}"
        out[p + ".pre_norm.gamma"] = blk.pre_norm.gamma
        out[p + ".pre_norm.beta"] = blk.pre_norm.beta
        out[p + ".self_attn.to_qkv.kernel"] = blk.self_attn.to_qkv.kernel
        out[p + ".self_attn.proj.kernel"] = blk.self_attn.proj.layers[0].kernel
        out[p + ".self_attn.proj.bias"] = blk.self_attn.proj.layers[0].bias
        out[p + ".linear1.kernel"] = blk.linear1.kernel
        out[p + ".linear1.bias"] = blk.linear1.bias
        out[p + ".norm1.gamma"] = blk.norm1.gamma
        out[p + ".norm1.beta"] = blk.norm1.beta
        out[p + ".linear2.kernel"] = blk.linear2.kernel
        out[p + ".linear2.bias"] = blk.linear2.bias
    out["classifier.norm.gamma"] = c.norm.gamma
    out["classifier.norm.beta"] = c.norm.beta
    out["classifier.fc.kernel"] = c.fc.kernel
    out["classifier.fc.bias"] = c.fc.bias
    return out


def make(case: str, b: int = 2) -> dict:
    from oracle.gen_ref_fixtures import _import_reference
    kw = CASES[case]
    install_shim_extras()
    mod = _import_reference("cct")
    tf_shim.seed(1234)
    with training_inherited():
        model = mod.CCT(**kw)
        seq_len = int(model.classifier.sequence_length)
        rng = np.random.Generator(np.random.PCG64(7))
        H, W = cct_ref.pair(kw["img_size"])
        img = rng.standard_normal((b, H, W, 3)).astype(np.float32)
        dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
        x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
        model(x, training=False)                                   # Keras builds the layers on the first call
        ref_vars = reference_variables(model)
        table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
        P = cct_ref.init_params(table, seed=1)
        for n, v in ref_vars.items():
            tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
        logits = model(x, training=False)
        loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
        grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()))
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": logits.numpy().astype(np.float64),
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1), "sequence_length": np.int64(seq_len),
           "names": np.array(list(ref_vars)), "shapes": np.array([",".join(str(s) for s in t[1]) for t in table])}
    for (n, v), g in zip(ref_vars.items(), grads[1:]):
        out["grad/" + n] = g.numpy().astype(np.float64).reshape(tuple(v.shape))
    return out


def load(case: str) -> dict:
    """A fixture with its parts put together."""
    out = {}
    for path in [os.path.join(GOLDEN, f"ref_{case}.npz")] + sorted(glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def params_of(z, case: str = "") -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return cct_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case])


def main(argv):
    for case in (argv or list(CASES)):
        out = make(case)
        for old in glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz")):
            os.remove(old)
        parts, size = [{}], 0
        for k, v in out.items():
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
