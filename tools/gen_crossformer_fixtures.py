"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_cf_*.npz by EXECUTING THE REFERENCE'S OWN crossformer.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  Conv2D (strided 'SAME') is the stand-in of
tools/gen_twins_fixtures.py; nn.ReLU is max(x, 0); two more names are installed on the shim module here, at run time, under the earlier
generators' rule:

  * tf.stack(values, axis=0) IS torch.stack of the values as shim tensors;
  * tf.meshgrid(*args, indexing='xy') IS torch.meshgrid with that indexing, as a list.

tests/test_crossformer_oracle.py checks both against numpy.

crossformer.py's own default runs the model with training=True; with ff_dropout 0.0 every Dropout is the identity, so that is the
deterministic path and the fixtures are generated that way.

Seeded weights (tests/crossformer_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img, dlogits,
logits, dimg, every gradient and the name / shape table, in files of at most PART_BYTES of arrays, cut and put together as NesT's are.  The
position-bias network gets no gradient from the reference (crossformer.py:163 goes through .numpy()): autograd returns None for its
variables and the fixture holds zeros.  When a fixture is written, zeroing every bias (the last Dense of every dpb network) must move the
float64 logits by at least 1e-2 of their spread -- otherwise the fixture would not pin the bias at all.

    python tools/gen_crossformer_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import gen_nest_fixtures as nest_gen  # noqa: E402
import gen_twins_fixtures as twins_gen  # noqa: E402
import crossformer_ref  # noqa: E402

GOLDEN = nest_gen.GOLDEN
PART_BYTES = nest_gen.PART_BYTES
Conv2D = twins_gen.Conv2D

# case -> ((H, W), constructor kwargs)
CASES = {
    # uneven 'SAME' padding (kernels 3, 4, 8 at stride 4; 2 and 4 at stride 1); three scales; width 48: inner = 32 != dim; two heads at stage 2;
    # windows of 9, 4 and 1 tokens; a dilated 3 x 3 window on the 3 x 6 map of stage 3; depth 2 at stage 2.  Maps 6x12, 6x12, 3x6, 3x6.
    "cf_rect": ((24, 48), dict(dim=(48, 64, 32, 32), depth=(1, 2, 1, 1), global_window_size=(2, 1, 3, 1), local_window_size=(3, 2, 1, 3),
                               cross_embed_kernel_sizes=((3, 4, 8), (2, 4), (3,), (2, 4)), cross_embed_strides=(4, 1, 2, 1), num_classes=4)),
    # the reference usage's token counts: 49-token local windows, 64 / 16 / 4 / 1-token dilated windows, on maps 56, 28, 14, 7
    "cf_usage_windows": ((56, 56), dict(dim=32, depth=1, global_window_size=(8, 4, 2, 1), local_window_size=7,
                                        cross_embed_kernel_sizes=((1, 2), (2, 4), (2, 4), (2, 4)), cross_embed_strides=(1, 2, 2, 2), num_classes=5)),
    # widths the bf16 mode takes; two and four heads; windows of 1, 4 and 16 tokens.  Maps 8x8, 8x8, 4x4, 2x2.
    "cf_bf16": ((16, 16), dict(dim=(64, 64, 128, 64), depth=1, global_window_size=(4, 2, 1, 1), local_window_size=(2, 4, 2, 1),
                               cross_embed_kernel_sizes=((2, 4), (2, 4), (2, 4), (1,)), cross_embed_strides=(2, 1, 2, 2), num_classes=5)),
    # the 49- and 64-token windows at a width the bf16 mode takes (two heads), one stage deep: maps 56x56, then 28, 14, 7 without layers
    "cf_bf16_w64": ((56, 56), dict(dim=(64, 64, 64, 64), depth=(1, 0, 0, 0), global_window_size=(8, 1, 1, 1), local_window_size=(7, 1, 1, 1),
                                   cross_embed_kernel_sizes=((1, 2), (2,), (2,), (2,)), cross_embed_strides=(1, 2, 2, 2), num_classes=5)),
}


# ------------------------------------------------------------------------------------------------ shim extras
def stack(values, axis=0, name=None):
    return tf_shim._t(torch.stack([tf_shim._t(v) for v in values], dim=axis))


def meshgrid(*args, indexing="xy", name=None):
    return [tf_shim._t(g) for g in torch.meshgrid(*[tf_shim._t(a) for a in args], indexing=indexing)]


class ReLU(tf_shim.Layer):
    def call(self, inputs):
        return torch.relu(tf_shim._t(inputs))


@contextlib.contextmanager
def crossformer_layers_installed():
    """nn.Conv2D is the Twins generator's while a CrossFormer is constructed; tf.stack / tf.meshgrid (and nn.ReLU where the shim has none) are
    this file's."""
    with twins_gen.twins_layers_installed():
        import tensorflow as tf
        import tensorflow.keras.layers as nn
        tf.stack, tf.meshgrid = stack, meshgrid
        had_relu = hasattr(nn, "ReLU")
        if not had_relu:
            nn.ReLU = ReLU
        try:
            yield
        finally:
            if not had_relu:
                del nn.ReLU


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}

    def attn(q, a):
        out[q + ".norm.g"], out[q + ".norm.b"] = a.norm.g, a.norm.b
        out[q + ".to_qkv.kernel"] = a.to_qkv.kernel
        out[q + ".to_out.kernel"], out[q + ".to_out.bias"] = a.to_out.kernel, a.to_out.bias
        layers = a.dpb.dpb_layers.layers
        for i in range(3):
            dense, norm = layers[3 * i], layers[3 * i + 1]
            out[f"{q}.dpb.dense.{i}.kernel"], out[f"{q}.dpb.dense.{i}.bias"] = dense.kernel, dense.bias
            out[f"{q}.dpb.norm.{i}.gamma"], out[f"{q}.dpb.norm.{i}.beta"] = norm.gamma, norm.beta
        out[q + ".dpb.dense.3.kernel"], out[q + ".dpb.dense.3.bias"] = layers[9].kernel, layers[9].bias

    def ff(q, f):
        norm, fc1, fc2 = f.net.layers[0], f.net.layers[1], f.net.layers[4]
        out[q + ".norm.g"], out[q + ".norm.b"] = norm.g, norm.b
        out[q + ".fc1.kernel"], out[q + ".fc1.bias"] = fc1.kernel, fc1.bias
        out[q + ".fc2.kernel"], out[q + ".fc2.bias"] = fc2.kernel, fc2.bias

    for s, (cel, tr) in enumerate(model.crossformer_layers):
        pre = f"crossformer_layers.{s}"
        for i, conv in enumerate(cel.convs):
            out[f"{pre}.cel.convs.{i}.kernel"], out[f"{pre}.cel.convs.{i}.bias"] = conv.kernel, conv.bias
        for l, (sa, sf, la, lf) in enumerate(tr.layers):
            q = f"{pre}.transformer.{l}"
            attn(q + ".short_attn", sa); ff(q + ".short_ff", sf)
            attn(q + ".long_attn", la); ff(q + ".long_ff", lf)
    head = model.to_logits.layers[1]
    out["to_logits.kernel"], out["to_logits.bias"] = head.kernel, head.bias
    return out


def make(case: str, b: int = 2) -> dict:
    from oracle.gen_ref_fixtures import _import_reference
    (H, W), kw = CASES[case]
    nest_gen.install_shim_extras()
    tf_shim.seed(1234)
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.standard_normal((b, H, W, 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    with crossformer_layers_installed():        # (the reference looks tf.stack / tf.meshgrid up at call time)
        mod = _import_reference("crossformer")
        model = mod.CrossFormer(**kw)
        model(x)                                                   # Keras builds the layers on the first call
        ref_vars = reference_variables(model)
        table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
        P = crossformer_ref.init_params(table, seed=1)
        for n, v in ref_vars.items():
            tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
        logits = model(x)
        loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
        grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()), allow_unused=True)
        # the bias must matter: zero the last Dense of every dpb network and look at the logits again
        saved = {n: v.detach().clone() for n, v in ref_vars.items() if ".dpb.dense.3." in n}
        for n in saved:
            tf_shim.assign(ref_vars[n], torch.zeros_like(saved[n]))
        unbiased = model(x).detach().numpy()
        for n, v in saved.items():
            tf_shim.assign(ref_vars[n], v)
    lg = logits.detach().numpy().astype(np.float64)
    moved, spread = np.abs(unbiased - lg).max(), lg.max() - lg.min()
    assert moved >= 1e-2 * spread, f"{case}: zeroing the position biases moves the logits by {moved:.3e} of a spread of {spread:.3e}"
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": lg,
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1), "bias_effect": np.float64(moved / spread),
           "names": np.array(list(ref_vars)), "shapes": np.array([",".join(str(s) for s in t[1]) for t in table])}
    for (n, v), g in zip(ref_vars.items(), grads[1:]):
        assert (g is None) == crossformer_ref.is_dpb(n), n           # exactly the dpb variables are off the tape
        out["grad/" + n] = (np.zeros(tuple(v.shape)) if g is None else g.numpy().astype(np.float64)).reshape(tuple(v.shape))
    return out


def load(case: str) -> dict:
    """A fixture put together; the gradients (stored as matrices so that a [1, 1, in, out] kernel can be cut by rows) in their table shapes."""
    z = nest_gen.load(case)
    for n, sh in zip(z["names"], z["shapes"]):
        z["grad/" + str(n)] = z["grad/" + str(n)].reshape(tuple(int(s) for s in str(sh).split(",")))
    return z


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return crossformer_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case][1])


def image_of(case: str):
    return CASES[case][0]


def main(argv):
    for case in (argv or list(CASES)):
        out = make(case)
        for old in glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz")):
            os.remove(old)
        items = []
        for k, v in out.items():
            items += twins_gen._cut(k, v.reshape(-1, v.shape[-1]) if k.startswith("grad/") else v)
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
