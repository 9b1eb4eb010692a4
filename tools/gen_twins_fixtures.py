"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_twins_*.npz by EXECUTING THE REFERENCE'S OWN twins_svt.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  The names that file needs beyond what the shim and
tools/gen_nest_fixtures.py provide are installed on the shim module here, at run time, under the earlier generators' rule:

  * Conv2D IS the shim's own tf.image.extract_patches (pinned to TensorFlow through the T2T fixtures) followed by a product with the kernel.
    groups == 1: a matmul with the kernel reshaped to [k*k*Cin, Cout].  groups == Cin == filters (the depthwise PEG convolution, kernel
    [k, k, 1, C]): the window axis of the patches times the kernel viewed as [k*k, C], summed over the window.  'valid' is extract_patches
    'VALID' (rows and columns past the last whole window are dropped, as TensorFlow does);
  * GlobalAvgPool2D IS the mean over the two map axes.

tests/test_twins_oracle.py checks both against torch's conv2d / mean on explicitly padded tensors.

twins_svt.py's own defaults run the model with training=True; with dropout 0.0 every Dropout is the identity, so that is the deterministic
path and the fixtures are generated that way.

Seeded weights (tests/twins_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img, dlogits, logits,
dimg, every gradient and the name / shape table, in files of at most PART_BYTES of arrays, cut and put together as NesT's are.

    python tools/gen_twins_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import twins_ref  # noqa: E402

GOLDEN = nest_gen.GOLDEN
PART_BYTES = nest_gen.PART_BYTES


def _stages(dims, patches, locals_, ks, depths):
    kw = {}
    for i, (d, p, lp, k, n) in enumerate(zip(dims, patches, locals_, ks, depths), 1):
        kw.update({f"s{i}_emb_dim": d, f"s{i}_patch_size": p, f"s{i}_local_patch_size": lp, f"s{i}_global_k": k, f"s{i}_depth": n})
    return kw


# case -> ((H, W), constructor kwargs)
CASES = {
    # maps 4x4, 4x4, 2x2, 2x2; 4, 4, 1, 1 global keys; stage 3 has a second transformer behind its PEG
    "twins_tiny": ((8, 8), dict(num_classes=5, **_stages((4, 4, 8, 8), (2, 1, 2, 1), (2, 2, 2, 1), (2, 2, 2, 2), (0, 0, 1, 0)))),
    # rectangular maps 4x8, 4x8, 2x4, 2x4; global_k 1 (as many keys as queries) at stages 2 and 4; one-token windows at stage 3
    "twins_rect": ((8, 16), dict(num_classes=5, **_stages((4, 4, 8, 8), (2, 1, 2, 1), (2, 2, 1, 1), (2, 1, 2, 1), (0, 0, 0, 0)))),
    # maps 16x16, 8x8, 4x4, 2x2 with global_k 2: 64, 16, 4, 1 keys (the usage's four counts), 256 queries at stage 1
    "twins_k64": ((16, 16), dict(num_classes=5, **_stages((4, 4, 4, 4), (1, 2, 2, 2), (2, 2, 2, 1), (2, 2, 2, 2), (0, 0, 0, 0)))),
}


# ------------------------------------------------------------------------------------------------ shim extras
class Conv2D(tf_shim.Layer):
    """nn.Conv2D(filters, kernel_size, strides, padding, use_bias, groups) as extract_patches + a product with the kernel + bias."""

    def __init__(self, filters, kernel_size, strides=1, padding="valid", use_bias=True, groups=1, **kw):
        super().__init__(**kw)
        self.filters, self.k, self.s, self.use_bias, self.groups = int(filters), int(kernel_size), int(strides), bool(use_bias), int(groups)
        self.padding = "SAME" if str(padding).upper() == "SAME" else "VALID"
        self.kernel = self.bias = None

    def build(self, input_shape):
        cin = int(input_shape[-1])
        assert self.groups == 1 or self.groups == cin == self.filters, "groups: 1 or depthwise"
        per = cin // self.groups
        lim = np.sqrt(6.0 / (self.k * self.k * (per + self.filters)))   # glorot_uniform
        self.kernel = tf_shim.Variable(tf_shim._random_uniform([self.k, self.k, per, self.filters], -lim, lim))
        self._weights = [self.kernel]
        if self.use_bias:
            self.bias = tf_shim.Variable(torch.zeros(self.filters, dtype=tf_shim.DTYPE))
            self._weights.append(self.bias)

    def call(self, inputs):
        rows = tf_shim.extract_patches(inputs, [1, self.k, self.k, 1], [1, self.s, self.s, 1], [1, 1, 1, 1], self.padding)
        if self.groups == 1:
            y = torch.matmul(rows, self.kernel.reshape(-1, self.filters))
        else:
            b, oh, ow, _ = rows.shape
            y = (rows.reshape(b, oh, ow, self.k * self.k, self.filters) * self.kernel.reshape(self.k * self.k, self.filters)).sum(dim=3)
        return y + self.bias if self.use_bias else y


class GlobalAvgPool2D(tf_shim.Layer):
    def call(self, inputs):
        return tf_shim._t(inputs).mean(dim=(1, 2))


@contextlib.contextmanager
def twins_layers_installed():
    """nn.Conv2D / nn.GlobalAvgPool2D are this file's while a TwinsSVT is constructed, and what they were again afterwards."""
    nest_gen.install_shim_extras()
    import tensorflow.keras.layers as nn
    saved = nn.Conv2D, getattr(nn, "GlobalAvgPool2D", None)
    nn.Conv2D, nn.GlobalAvgPool2D = Conv2D, GlobalAvgPool2D
    try:
        yield
    finally:
        nn.Conv2D = saved[0]
        if saved[1] is None:
            del nn.GlobalAvgPool2D
        else:
            nn.GlobalAvgPool2D = saved[1]


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    stages = model.svt_layers.layers

    def attn(q, res):
        a = res.fn.fn
        out[q + ".norm.g"], out[q + ".norm.b"] = res.fn.norm.g, res.fn.norm.b
        out[q + ".to_q.kernel"], out[q + ".to_kv.kernel"] = a.to_q.kernel, a.to_kv.kernel
        out[q + ".to_out.kernel"], out[q + ".to_out.bias"] = a.to_out.layers[0].kernel, a.to_out.layers[0].bias

    def ff(q, res):
        fc1, fc2 = res.fn.fn.net.layers[0], res.fn.fn.net.layers[3]
        out[q + ".norm.g"], out[q + ".norm.b"] = res.fn.norm.g, res.fn.norm.b
        out[q + ".fc1.kernel"], out[q + ".fc1.bias"] = fc1.kernel, fc1.bias
        out[q + ".fc2.kernel"], out[q + ".fc2.bias"] = fc2.kernel, fc2.bias

    for s, stage in enumerate(stages[:-1]):
        pe, t0, peg, t1 = stage.layers
        pre = f"svt_layers.{s}"
        out[pre + ".patch_embedding.proj.kernel"], out[pre + ".patch_embedding.proj.bias"] = pe.proj.kernel, pe.proj.bias
        for ti, tr in ((0, t0), (1, t1)):
            if ti == 1:
                out[pre + ".peg.kernel"], out[pre + ".peg.bias"] = peg.proj.fn.kernel, peg.proj.fn.bias
            for l, (la, f1, ga, f2) in enumerate(tr.layers):
                q = f"{pre}.transformer.{ti}.{l}"
                if hasattr(la, "fn"):      # Identity at the last stage
                    attn(q + ".local_attn", la)
                    ff(q + ".ff1", f1)
                attn(q + ".global_attn", ga)
                ff(q + ".ff2", f2)
    head = stages[-1].layers[1]
    out["head.kernel"], out["head.bias"] = head.kernel, head.bias
    return out


def make(case: str, b: int = 2) -> dict:
    from oracle.gen_ref_fixtures import _import_reference
    (H, W), kw = CASES[case]
    nest_gen.install_shim_extras()
    tf_shim.seed(1234)
    with twins_layers_installed():
        mod = _import_reference("twins_svt")
        model = mod.TwinsSVT(**kw)
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.standard_normal((b, H, W, 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    model(x)                                                   # Keras builds the layers on the first call
    ref_vars = reference_variables(model)
    table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
    P = twins_ref.init_params(table, seed=1)
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
    return nest_gen.load(case)


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return twins_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case][1])


def image_of(case: str):
    return CASES[case][0]


def _cut(k, v):
    """Pieces of at most PART_BYTES along the first axis (load() concatenates them again)."""
    if v.nbytes <= PART_BYTES:
        return [(k, v)]
    n = -(-v.nbytes // PART_BYTES)
    assert v.shape[0] >= n, k
    return [(f"{k}@{i}", piece) for i, piece in enumerate(np.array_split(v, n, axis=0))]


def main(argv):
    for case in (argv or list(CASES)):
        out = make(case)
        for old in glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz")):
            os.remove(old)
        items = []
        for k, v in out.items():
            items += _cut(k, v)
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
