"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_cvt_*.npz by EXECUTING THE REFERENCE'S OWN cvt.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  Conv2D (strided 'SAME', depthwise) and
GlobalAvgPool2D are the stand-ins of tools/gen_twins_fixtures.py; one more is installed here under the same rule:

  * BatchNormalization(momentum, epsilon) over the last axis: under a truthy `training` the mean and the biased variance over every other axis
    of the batch, otherwise moving_mean / moving_variance; (x - mean) * rsqrt(var + epsilon) * gamma + beta.  The moving statistics are not
    updated (the fixtures hold no state that depends on the update rule).

tests/test_cvt_oracle.py checks it against torch.nn.functional.batch_norm and the Conv2D against torch's conv2d on explicitly padded tensors.

cvt.py's own default runs the model with training=True; with dropout 0.0 every Dropout is the identity, so that is the deterministic path
and the fixtures are generated that way.  `cvt_eval` calls with training=False (logits only).

Seeded weights (tests/cvt_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img, dlogits, logits,
dimg, every gradient and the name / shape table, in files of at most PART_BYTES of arrays, cut and put together as NesT's are.

    python tools/gen_cvt_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import cvt_ref  # noqa: E402

GOLDEN = nest_gen.GOLDEN
PART_BYTES = nest_gen.PART_BYTES
Conv2D, GlobalAvgPool2D = twins_gen.Conv2D, twins_gen.GlobalAvgPool2D


def _stages(**cols):
    """emb_dim=(a, b, c), ... -> s1_emb_dim=a, s2_emb_dim=b, ..."""
    return {f"s{i + 1}_{k}": v[i] for k, v in cols.items() for i in range(3)}


_ODD = dict(num_classes=5, **_stages(emb_dim=(4, 8, 4), emb_kernel=(3, 3, 3), emb_stride=(2, 1, 2), proj_kernel=(3, 3, 3), kv_proj_stride=(2, 2, 2),
                                     heads=(2, 1, 1), depth=(1, 2, 1), mlp_mult=(2, 1, 2)))
# case -> ((H, W), constructor kwargs, training)
CASES = {
    # 7/4 embedding (pads 1 in front, 2 behind); maps 4x4, 2x2, 1x1 with 4, 1, 1 keys (3/2 on even maps: 0 in front, 1 behind); one key: the q
    # branch's true gradients are zero; BatchNorm over 2 samples at the last stage
    "cvt_tiny": ((16, 16), dict(num_classes=5, **_stages(emb_dim=(4, 8, 8), emb_kernel=(7, 3, 3), emb_stride=(4, 2, 2), proj_kernel=(3, 3, 3),
                                                         kv_proj_stride=(2, 2, 2), heads=(1, 2, 1), depth=(1, 1, 2), mlp_mult=(2, 2, 1))), True),
    # odd maps: 9x13 -> 5x7 (35 queries, 3x4 = 12 keys), again 5x7 (emb stride 1, depth 2), then 3x4 against 2x2
    "cvt_odd": ((9, 13), _ODD, True),
    # proj_kernel 5 with kv stride 3 on 7x10 (70 queries, 12 keys); a 5/3 embedding to 3x4 with proj_kernel 5 (taller than the map) and kv
    # stride 1 (keys = queries); an even (2/2) embedding to 2x2 with proj_kernel 1, stride 2: one key
    "cvt_k5s3": ((7, 10), dict(num_classes=4, **_stages(emb_dim=(4, 4, 8), emb_kernel=(3, 5, 2), emb_stride=(1, 3, 2), proj_kernel=(5, 5, 1),
                                                        kv_proj_stride=(3, 1, 2), heads=(1, 2, 1), depth=(1, 1, 1), mlp_mult=(1, 2, 1))), True),
    # cvt_odd's configuration called with training=False: BatchNorm on the (seeded, non-trivial) moving statistics.  Logits only.
    "cvt_eval": ((9, 13), _ODD, False),
}


# ------------------------------------------------------------------------------------------------ shim extras
class BatchNormalization(tf_shim.Layer):
    """nn.BatchNormalization(momentum, epsilon) over the last axis; see the module docstring."""

    def __init__(self, momentum=0.99, epsilon=1e-3, **kw):
        super().__init__(**kw)
        self.momentum, self.epsilon = float(momentum), float(epsilon)
        self.gamma = self.beta = self.moving_mean = self.moving_variance = None

    def build(self, input_shape):
        c = int(input_shape[-1])
        self.gamma = tf_shim.Variable(torch.ones(c, dtype=tf_shim.DTYPE))
        self.beta = tf_shim.Variable(torch.zeros(c, dtype=tf_shim.DTYPE))
        self.moving_mean = tf_shim.Variable(torch.zeros(c, dtype=tf_shim.DTYPE), trainable=False)
        self.moving_variance = tf_shim.Variable(torch.ones(c, dtype=tf_shim.DTYPE), trainable=False)
        self._weights = [self.gamma, self.beta, self.moving_mean, self.moving_variance]

    def call(self, inputs, training=None):
        x = tf_shim._t(inputs)
        if training:
            axes = tuple(range(x.dim() - 1))
            mean = x.mean(dim=axes)
            var = ((x - mean) ** 2).mean(dim=axes)
        else:
            mean, var = self.moving_mean, self.moving_variance
        return (x - mean) * torch.rsqrt(var + self.epsilon) * self.gamma + self.beta


@contextlib.contextmanager
def cvt_layers_installed():
    """nn.Conv2D / nn.GlobalAvgPool2D / nn.BatchNormalization are the stand-ins while a CvT is constructed, and what they were again afterwards."""
    with twins_gen.twins_layers_installed():
        import tensorflow.keras.layers as nn
        saved = getattr(nn, "BatchNormalization", None)
        nn.BatchNormalization = BatchNormalization
        try:
            yield
        finally:
            if saved is None:
                del nn.BatchNormalization
            else:
                nn.BatchNormalization = saved


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    stages = model.cvt_layers.layers
    for s, stage in enumerate(stages[:-1]):
        emb, norm, tr = stage.layers
        pre = f"cvt_layers.{s}"
        out[pre + ".embed.kernel"], out[pre + ".embed.bias"] = emb.kernel, emb.bias
        out[pre + ".norm.g"], out[pre + ".norm.b"] = norm.g, norm.b
        for l, (attn, ff) in enumerate(tr.layers):
            q = f"{pre}.transformer.{l}"
            out[q + ".attn.norm.g"], out[q + ".attn.norm.b"] = attn.norm.g, attn.norm.b
            for name, proj in (("to_q", attn.fn.to_q), ("to_kv", attn.fn.to_kv)):
                dw, bn, pw = proj.net.layers
                out[f"{q}.attn.{name}.dw.kernel"] = dw.kernel
                for leaf in cvt_ref.BN_LEAVES:
                    out[f"{q}.attn.{name}.bn.{leaf}"] = getattr(bn, leaf)
                out[f"{q}.attn.{name}.pw.kernel"] = pw.kernel
            to_out = attn.fn.to_out.layers[0]
            out[q + ".attn.to_out.kernel"], out[q + ".attn.to_out.bias"] = to_out.kernel, to_out.bias
            fc1, fc2 = ff.fn.net.layers[0], ff.fn.net.layers[3]
            out[q + ".ff.norm.g"], out[q + ".ff.norm.b"] = ff.norm.g, ff.norm.b
            out[q + ".ff.fc1.kernel"], out[q + ".ff.fc1.bias"] = fc1.kernel, fc1.bias
            out[q + ".ff.fc2.kernel"], out[q + ".ff.fc2.bias"] = fc2.kernel, fc2.bias
    head = stages[-1].layers[1]
    out["head.kernel"], out["head.bias"] = head.kernel, head.bias
    return out


def build_reference(kw: dict, H: int, W: int, b: int = 2):
    """(model, {table name: variable}) of the reference's CvT(**kw), built by one call on a zero image."""
    from oracle.gen_ref_fixtures import _import_reference
    nest_gen.install_shim_extras()
    tf_shim.seed(1234)
    with cvt_layers_installed():
        mod = _import_reference("cvt")
        model = mod.CvT(**kw)
    model(torch.zeros((b, H, W, 3), dtype=torch.float64).as_subclass(tf_shim._T))   # Keras builds the layers on the first call
    return model, reference_variables(model)


def make(case: str, b: int = 2) -> dict:
    (H, W), kw, training = CASES[case]
    model, ref_vars = build_reference(kw, H, W, b)
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.standard_normal((b, H, W, 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
    P = cvt_ref.init_params(table, seed=1)
    for n, v in ref_vars.items():
        tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
    logits = model(x, training=training)
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": logits.detach().numpy().astype(np.float64),
           "param_seed": np.int64(1), "training": np.int64(int(training)),
           "names": np.array(list(ref_vars)), "shapes": np.array([",".join(str(s) for s in t[1]) for t in table])}
    if not training:
        return out
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
    trainable = {n: v for n, v in ref_vars.items() if not cvt_ref.is_moving(n)}
    grads = torch.autograd.grad(loss, [x] + list(trainable.values()), allow_unused=True)
    out["dimg"] = grads[0].numpy().astype(np.float64)
    for (n, v), g in zip(trainable.items(), grads[1:]):
        out["grad/" + n] = (np.zeros(tuple(v.shape)) if g is None else g.numpy().astype(np.float64)).reshape(tuple(v.shape))
    return out


def load(case: str) -> dict:
    return nest_gen.load(case)


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return cvt_ref.init_params(table, seed=int(z["param_seed"]))


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
            items += twins_gen._cut(k, v)
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
