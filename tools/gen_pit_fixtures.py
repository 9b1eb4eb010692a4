"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_pit_*.npz by EXECUTING THE REFERENCE'S OWN pit.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).

One name is installed on the shim here, at run time, under the earlier generators' rule: nn.Conv2D.  The Twins generator's stand-in asserts
"groups: 1 or depthwise" and rejects Pool's Conv2D(filters = 2 dim, groups = dim) (pit.py:130).  This file's stand-in is the same
extract_patches + product, with a channel multiplier: for groups == input channels and filters = m * groups, output channel o reads input
channel o // m through kernel[:, :, 0, o] (Keras / TensorFlow's grouped-convolution channel order).  check_standin() compares it with
torch.nn.functional.conv2d(groups=...) on explicitly, unevenly padded input; tests/test_pit_oracle.py runs that check.

pit.py:194 `not_last = ind < (len(depth) < 1)` is never true, so the reference's PiT holds Transformers only: pit_small records the class names
in PiT.transformer_layers.  pit_pooled and pit_w64 are COMPOSED here from the reference's own patch_embedding, pos_embedding, cls_token,
Transformer, Pool and mlp_head objects in the order of pit.py:193-200 with not_last true (the file's evident intent, not reference behaviour).
pit_pool_layer is the reference's Pool(8) alone on maps 7 x 7 (pads 1 | 1), 6 x 6 (0 | 1), 2 x 2 and 1 x 1.

The reference's default runs with training=True; with dropout 0.0 every Dropout is the identity, so that is the deterministic path.
Seeded weights (tests/pit_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img (or tokens), the
cotangent, the outputs, d(input), every gradient and the name / shape table, in files of at most PART_BYTES of arrays, cut and put together as
NesT's are.

    python tools/gen_pit_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import pit_ref  # noqa: E402

GOLDEN = nest_gen.GOLDEN
PART_BYTES = nest_gen.PART_BYTES
POOL_MAPS = (7, 6, 2, 1)
POOL_DIM = 8

# case -> constructor kwargs (pool_stages is this project's switch, not the reference's)
CASES = {
    # 7 x 7 + 1 = 50 tokens; stage 0 has no to_out (heads 1, dim_head == dim); the reference as it is: no Pool
    "pit_small": dict(image_size=32, patch_size=8, num_classes=5, dim=16, depth=(1, 2, 1), heads=(1, 2, 4), dim_head=16, mlp_dim=24),
    # odd patch, stride 3: 8 x 8 + 1 tokens; int heads, dim_head != dim
    "pit_odd": dict(image_size=28, patch_size=7, num_classes=3, dim=12, depth=(1, 1), heads=2, dim_head=8, mlp_dim=16),
    # pooling between stages: 49 -> 16 -> 4 patch tokens, widths 8 -> 16 -> 32
    "pit_pooled": dict(image_size=32, patch_size=8, num_classes=4, dim=8, depth=(1, 1, 1), heads=(1, 2, 2), dim_head=8, mlp_dim=16, pool_stages=True),
    # bf16 widths: 64 -> 128, heads of 64, 49 -> 16 patch tokens
    "pit_w64": dict(image_size=32, patch_size=8, num_classes=5, dim=64, depth=(1, 1), heads=(2, 2), dim_head=64, mlp_dim=128, pool_stages=True),
}


# ------------------------------------------------------------------------------------------------ shim extra
class Conv2D(tf_shim.Layer):
    """nn.Conv2D(filters, kernel_size, strides, padding, use_bias, groups) as extract_patches + a product with the kernel + bias; groups > 1:
    one input channel per group, filters / groups outputs each (output o reads input channel o // (filters / groups))."""

    def __init__(self, filters, kernel_size, strides=1, padding="valid", use_bias=True, groups=1, **kw):
        super().__init__(**kw)
        self.filters, self.k, self.s, self.use_bias, self.groups = int(filters), int(kernel_size), int(strides), bool(use_bias), int(groups)
        self.padding = "SAME" if str(padding).upper() == "SAME" else "VALID"
        self.kernel = self.bias = None

    def build(self, input_shape):
        cin = int(input_shape[-1])
        assert self.groups == 1 or (self.groups == cin and self.filters % self.groups == 0), "groups: 1, or one input channel per group"
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
            src = torch.arange(self.filters) // (self.filters // self.groups)          # the input channel of every output
            taps = rows.reshape(b, oh, ow, self.k * self.k, self.groups)[..., src]       # [b, oh, ow, k k, filters]
            y = (taps * self.kernel.reshape(self.k * self.k, self.filters)).sum(dim=3)
        return y + self.bias if self.use_bias else y


@contextlib.contextmanager
def pit_layers_installed():
    """nn.Conv2D is this file's while the reference's layers are constructed, and what it was again afterwards."""
    nest_gen.install_shim_extras()
    import tensorflow.keras.layers as nn
    saved = nn.Conv2D
    nn.Conv2D = Conv2D
    try:
        yield
    finally:
        nn.Conv2D = saved


def check_standin():
    """The stand-in against torch.nn.functional.conv2d(groups=...) on input padded explicitly (and unevenly) by the 'SAME' rule: depthwise
    with a multiplier of 2 on an odd and an even map, and a multiplier of 3; the worst absolute difference.  (The layer needs the shim's
    module, not its registration as `tensorflow`: nothing is installed here.)"""
    rng = np.random.Generator(np.random.PCG64(5))
    worst = 0.0
    for (h, w, c, mult, k, s) in ((7, 7, 4, 2, 3, 2), (6, 6, 4, 2, 3, 2), (5, 4, 3, 3, 3, 2), (2, 2, 2, 2, 3, 2), (1, 1, 2, 2, 3, 2), (6, 5, 3, 1, 3, 1)):
        x = torch.tensor(rng.standard_normal((2, h, w, c)))
        layer = Conv2D(filters=c * mult, kernel_size=k, strides=s, padding="SAME", groups=c)
        got = layer(x.as_subclass(tf_shim._T))
        kern, bias = torch.tensor(rng.standard_normal((k, k, 1, c * mult))), torch.tensor(rng.standard_normal(c * mult))
        tf_shim.assign(layer.kernel, kern)
        tf_shim.assign(layer.bias, bias)
        got = torch.as_tensor(layer(x.as_subclass(tf_shim._T))).detach()
        (pt, pb), (pl, pr) = pit_ref.same_pads(h, k, s), pit_ref.same_pads(w, k, s)
        xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
        want = torch.nn.functional.conv2d(xp, kern.permute(3, 2, 0, 1), bias, stride=s, groups=c).permute(0, 2, 3, 1)
        assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
        worst = max(worst, float((got - want).abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def _transformer_vars(out: dict, pre: str, tr):
    for l, (a, f) in enumerate(tr.layers):
        q = f"{pre}.{l}"
        out[q + ".attn.norm.gamma"], out[q + ".attn.norm.beta"] = a.norm.gamma, a.norm.beta
        out[q + ".attn.to_qkv.kernel"] = a.fn.to_qkv.kernel
        if a.fn.to_out.layers:
            out[q + ".attn.to_out.kernel"], out[q + ".attn.to_out.bias"] = a.fn.to_out.layers[0].kernel, a.fn.to_out.layers[0].bias
        fc1, fc2 = f.fn.net.layers[0], f.fn.net.layers[3]
        out[q + ".ff.norm.gamma"], out[q + ".ff.norm.beta"] = f.norm.gamma, f.norm.beta
        out[q + ".ff.fc1.kernel"], out[q + ".ff.fc1.bias"] = fc1.kernel, fc1.bias
        out[q + ".ff.fc2.kernel"], out[q + ".ff.fc2.bias"] = fc2.kernel, fc2.bias


def _pool_vars(out: dict, pre: str, pool):
    dw, pw = pool.downsample.net.layers
    out[pre + "downsample.dw.kernel"], out[pre + "downsample.dw.bias"] = dw.kernel, dw.bias
    out[pre + "downsample.pw.kernel"], out[pre + "downsample.pw.bias"] = pw.kernel, pw.bias
    out[pre + "cls_ff.kernel"], out[pre + "cls_ff.bias"] = pool.cls_ff.kernel, pool.cls_ff.bias


def reference_variables(base, layers) -> dict:
    """Library table name -> the reference's variable, in the library's order; layers: [Transformer | Pool]."""
    out = {}
    dense = base.patch_embedding.layers[1]
    out["patch_embedding.kernel"], out["patch_embedding.bias"] = dense.kernel, dense.bias
    out["pos_embedding"], out["cls_token"] = base.pos_embedding, base.cls_token
    s = -1
    for layer in layers:
        if type(layer).__name__ == "Transformer":
            s += 1
            _transformer_vars(out, f"stage.{s}", layer)
        else:
            _pool_vars(out, f"pool.{s}.", layer)
    norm, head = base.mlp_head.layers
    out["mlp_head.norm.gamma"], out["mlp_head.norm.beta"] = norm.gamma, norm.beta
    out["mlp_head.kernel"], out["mlp_head.bias"] = head.kernel, head.bias
    return out


def _record(out: dict, ref_vars: dict, grads, table):
    out["names"] = np.array(list(ref_vars))
    out["shapes"] = np.array([",".join(str(s) for s in t[1]) for t in table])
    for (n, v), g in zip(ref_vars.items(), grads):
        assert g is not None, n
        out["grad/" + n] = g.numpy().astype(np.float64).reshape(tuple(v.shape))


def make(case: str, b: int = 2) -> dict:
    if case == "pit_pool_layer":
        return make_pool_layer(b)
    from oracle.gen_ref_fixtures import _import_reference
    kw = dict(CASES[case])
    pooled = kw.pop("pool_stages", False)
    nest_gen.install_shim_extras()
    tf_shim.seed(1234)
    rng = np.random.Generator(np.random.PCG64(7))
    img = rng.standard_normal((b, kw["image_size"], kw["image_size"], 3)).astype(np.float32)
    dlogits = (rng.standard_normal((b, kw["num_classes"])) / b).astype(np.float32)
    x = torch.tensor(np.asarray(img, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
    with pit_layers_installed():
        mod = _import_reference("pit")
        base = mod.PiT(**kw)
        classes = [type(l).__name__ for l in base.transformer_layers.layers]
        assert classes == ["Transformer"] * len(kw["depth"]), classes      # the dead `not_last` (pit.py:194)
        if not pooled:
            layers = list(base.transformer_layers.layers)
            model = base
        else:
            # the reference's own objects, one Transformer per stage and a Pool behind every stage but the last, the width doubling there
            # (what pit.py:196-200 would build if not_last were ever true); the glue between them is plain torch
            layers = []
            for s, (stage_depth, stage_heads, width, has_pool) in enumerate(pit_ref.stages_of(dict(kw, pool_stages=True))):
                layers.append(mod.Transformer(width, stage_depth, stage_heads, kw["dim_head"], kw["mlp_dim"], 0.0))
                if has_pool:
                    layers.append(mod.Pool(width))

            def model(im):
                patches = torch.as_tensor(base.patch_embedding(im))
                rows = patches.shape[1] + 1
                cls = torch.as_tensor(base.cls_token).expand(patches.shape[0], 1, patches.shape[2])
                t = (torch.cat([cls, patches], dim=1) + torch.as_tensor(base.pos_embedding)[:, :rows]).as_subclass(tf_shim._T)
                for layer in layers:
                    t = layer(t, training=True)
                return base.mlp_head(t[:, 0])
        model(x)                                                           # Keras builds the layers on the first call
        ref_vars = reference_variables(base, layers)
        table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
        want = pit_ref.table_of(dict(CASES[case]))
        assert [(n, s) for n, s, _ in table] == [(n, s) for n, s, _ in want], "table order / shapes"
        P = pit_ref.init_params(table, seed=1)
        for n, v in ref_vars.items():
            tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
        logits = model(x)
        loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
        grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()), allow_unused=True)
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": logits.detach().numpy().astype(np.float64),
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1), "layer_classes": np.array(classes)}
    _record(out, ref_vars, grads[1:], table)
    return out


def make_pool_layer(b: int = 2) -> dict:
    from oracle.gen_ref_fixtures import _import_reference
    nest_gen.install_shim_extras()
    tf_shim.seed(1234)
    rng = np.random.Generator(np.random.PCG64(11))
    out = {"param_seed": np.int64(3), "maps": np.array(POOL_MAPS, np.int64), "dim": np.int64(POOL_DIM)}
    with pit_layers_installed():
        mod = _import_reference("pit")
        pool = mod.Pool(POOL_DIM)
        for i, hw in enumerate(POOL_MAPS):
            tokens = rng.standard_normal((b, 1 + hw * hw, POOL_DIM)).astype(np.float32)
            no = 1 + (-(-hw // 2)) ** 2
            dout = (rng.standard_normal((b, no, 2 * POOL_DIM)) / b).astype(np.float32)
            x = torch.tensor(np.asarray(tokens, np.float64)).as_subclass(tf_shim._T).requires_grad_(True)
            if i == 0:
                pool(x)
                ref_vars = {}
                _pool_vars(ref_vars, "", pool)
                table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
                assert [(n, s) for n, s, _ in table] == pit_ref.pool_table(POOL_DIM, ""), "table order / shapes"
                P = pit_ref.init_params(table, seed=3)
                for n, v in ref_vars.items():
                    tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
                out["names"] = np.array(list(ref_vars))
                out["shapes"] = np.array([",".join(str(s) for s in t[1]) for t in table])
            y = pool(x)
            assert tuple(y.shape) == (b, no, 2 * POOL_DIM), (hw, tuple(y.shape))
            grads = torch.autograd.grad((y * torch.tensor(np.asarray(dout, np.float64))).sum(), [x] + list(ref_vars.values()))
            out[f"tokens_{hw}"], out[f"dout_{hw}"] = tokens.astype(np.float64), dout.astype(np.float64)
            out[f"out_{hw}"], out[f"dtokens_{hw}"] = y.detach().numpy().astype(np.float64), grads[0].numpy().astype(np.float64)
            for (n, v), g in zip(ref_vars.items(), grads[1:]):
                out[f"grad_{hw}/" + n] = g.numpy().astype(np.float64).reshape(tuple(v.shape))
    return out


def load(case: str) -> dict:
    """A fixture put together; the gradients (stored as matrices so that a 4-d kernel can be cut by rows) in their table shapes."""
    z = nest_gen.load(case)
    shapes = {str(n): tuple(int(s) for s in str(sh).split(",")) for n, sh in zip(z["names"], z["shapes"])}
    for k in list(z):
        if k.startswith("grad") and "/" in k:
            z[k] = z[k].reshape(shapes[k.split("/", 1)[1]])
    return z


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    return pit_ref.init_params(table, seed=int(z["param_seed"]))


def kwargs_of(case: str) -> dict:
    return dict(CASES[case])


def main(argv):
    print(f"stand-in against torch conv2d(groups): worst |difference| {check_standin():.3e}")
    for case in (argv or list(CASES) + ["pit_pool_layer"]):
        out = make(case)
        for old in glob.glob(os.path.join(GOLDEN, f"ref_{case}.part*.npz")):
            os.remove(old)
        items = []
        for k, v in out.items():
            items += twins_gen._cut(k, v.reshape(-1, v.shape[-1]) if k.startswith("grad") and "/" in k else v)
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
