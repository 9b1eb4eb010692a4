"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Writes tests/golden/ref_rv_*.npz by EXECUTING THE REFERENCE'S OWN regionvit.py (imported unmodified through
oracle.gen_ref_fixtures._import_reference, under the float64 torch shim oracle/tf_shim).  Conv2D (strided 'SAME', depthwise for the PEG),
tf.stack and tf.meshgrid are the stand-ins tools/gen_crossformer_fixtures.py installs; two more names are installed on the shim module here,
at run time, under the earlier generators' rule:

  * tf.pad(tensor, paddings) IS torch's constant zero pad with the [before, after] pairs taken per axis, first axis first;
  * tf.convert_to_tensor(value) IS the value as a shim tensor.

tests/test_regionvit_oracle.py checks both against numpy.

regionvit.py's own default runs the model with training=True; with ff_dropout 0.0 every Dropout is the identity, so that is the deterministic
path and the fixtures are generated that way.

Seeded weights (tests/regionvit_ref.py:init_params) are loaded into the reference's variables by table name; a fixture holds img, dlogits,
logits, dimg, every gradient and the name / shape table, in files of at most PART_BYTES of arrays, cut and put together as NesT's are.
Asserted when a fixture is written: autograd returns None exactly for the relative-position embeddings of the stages without layers (the
fixture holds zeros); every other embedding gradient is non-zero, except that of the last stage with layers when its depth is 1, which is
exactly zero (its only layer's local tokens reach nothing); zeroing every embedding moves the float64 logits by at least 1e-2 of their spread.

    python tools/gen_regionvit_fixtures.py [case ...]     # needs the reference staged in oracle/_ref (build()) or VITX_REFERENCE_DIR
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
import gen_crossformer_fixtures as cf_gen  # noqa: E402
import regionvit_ref  # noqa: E402

GOLDEN = nest_gen.GOLDEN
PART_BYTES = nest_gen.PART_BYTES

# case -> ((H, W), constructor kwargs)
CASES = {
    # the 50-token usage window at stage 0, then rectangular windows of 4x7, 2x4 and 1x2 (region maps 1x2, 1x1, 1x1, 1x1); the last stage's
    # embedding gradient is exactly zero
    "rv_rect": ((28, 56), dict(dim=32, depth=1, window_size=7, num_classes=5)),
    # 5-token windows, region sequences of 64, 16, 4 and 1, a bias shared by two layers, PEG, the 3-conv encoder, the shared Downsample
    "rv_small": ((64, 64), dict(dim=(32, 32, 64, 32), depth=(1, 2, 1, 1), window_size=2, use_peg=True, tokenize_local_3_conv=True, num_classes=4)),
    # a 2x2 window under window_size 4: the index stride is 7
    "rv_lps2": ((32, 32), dict(dim=32, depth=1, window_size=4, local_patch_size=2, num_classes=3)),
    # 197 tokens, then a 50-token stage at a bf16 width; two stages without layers
    "rv_w14": ((56, 56), dict(dim=64, depth=(1, 1, 0, 0), window_size=14, num_classes=3)),
    # bf16 widths at every stage; the last stage two layers deep (its embedding gradient is non-zero)
    "rv_bf16": ((64, 64), dict(dim=64, depth=(1, 1, 1, 2), window_size=2, num_classes=5)),
}


# ------------------------------------------------------------------------------------------------ shim extras
def pad(tensor, paddings, mode="CONSTANT", constant_values=0, name=None):
    assert str(mode).upper() == "CONSTANT"
    flat = []
    for before, after in reversed([tuple(int(v) for v in p) for p in paddings]):   # torch pads the last axis first
        flat += [before, after]
    return tf_shim._t(torch.nn.functional.pad(tf_shim._t(tensor), flat, value=constant_values))


def convert_to_tensor(value, dtype=None, name=None):
    return tf_shim._t(torch.as_tensor(np.asarray(value)))


@contextlib.contextmanager
def regionvit_layers_installed():
    with cf_gen.crossformer_layers_installed():
        import tensorflow as tf
        tf.pad, tf.convert_to_tensor = pad, convert_to_tensor
        yield


# ------------------------------------------------------------------------------------------------ table name -> the reference's variable
def reference_variables(model, kw: dict) -> dict:
    """Library table name -> the reference's variable, in the library's order."""
    out = {}
    if kw.get("tokenize_local_3_conv"):
        L = model.local_encoder.layers
        for i in (0, 3, 6):
            out[f"local_encoder.{i}.kernel"], out[f"local_encoder.{i}.bias"] = L[i].kernel, L[i].bias
            if i < 6:
                out[f"local_encoder.{i + 1}.gamma"], out[f"local_encoder.{i + 1}.beta"] = L[i + 1].gamma, L[i + 1].beta
    else:
        out["local_encoder.kernel"], out["local_encoder.bias"] = model.local_encoder.kernel, model.local_encoder.bias
    conv = model.region_encoder.layers[1]
    out["region_encoder.1.kernel"], out["region_encoder.1.bias"] = conv.kernel, conv.bias
    for s, (down, peg, tr) in enumerate(model.region_layers):
        pre = f"region_layers.{s}"
        if hasattr(down, "conv"):
            out[pre + ".down.conv.kernel"], out[pre + ".down.conv.bias"] = down.conv.kernel, down.conv.bias
        if hasattr(peg, "proj"):
            out[pre + ".peg.proj.kernel"], out[pre + ".peg.proj.bias"] = peg.proj.kernel, peg.proj.bias
        out[pre + ".transformer.local_rel_pos_bias"] = tr.local_rel_pos_bias.embeddings
        for l, (a, f) in enumerate(tr.layers):
            q = f"{pre}.transformer.{l}"
            out[q + ".attn.norm.gamma"], out[q + ".attn.norm.beta"] = a.norm.gamma, a.norm.beta
            out[q + ".attn.to_qkv.kernel"] = a.to_qkv.kernel
            out[q + ".attn.to_out.kernel"], out[q + ".attn.to_out.bias"] = a.to_out.kernel, a.to_out.bias
            norm, fc1, fc2 = f.net.layers[0], f.net.layers[1], f.net.layers[4]
            out[q + ".ff.norm.gamma"], out[q + ".ff.norm.beta"] = norm.gamma, norm.beta
            out[q + ".ff.fc1.kernel"], out[q + ".ff.fc1.bias"] = fc1.kernel, fc1.bias
            out[q + ".ff.fc2.kernel"], out[q + ".ff.fc2.bias"] = fc2.kernel, fc2.bias
    norm, head = model.to_logits.layers[1], model.to_logits.layers[2]
    out["to_logits.norm.gamma"], out["to_logits.norm.beta"] = norm.gamma, norm.beta
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
    with regionvit_layers_installed():        # (the reference looks tf.pad / tf.stack / ... up at call time)
        mod = _import_reference("regionvit")
        model = mod.RegionViT(**kw)
        model(x)                                                   # Keras builds the layers on the first call
        ref_vars = reference_variables(model, kw)
        table = [(n, tuple(int(d) for d in v.shape), 0) for n, v in ref_vars.items()]
        assert [(n, s) for n, s, _ in table] == [(n, s) for n, s, _ in regionvit_ref.table_of(kw)], "table order / shapes"
        P = regionvit_ref.init_params(table, seed=1)
        for n, v in ref_vars.items():
            tf_shim.assign(v, P[n].reshape(tuple(v.shape)))
        logits = model(x)
        loss = (logits * torch.tensor(np.asarray(dlogits, np.float64))).sum()
        grads = torch.autograd.grad(loss, [x] + list(ref_vars.values()), allow_unused=True)
        # the embeddings must matter: zero them all and look at the logits again
        saved = {n: v.detach().clone() for n, v in ref_vars.items() if regionvit_ref.is_embedding(n)}
        for n in saved:
            tf_shim.assign(ref_vars[n], torch.zeros_like(saved[n]))
        unbiased = model(x).detach().numpy()
        for n, v in saved.items():
            tf_shim.assign(ref_vars[n], v)
    lg = logits.detach().numpy().astype(np.float64)
    moved, spread = np.abs(unbiased - lg).max(), lg.max() - lg.min()
    assert moved >= 1e-2 * spread, f"{case}: zeroing the embeddings moves the logits by {moved:.3e} of a spread of {spread:.3e}"
    depths = regionvit_ref.config_of(kw)["depth"]
    last = max(s for s in range(4) if depths[s] > 0)
    out = {"img": img.astype(np.float64), "dlogits": dlogits.astype(np.float64), "logits": lg,
           "dimg": grads[0].numpy().astype(np.float64), "param_seed": np.int64(1), "bias_effect": np.float64(moved / spread),
           "emb_scale": np.float64(regionvit_ref.EMB_SCALE),
           "names": np.array(list(ref_vars)), "shapes": np.array([",".join(str(s) for s in t[1]) for t in table])}
    for (n, v), g in zip(ref_vars.items(), grads[1:]):
        if regionvit_ref.is_embedding(n):
            s = int(n.split(".")[1])
            assert (g is None) == (depths[s] == 0), n                # exactly the embeddings of the stages without layers are off the tape
            if g is not None:
                dead = s == last and depths[s] == 1
                assert bool((g == 0).all()) == dead, (n, float(g.abs().max()))
        else:
            assert g is not None, n
        out["grad/" + n] = (np.zeros(tuple(v.shape)) if g is None else g.numpy().astype(np.float64)).reshape(tuple(v.shape))
    print(f"{case}: bias effect {moved / spread:.3e} of the logits' spread")
    return out


def load(case: str) -> dict:
    """A fixture put together; the gradients (stored as matrices so that a 4-d kernel can be cut by rows) in their table shapes."""
    z = nest_gen.load(case)
    for n, sh in zip(z["names"], z["shapes"]):
        z["grad/" + str(n)] = z["grad/" + str(n)].reshape(tuple(int(s) for s in str(sh).split(",")))
    return z


def params_of(z) -> dict:
    """The seeded weights a fixture was generated with (regenerated from its table)."""
    table = [(str(n), tuple(int(s) for s in str(sh).split(",")), 0) for n, sh in zip(z["names"], z["shapes"])]
    saved = regionvit_ref.EMB_SCALE
    regionvit_ref.EMB_SCALE = float(z["emb_scale"])
    try:
        return regionvit_ref.init_params(table, seed=int(z["param_seed"]))
    finally:
        regionvit_ref.EMB_SCALE = saved


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
