"""Op-for-op float64 torch restatement of the reference's PiT and Pool (pit.py:91-219) on the deterministic path (dropout 0), on parameters
keyed by the library's table names.  Pinned to the reference by tests/golden/ref_pit_*.npz (tests/test_pit_oracle.py);
used by the GPU tier for the shapes no fixture covers.

Stated independently of the library's formulation: the overlapping patches are torch's unfold on NCHW with the feature axis permuted to
TensorFlow's (kh, kw, c), the depthwise convolution with its channel multiplier is torch's conv2d(groups = dim) on a map padded explicitly by
the 'SAME' rule, and Pool rearranges its tokens into a map as the reference does.  The parameter table is computed here from the constructor
arguments, not read from the library.

pit.py:194 `not_last = ind < (len(depth) < 1)` is never true: `pool_stages=False` (no Pool, one width) is the reference.  `pool_stages=True`
composes the reference's pieces in the order of :193-200 with not_last true."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-3   # Keras LayerNormalization's default epsilon (pit.py:23,203)


def cast_tuple(val, num):
    return val if isinstance(val, tuple) else (val,) * num


def conv_output_size(image_size, kernel_size, stride, padding=0):
    return int(((image_size - kernel_size + (2 * padding)) / stride) + 1)


def same_pads(extent: int, k: int, s: int):
    """(pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), the smaller half first."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return total // 2, total - total // 2


def stages_of(kw: dict):
    """[(depth, heads, width, pool_behind)] of zip(depth, cast_tuple(heads, len(depth)))."""
    depth = kw["depth"]
    heads = cast_tuple(kw["heads"], len(depth))
    pairs = list(zip(depth, heads))
    out, d = [], kw["dim"]
    for i, (dp, h) in enumerate(pairs):
        pool = bool(kw.get("pool_stages")) and i + 1 < len(pairs)
        out.append((dp, h, d, pool))
        if pool:
            d *= 2
    return out


def pool_table(d: int, pre: str):
    return [(pre + "downsample.dw.kernel", (3, 3, 1, 2 * d)), (pre + "downsample.dw.bias", (2 * d,)),
            (pre + "downsample.pw.kernel", (1, 1, 2 * d, 2 * d)), (pre + "downsample.pw.bias", (2 * d,)),
            (pre + "cls_ff.kernel", (d, 2 * d)), (pre + "cls_ff.bias", (2 * d,))]


def _with_offsets(t):
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in attribute order, shapes as the reference holds them."""
    p, dim, dh, mlp = kw["patch_size"], kw["dim"], kw.get("dim_head", 64), kw["mlp_dim"]
    out = conv_output_size(kw["image_size"], p, p // 2)
    t = [("patch_embedding.kernel", (p * p * 3, dim)), ("patch_embedding.bias", (dim,)), ("pos_embedding", (1, out * out + 1, dim)),
         ("cls_token", (1, 1, dim))]
    d = dim
    for s, (depth, heads, d, pool) in enumerate(stages_of(kw)):
        inner = heads * dh
        for l in range(depth):
            q = f"stage.{s}.{l}"
            t += [(q + ".attn.norm.gamma", (d,)), (q + ".attn.norm.beta", (d,)), (q + ".attn.to_qkv.kernel", (d, 3 * inner))]
            if not (heads == 1 and dh == d):
                t += [(q + ".attn.to_out.kernel", (inner, d)), (q + ".attn.to_out.bias", (d,))]
            t += [(q + ".ff.norm.gamma", (d,)), (q + ".ff.norm.beta", (d,)), (q + ".ff.fc1.kernel", (d, mlp)), (q + ".ff.fc1.bias", (mlp,)),
                  (q + ".ff.fc2.kernel", (mlp, d)), (q + ".ff.fc2.bias", (d,))]
        if pool:
            t += pool_table(d, f"pool.{s}.")
    dl = d   # the last stage's width
    t += [("mlp_head.norm.gamma", (dl,)), ("mlp_head.norm.beta", (dl,)), ("mlp_head.kernel", (dl, kw["num_classes"])),
          ("mlp_head.bias", (kw["num_classes"],))]
    return _with_offsets(t)


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table: every tensor moved off its default so that each gradient is exercised.  Kernels are scaled by their fan-in."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "gamma":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        elif name in ("pos_embedding", "cls_token"):
            a = rng.standard_normal(shape)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def _ln(x, P, pre):
    return F.layer_norm(x, x.shape[-1:], P[pre + ".gamma"], P[pre + ".beta"], LN_EPS)


def transformer(x, P, pre: str, depth: int, heads: int, dh: int):
    """pit.py:91-108 with Attention (:55-89) and MLP (:29-53)."""
    b, n, d = x.shape
    for l in range(depth):
        q = f"{pre}.{l}"
        y = _ln(x, P, q + ".attn.norm")
        qkv = (y @ P[q + ".attn.to_qkv.kernel"]).reshape(b, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
        attn = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * dh ** -0.5, dim=-1)
        o = (attn @ qkv[2]).permute(0, 2, 1, 3).reshape(b, n, heads * dh)
        if (q + ".attn.to_out.kernel") in P:
            o = o @ P[q + ".attn.to_out.kernel"] + P[q + ".attn.to_out.bias"]
        x = o + x
        y = _ln(x, P, q + ".ff.norm")
        y = y @ P[q + ".ff.fc1.kernel"] + P[q + ".ff.fc1.bias"]
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
        x = y @ P[q + ".ff.fc2.kernel"] + P[q + ".ff.fc2.bias"] + x
    return x


def pool(x, P, pre: str = ""):
    """Pool.call (pit.py:146-156) on [b, 1 + h h, d] -> [b, 1 + ceil(h / 2)^2, 2 d]."""
    b, n, d = x.shape
    h = int(math.sqrt(n - 1))
    if h * h != n - 1:
        raise ValueError(f"Pool: {n - 1} tokens are not a square map")
    cls = x[:, :1] @ P[pre + "cls_ff.kernel"] + P[pre + "cls_ff.bias"]
    t = x[:, 1:].reshape(b, h, h, d).permute(0, 3, 1, 2)
    pt, pb = same_pads(h, 3, 2)
    t = F.pad(t, (pt, pb, pt, pb))
    t = F.conv2d(t, P[pre + "downsample.dw.kernel"].permute(3, 2, 0, 1), P[pre + "downsample.dw.bias"], stride=2, groups=d)
    t = F.conv2d(t, P[pre + "downsample.pw.kernel"].permute(3, 2, 0, 1), P[pre + "downsample.pw.bias"])
    t = t.permute(0, 2, 3, 1).reshape(b, -1, 2 * d)
    return torch.cat([cls, t], dim=1)


def unfold(img, p: int, st: int):
    """tf.image.extract_patches(sizes p, strides st, 'VALID') as rows [b, oh ow, p p c] in (kh, kw, c) order (pit.py:119-120)."""
    b, H, W, c = img.shape
    u = F.unfold(img.permute(0, 3, 1, 2), kernel_size=p, stride=st)            # [b, c p p, L], features (c, kh, kw)
    return u.reshape(b, c, p, p, -1).permute(0, 4, 2, 3, 1).reshape(b, -1, p * p * c)


def forward(kw: dict, P: dict, img, taps: dict | None = None):
    """PiT.call (pit.py:207-219); `taps` collects 'tokens', 'stage.<s>' and 'pooled.<s>'."""
    p, dh = kw["patch_size"], kw.get("dim_head", 64)
    x = unfold(img, p, p // 2) @ P["patch_embedding.kernel"] + P["patch_embedding.bias"]
    b, n, d = x.shape
    x = torch.cat([P["cls_token"].expand(b, 1, d), x], dim=1)
    if n + 1 > P["pos_embedding"].shape[1]:
        raise ValueError(f"the image makes {n + 1} tokens, pos_embedding has {P['pos_embedding'].shape[1]} rows")
    x = x + P["pos_embedding"][:, :n + 1]
    if taps is not None:
        taps["tokens"] = x
    for s, (depth, heads, width, has_pool) in enumerate(stages_of(kw)):
        x = transformer(x, P, f"stage.{s}", depth, heads, dh)
        if taps is not None:
            taps[f"stage.{s}"] = x
        if has_pool:
            x = pool(x, P, f"pool.{s}.")
            if taps is not None:
                taps[f"pooled.{s}"] = x
    return _ln(x[:, 0], P, "mlp_head.norm") @ P["mlp_head.kernel"] + P["mlp_head.bias"]


def run(kw: dict, params: dict, img, dlogits):
    """(logits, {name: grad}, dimg) in float64."""
    P = {n: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), requires_grad=True)
    logits = forward(kw, P, x)
    names = list(P)
    grads = torch.autograd.grad((logits * torch.tensor(np.asarray(dlogits, np.float64))).sum(), [x] + [P[n] for n in names], allow_unused=True)
    g = {n: (np.zeros(tuple(P[n].shape)) if t is None else t.numpy()) for n, t in zip(names, grads[1:])}
    return logits.detach().numpy(), g, grads[0].numpy()


def run_pool(params: dict, tokens, dout):
    """(out, {name: grad}, dtokens) of Pool alone in float64; params keyed 'downsample.dw.kernel' ..."""
    P = {n: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(tokens, np.float64), requires_grad=True)
    out = pool(x, P)
    names = list(P)
    grads = torch.autograd.grad((out * torch.tensor(np.asarray(dout, np.float64))).sum(), [x] + [P[n] for n in names])
    return out.detach().numpy(), {n: t.numpy() for n, t in zip(names, grads[1:])}, grads[0].numpy()
