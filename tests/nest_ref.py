"""Op-for-op float64 torch restatement of the reference's NesT (nest.py:28-216) on its deterministic path (dropout 0), on parameters keyed by
the library's table names.  Pinned to the reference by tests/golden/ref_nest_*.npz (tests/test_nest_oracle.py); used by
the GPU tier for the shapes no fixture covers.

Stated independently of the library's formulation: every 1x1 Conv2D is a matmul over the channel axis, the aggregation convolution and the
pooling are torch's conv2d / max_pool2d on tensors padded explicitly by the 'SAME' rule (zeros for the convolution, -inf for the pooling), and
the block partition is plain reshape / permute.  The parameter table is computed here from the constructor arguments, not read from the library."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5   # nest.py:29


def cast_tuple(val, depth):
    return val if isinstance(val, tuple) else ((val,) * depth)


def same_pads(extent: int, k: int, s: int):
    """(out, pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before = pad_total // 2."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return out, total // 2, total - total // 2


def conv_same(x, kernel, bias, s=1):
    """Conv2D(padding='SAME'): x [b, H, W, Cin], kernel [k, k, Cin, Cout] (Keras HWIO), bias [Cout]."""
    k = kernel.shape[0]
    _, pt, pb = same_pads(x.shape[1], k, s)
    _, pl, pr = same_pads(x.shape[2], k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, kernel.permute(3, 2, 0, 1), bias, stride=s).permute(0, 2, 3, 1)


def maxpool_same(x, k=3, s=2):
    """MaxPool2D(padding='SAME') on a signed input: padding never wins."""
    _, pt, pb = same_pads(x.shape[1], k, s)
    _, pl, pr = same_pads(x.shape[2], k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=-float("inf"))
    return F.max_pool2d(xp, k, s).permute(0, 2, 3, 1)


def levels_of(kw: dict):
    """[(dim, heads, dim_head, inner, depth, blocks)] per entry of nest_layers (nest.py:165-194), finest level first, and seq_len."""
    H = kw["num_hierarchies"]
    fmap = kw["image_size"] // kw["patch_size"]
    seq_len = (fmap // 2 ** (H - 1)) ** 2
    reps = cast_tuple(kw["block_repeats"], H)
    out = []
    for i in range(H):
        d, h = kw["dim"] * 2 ** i, kw["heads"] * 2 ** i
        dh = d // h
        out.append((d, h, dh, dh * h, reps[i], 2 ** (H - 1 - i)))
    return out, seq_len


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in the documented order, shapes as the reference holds them."""
    lv, seq_len = levels_of(kw)
    p, dim, mult = kw["patch_size"], kw["dim"], kw.get("mlp_mult", 4)
    t = [("patch_embedding.kernel", (1, 1, p * p * 3, dim)), ("patch_embedding.bias", (dim,))]
    for i, (d, h, dh, inner, depth, _) in enumerate(lv):
        pre = f"nest_layers.{i}"
        t.append((pre + ".transformer.pos_emb", (seq_len,)))
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            t += [(q + ".attn.norm.g", (1, 1, 1, d)), (q + ".attn.norm.b", (1, 1, 1, d)), (q + ".attn.to_qkv.kernel", (1, 1, d, 3 * inner)),
                  (q + ".attn.to_out.kernel", (1, 1, inner, d)), (q + ".attn.to_out.bias", (d,)),
                  (q + ".ff.norm.g", (1, 1, 1, d)), (q + ".ff.norm.b", (1, 1, 1, d)), (q + ".ff.fc1.kernel", (1, 1, d, d * mult)),
                  (q + ".ff.fc1.bias", (d * mult,)), (q + ".ff.fc2.kernel", (1, 1, d * mult, d)), (q + ".ff.fc2.bias", (d,))]
        if i < len(lv) - 1:
            dn = lv[i + 1][0]
            t += [(pre + ".aggregate.conv.kernel", (3, 3, d, dn)), (pre + ".aggregate.conv.bias", (dn,)),
                  (pre + ".aggregate.norm.g", (1, 1, 1, dn)), (pre + ".aggregate.norm.b", (1, 1, 1, dn))]
    dl = lv[-1][0]
    t += [("mlp_head.norm.g", (1, 1, 1, dl)), ("mlp_head.norm.b", (1, 1, 1, dl)), ("mlp_head.kernel", (dl, kw["num_classes"])),
          ("mlp_head.bias", (kw["num_classes"],))]
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def last_pos_emb(kw: dict) -> str:
    """The last level's pos_emb: one scalar per position ahead of channel LayerNorms only, so its true gradient is zero."""
    return f"nest_layers.{kw['num_hierarchies'] - 1}.transformer.pos_emb"


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table [(name, shape, offset)]: every tensor moved off its default so that each gradient is exercised.  Kernels are
    scaled by their fan-in."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "g":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        elif leaf == "pos_emb":
            a = rng.standard_normal(shape)            # tf.random.normal (nest.py:129)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def _ln(x, P, pre):
    """nest.py:36-41 (reduce_variance is the biased variance)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * P[pre + ".g"].reshape(-1) + P[pre + ".b"].reshape(-1)


def _dense(x, P, pre, bias=True):
    k = P[pre + ".kernel"]
    y = x @ k.reshape(k.shape[-2], k.shape[-1])
    return y + P[pre + ".bias"] if bias else y


def attention(x, P, pre, heads):
    """nest.py:93-109 on [B, h, w, c]."""
    B, h, w, c = x.shape
    qkv = _dense(x, P, pre + ".to_qkv", bias=False).reshape(B, h * w, 3, heads, -1)
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    dh = q.shape[-1]
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(B, h, w, heads * dh)
    return _dense(o, P, pre + ".to_out")


def transformer(x, P, pre, depth, heads):
    """nest.py:137-148."""
    _, h, w, _ = x.shape
    x = x + P[pre + ".pos_emb"][:h * w].reshape(1, h, w, 1)
    for l in range(depth):
        q = f"{pre}.{l}"
        x = attention(_ln(x, P, q + ".attn.norm"), P, q + ".attn", heads) + x
        y = _dense(_ln(x, P, q + ".ff.norm"), P, q + ".ff.fc1")
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
        x = _dense(y, P, q + ".ff.fc2") + x
    return x


def to_blocks(x, nb):
    """'b (b1 h) (b2 w) c -> (b b1 b2) h w c' (nest.py:209)."""
    b, H, W, c = x.shape
    h, w = H // nb, W // nb
    return x.reshape(b, nb, h, nb, w, c).permute(0, 1, 3, 2, 4, 5).reshape(b * nb * nb, h, w, c)


def from_blocks(x, nb):
    """'(b b1 b2) h w c -> b (b1 h) (b2 w) c' (nest.py:211)."""
    B, h, w, c = x.shape
    b = B // (nb * nb)
    return x.reshape(b, nb, nb, h, w, c).permute(0, 1, 3, 2, 4, 5).reshape(b, nb * h, nb * w, c)


def forward(kw: dict, P: dict, img, taps: dict | None = None):
    """NesT.call(img) in the dtype of its inputs; kw = the constructor kwargs.  taps, when given, receives the tensors vitx_nest_read names."""
    lv, _ = levels_of(kw)
    p = kw["patch_size"]
    b, H, W, c = img.shape
    x = img.reshape(b, H // p, p, W // p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b, H // p, W // p, p * p * c)   # nest.py:179
    x = _dense(x, P, "patch_embedding")
    if taps is not None:
        taps["embedded"] = x
    for i, (d, heads, dh, inner, depth, nb) in enumerate(lv):
        pre = f"nest_layers.{i}"
        x = from_blocks(transformer(to_blocks(x, nb), P, pre + ".transformer", depth, heads), nb)
        if taps is not None:
            taps[f"level.{i}"] = x
        if i < len(lv) - 1:
            x = conv_same(x, P[pre + ".aggregate.conv.kernel"], P[pre + ".aggregate.conv.bias"])
            x = maxpool_same(_ln(x, P, pre + ".aggregate.norm"))
            if taps is not None:
                taps[f"aggregated.{i}"] = x
    x = _ln(x, P, "mlp_head.norm").mean(dim=(1, 2))
    if taps is not None:
        taps["pooled"] = x
    return x @ P["mlp_head.kernel"] + P["mlp_head.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, dtype=torch.float64):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in `dtype` (float64: the reference; float32: an honest fp32 evaluation)."""
    P = {n: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), dtype=dtype, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), dtype=dtype)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().numpy(), grads, g[0].detach().numpy()
