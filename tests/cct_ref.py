"""Op-for-op float64 torch restatement of the reference's CCT (cct.py:105-345) on its deterministic path (training falsy: no attention dropout,
no stochastic depth), on parameters keyed by the library's table names.  Pinned to the reference by
tests/golden/ref_cct_*.npz (tests/test_cct_oracle.py); used by the GPU tier for the shapes no fixture covers.

The convolution and the pooling are stated independently of the library's im2col formulation: torch's conv2d / max_pool2d on tensors padded
explicitly by the 'SAME' rule (zeros for the convolution, -inf for the pooling)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3   # Keras LayerNormalization default


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


def same_pads(extent: int, k: int, s: int):
    """(out, pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before = pad_total // 2."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return out, total // 2, total - total // 2


def conv_same(x, kernel, s):
    """Conv2D(padding='SAME', use_bias=False): x [b, H, W, Cin], kernel [k, k, Cin, Cout] (Keras HWIO)."""
    k = kernel.shape[0]
    _, pt, pb = same_pads(x.shape[1], k, s)
    _, pl, pr = same_pads(x.shape[2], k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, kernel.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)


def maxpool_same(x, k, s):
    """MaxPool2D(padding='SAME'): padding never wins."""
    _, pt, pb = same_pads(x.shape[1], k, s)
    _, pl, pr = same_pads(x.shape[2], k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=-float("inf"))
    return F.max_pool2d(xp, k, s).permute(0, 2, 3, 1)


def sequence_length(kw: dict) -> int:
    h, w = pair(kw.get("img_size", 224))
    for _ in range(kw.get("n_conv_layers", 1)):
        h = same_pads(same_pads(h, kw.get("kernel_size", 7), kw.get("stride", 2))[0], kw.get("pooling_kernel_size", 3), kw.get("pooling_stride", 2))[0]
        w = same_pads(same_pads(w, kw.get("kernel_size", 7), kw.get("stride", 2))[0], kw.get("pooling_kernel_size", 3), kw.get("pooling_stride", 2))[0]
    return h * w


def sine_table(n: int, dim: int) -> np.ndarray:
    """cct.py:269-275 as evidently meant (the reference itself raises there): [1, n, dim]."""
    pe = np.array([[p / (10000 ** (2 * (i // 2) / dim)) for i in range(dim)] for p in range(n)], np.float64)
    pe[:, 0::2] = np.sin(pe[:, 0::2])
    pe[:, 1::2] = np.cos(pe[:, 1::2])
    return pe.astype(np.float32).astype(np.float64)[None]


def _ln(x, P, pre):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * P[pre + ".gamma"] + P[pre + ".beta"]


def tokenizer(kw: dict, P: dict, img):
    """Tokenizer.call (cct.py:211-215): [b, H, W, C] -> [b, n, embedding_dim]."""
    x = img
    for i in range(kw.get("n_conv_layers", 1)):
        x = conv_same(x, P[f"tokenizer.conv_layers.{i}.kernel"], kw.get("stride", 2))
        x = maxpool_same(torch.relu(x), kw.get("pooling_kernel_size", 3), kw.get("pooling_stride", 2))
    return x.reshape(x.shape[0], -1, x.shape[-1])


def block(x, P, p, heads):
    """TransformerEncoderLayer.call (cct.py:159-174), deterministic."""
    y = _ln(x, P, p + ".pre_norm")
    qkv = y @ P[p + ".self_attn.to_qkv.kernel"]
    b, n, d3 = qkv.shape
    dh = d3 // 3 // heads
    q, k, v = (t.reshape(b, n, heads, dh).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1))
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(b, n, heads * dh)
    x = x + (o @ P[p + ".self_attn.proj.kernel"] + P[p + ".self_attn.proj.bias"])
    x = _ln(x, P, p + ".norm1")                                   # the normalised stream is the MLP input AND its residual
    h = x @ P[p + ".linear1.kernel"] + P[p + ".linear1.bias"]
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return x + (h @ P[p + ".linear2.kernel"] + P[p + ".linear2.bias"])


def seq_pool(x, P):
    """cct.py:293-299."""
    w = torch.softmax(x @ P["classifier.attention_pool.kernel"] + P["classifier.attention_pool.bias"], 1)
    return (w.transpose(1, 2) @ x).squeeze(1)


def forward(kw: dict, P: dict, img):
    """CCT.call(img, training=False) in float64; kw = the constructor kwargs."""
    x = tokenizer(kw, P, img)
    pe = kw.get("positional_embedding", "sine")
    if pe == "learnable":
        x = x + P["classifier.positional_emb"]
    elif pe != "none":
        x = x + torch.tensor(sine_table(x.shape[1], x.shape[2]), device=x.device)
    for l in range(kw.get("num_layers", 12)):
        x = block(x, P, f"classifier.blocks.{l}", kw.get("num_heads", 12))
    x = seq_pool(_ln(x, P, "classifier.norm"), P)
    return x @ P["classifier.fc.kernel"] + P["classifier.fc.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, device="cpu"):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in float64."""
    P = {n: torch.tensor(np.asarray(v, np.float64), device=device, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), device=device, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), device=device)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().cpu().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    dimg = g[0].detach().cpu().numpy() if g[0] is not None else np.zeros(np.shape(img))
    return logits.detach().cpu().numpy(), grads, dimg


def table_of(kw: dict):
    """[(name, shape, offset)] of the library's parameter table for these constructor kwargs (host only)."""
    from vit_tensorflow.cct import CCT
    return list(CCT(**kw)._table)


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table [(name, shape, offset)]: every tensor moved off its default so that each gradient is exercised.  Conv kernels
    are scaled by their fan-in, k * k * Cin."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "gamma":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        elif leaf == "positional_emb":
            a = 0.2 * rng.standard_normal(shape)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out
