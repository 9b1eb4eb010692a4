"""Op-for-op float64 torch restatement of the reference's vit_for_small_dataset.ViT (vit_for_small_dataset.py:15-215) on parameters keyed by
the library's table names.  Pinned to the reference by tests/golden/ref_sd_*.npz (tests/test_small_dataset_oracle.py);
used by the GPU tier for the shapes no fixture covers.  Dropout is not modelled (rates 0 or training=False)."""
from __future__ import annotations

import math

import numpy as np
import torch

EPS = 1e-3   # Keras LayerNormalization default


def _ln(x, P, pre):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * P[pre + ".gamma"] + P[pre + ".beta"]


def _dense(x, P, pre, bias=True):
    y = x @ P[pre + ".kernel"]
    return y + P[pre + ".bias"] if bias else y


def shifted(img):
    """vit_for_small_dataset.py:15-47,154: [x, x shifted +1 / -1 along the width, +1 / -1 along the height] on the channel axis, zero fill."""
    z = torch.zeros_like(img)
    w1 = torch.cat([z[:, :, :1], img[:, :, :-1]], 2)
    w2 = torch.cat([img[:, :, 1:], z[:, :, :1]], 2)
    h1 = torch.cat([z[:, :1], img[:, :-1]], 1)
    h2 = torch.cat([img[:, 1:], z[:, :1]], 1)
    return torch.cat([img, w1, w2, h1, h2], -1)


def spt(img, P, p, pre="patch_embedding"):
    """SPT.call (vit_for_small_dataset.py:152-157): [b, H, W, C] -> [b, np, dim]."""
    x = shifted(img)
    b, H, W, C5 = x.shape
    x = x.reshape(b, H // p, p, W // p, p, C5).permute(0, 1, 3, 2, 4, 5).reshape(b, (H // p) * (W // p), p * p * C5)
    return _dense(_ln(x, P, pre + ".norm"), P, pre)


def lsa(x, P, pre, heads):
    """LSA.call (vit_for_small_dataset.py:104-121), x already normalised by PreNorm."""
    qkv = _dense(x, P, pre + ".to_qkv", bias=False)
    b, n, inner3 = qkv.shape
    dh = inner3 // 3 // heads
    q, k, v = (t.reshape(b, n, heads, dh).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1))
    dots = q @ k.transpose(-1, -2) * torch.exp(P[pre + ".temperature"])
    mask = torch.eye(n, dtype=torch.bool, device=x.device)
    dots = torch.where(mask, torch.full_like(dots, -float(np.finfo(np.float32).max)), dots)
    o = (torch.softmax(dots, -1) @ v).permute(0, 2, 1, 3).reshape(b, n, heads * dh)
    return _dense(o, P, pre + ".to_out") if (pre + ".to_out.kernel") in P else o


def forward(kw: dict, P: dict, img):
    """ViT.call(img) (vit_for_small_dataset.py:197-215) in float64; kw = the constructor kwargs."""
    ph = kw["patch_size"] if isinstance(kw["patch_size"], int) else kw["patch_size"][0]
    x = spt(img, P, ph)
    b = x.shape[0]
    x = torch.cat([P["cls_token"].expand(b, 1, x.shape[-1]), x], 1)
    x = x + P["pos_embedding"][:, :x.shape[1]]
    for l in range(kw["depth"]):
        p = f"transformer.{l}"
        x = lsa(_ln(x, P, p + ".attn.norm"), P, p + ".attn", kw["heads"]) + x
        h = _dense(_ln(x, P, p + ".mlp.norm"), P, p + ".mlp.fc1")
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = _dense(h, P, p + ".mlp.fc2") + x
    x = x.mean(1) if kw.get("pool", "cls") == "mean" else x[:, 0]
    return _dense(_ln(x, P, "mlp_head.norm"), P, "mlp_head")


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, device="cpu"):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in float64."""
    P = {n: torch.tensor(np.asarray(v, np.float64), device=device, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), device=device, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), device=device)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().cpu().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().cpu().numpy(), grads, g[0].detach().cpu().numpy()


def table_of(kw: dict):
    """[(name, shape, offset)] of the library's parameter table for these constructor kwargs (host only)."""
    from vit_tensorflow.vit_for_small_dataset import ViT
    return list(ViT(**kw)._table)


def init_params(table, seed: int = 1, dim_head: int = 64) -> dict:
    """Seeded weights for a table [(name, shape, offset)]: every tensor moved off its default (gamma around 1, beta around 0, each layer's
    temperature somewhere else near log(dim_head ** -0.5)) so that each gradient is exercised."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "gamma":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(shape[0])
        elif leaf in ("pos_embedding", "cls_token"):
            a = rng.standard_normal(shape)
        elif leaf == "temperature":
            a = math.log(dim_head ** -0.5) + 0.3 * rng.standard_normal(shape)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out
