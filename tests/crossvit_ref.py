"""Op-for-op float64 torch restatement of the reference's CrossViT (cross_vit.py:14-301) on parameters keyed by the library's table
names.  Pinned to the reference by tests/golden/ref_crossvit_*.npz (tests/test_crossvit_oracle.py); used by the GPU
tier for the shapes no fixture covers.  Dropout is not modelled (rates 0 or training=False)."""
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


def _attention(x, P, pre, heads, context=None, kv_include_self=False):
    """cross_vit.py:70-93 (x already normalised by PreNorm)."""
    context = x if context is None else context
    if kv_include_self:
        context = torch.cat([x, context], 1)
    q = _dense(x, P, pre + ".to_q", bias=False)
    kv = _dense(context, P, pre + ".to_kv", bias=False)
    k, v = kv.chunk(2, -1)
    b, n, inner = q.shape
    dh = inner // heads
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, dh).permute(0, 2, 1, 3)
    q, k, v = sp(q), sp(k), sp(v)
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(b, n, inner)
    return _dense(o, P, pre + ".to_out")


def _transformer(x, P, pre, depth, heads):
    """cross_vit.py:108-115: blocks, then the encoder's own final LayerNorm (also at depth 0)."""
    for j in range(depth):
        p = f"{pre}.{j}"
        x = _attention(_ln(x, P, p + ".attn.norm"), P, p + ".attn", heads) + x
        h = _dense(_ln(x, P, p + ".mlp.norm"), P, p + ".mlp.fc1")
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = _dense(h, P, p + ".mlp.fc2") + x
    return _ln(x, P, pre + ".norm")


def _project_attend(cls, context, P, pre, heads, proj):
    """ProjectInOut(PreNorm(Attention)) with kv_include_self (cross_vit.py:128-141, 158-159)."""
    x = _dense(cls, P, pre + ".project_in") if proj else cls
    x = _attention(_ln(x, P, pre + ".norm"), P, pre, heads, context=context, kv_include_self=True)
    return _dense(x, P, pre + ".project_out") if proj else x


def _embed(img, P, pre, p):
    b, H, W, C = img.shape
    x = img.reshape(b, H // p, p, W // p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(b, (H // p) * (W // p), p * p * C)
    x = _dense(x, P, pre + ".patch_embedding")
    cls = P[pre + ".cls_token"].expand(b, 1, x.shape[-1])
    x = torch.cat([cls, x], 1)
    return x + P[pre + ".pos_embedding"][:, :x.shape[1]]


def forward(kw: dict, P: dict, img):
    """CrossViT.call(img) in float64; kw = the constructor kwargs (reference defaults filled in)."""
    kw = {**DEFAULTS, **kw}
    sm = _embed(img, P, "sm_image_embedder", kw["sm_patch_size"])
    lg = _embed(img, P, "lg_image_embedder", kw["lg_patch_size"])
    proj = kw["sm_dim"] != kw["lg_dim"]
    for i in range(kw["depth"]):
        L = f"multi_scale_encoder.{i}"
        sm = _transformer(sm, P, L + ".sm_enc", kw["sm_enc_depth"], kw["sm_enc_heads"])
        lg = _transformer(lg, P, L + ".lg_enc", kw["lg_enc_depth"], kw["lg_enc_heads"])
        sm_cls, sm_patch, lg_cls, lg_patch = sm[:, :1], sm[:, 1:], lg[:, :1], lg[:, 1:]
        for k in range(kw["cross_attn_depth"]):
            c = f"{L}.cross.{k}"
            sm_cls = _project_attend(sm_cls, lg_patch, P, c + ".sm_attend_lg", kw["cross_attn_heads"], proj) + sm_cls
            lg_cls = _project_attend(lg_cls, sm_patch, P, c + ".lg_attend_sm", kw["cross_attn_heads"], proj) + lg_cls
        sm, lg = torch.cat([sm_cls, sm_patch], 1), torch.cat([lg_cls, lg_patch], 1)
    head = lambda t, pre: _dense(_ln(t[:, 0], P, pre + ".norm"), P, pre)
    return head(sm, "sm_mlp_head") + head(lg, "lg_mlp_head")


DEFAULTS = dict(sm_patch_size=12, sm_enc_depth=1, sm_enc_heads=8, sm_enc_mlp_dim=2048, sm_enc_dim_head=64, lg_patch_size=16, lg_enc_depth=4,
                lg_enc_heads=8, lg_enc_mlp_dim=2048, lg_enc_dim_head=64, cross_attn_depth=2, cross_attn_heads=8, cross_attn_dim_head=64, depth=3,
                dropout=0.1, emb_dropout=0.1)


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


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table [(name, shape, offset)]: every tensor random (LayerNorm gamma around 1) so that each gradient is exercised."""
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
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out
