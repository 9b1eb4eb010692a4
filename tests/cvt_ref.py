"""Op-for-op float64 torch restatement of the reference's CvT (cvt.py:30-202) on its deterministic path (dropout 0), on parameters keyed by the
library's table names.  Pinned to the reference by tests/golden/ref_cvt_*.npz (tests/test_cvt_oracle.py); used by the
GPU tier for the shapes no fixture covers.

Stated independently of the library's formulation: every 1x1 Conv2D is a matmul over the channel axis, the embedding and the depthwise
convolutions are torch's conv2d on a tensor padded explicitly by the 'SAME' rule, BatchNormalization is written out (batch mean and biased
variance under `training`, the moving statistics otherwise).  The parameter table is computed here from the constructor arguments, not read
from the library."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5        # cvt.py:31 (LayerNorm) and :85 (BatchNormalization)
DIM_HEAD = 64     # CvT never passes dim_head (cvt.py:130,189-191)

DEFAULTS = dict(s1_emb_dim=64, s1_emb_kernel=7, s1_emb_stride=4, s1_proj_kernel=3, s1_kv_proj_stride=2, s1_heads=1, s1_depth=1, s1_mlp_mult=4,
                s2_emb_dim=192, s2_emb_kernel=3, s2_emb_stride=2, s2_proj_kernel=3, s2_kv_proj_stride=2, s2_heads=3, s2_depth=2, s2_mlp_mult=4,
                s3_emb_dim=384, s3_emb_kernel=3, s3_emb_stride=2, s3_proj_kernel=3, s3_kv_proj_stride=2, s3_heads=6, s3_depth=10, s3_mlp_mult=4,
                dropout=0.0)
# the usage block of the reference (cvt.py:204-232): the defaults with s3_heads = 4
USAGE = dict(num_classes=1000, s3_heads=4)
STAGE_KEYS = ("emb_dim", "emb_kernel", "emb_stride", "proj_kernel", "kv_proj_stride", "heads", "depth", "mlp_mult")
BN_LEAVES = ("gamma", "beta", "moving_mean", "moving_variance")


def stages_of(kw: dict):
    """[(emb_dim, emb_kernel, emb_stride, proj_kernel, kv_proj_stride, heads, depth, mlp_mult)] for s1..s3 (cvt.py:184-192)."""
    c = {**DEFAULTS, **kw}
    return [tuple(c[f"s{i}_{k}"] for k in STAGE_KEYS) for i in (1, 2, 3)]


def same_pads(extent: int, k: int, s: int = 1):
    """(pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), the smaller half first."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return total // 2, total - total // 2


def maps_of(kw: dict, H: int, W: int):
    """[((H_s, W_s), (kv H_s, kv W_s))] of the three stages."""
    out = []
    for d, ek, es, pk, ks, heads, depth, mult in stages_of(kw):
        H, W = -(-H // es), -(-W // es)
        out.append(((H, W), (-(-H // ks), -(-W // ks))))
    return out


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in attribute order, shapes as the reference holds them."""
    c = {**DEFAULTS, **kw}
    t, cin = [], 3
    for s, (d, ek, es, pk, ks, heads, depth, mult) in enumerate(stages_of(kw)):
        pre = f"cvt_layers.{s}"
        inner = heads * DIM_HEAD
        t += [(pre + ".embed.kernel", (ek, ek, cin, d)), (pre + ".embed.bias", (d,)), (pre + ".norm.g", (1, 1, 1, d)), (pre + ".norm.b", (1, 1, 1, d))]
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            t += [(q + ".attn.norm.g", (1, 1, 1, d)), (q + ".attn.norm.b", (1, 1, 1, d))]
            for proj, width in (("to_q", inner), ("to_kv", 2 * inner)):
                t += [(f"{q}.attn.{proj}.dw.kernel", (pk, pk, 1, d))]
                t += [(f"{q}.attn.{proj}.bn.{leaf}", (d,)) for leaf in BN_LEAVES]
                t += [(f"{q}.attn.{proj}.pw.kernel", (1, 1, d, width))]
            t += [(q + ".attn.to_out.kernel", (1, 1, inner, d)), (q + ".attn.to_out.bias", (d,))]
            t += [(q + ".ff.norm.g", (1, 1, 1, d)), (q + ".ff.norm.b", (1, 1, 1, d)), (q + ".ff.fc1.kernel", (1, 1, d, d * mult)),
                  (q + ".ff.fc1.bias", (d * mult,)), (q + ".ff.fc2.kernel", (1, 1, d * mult, d)), (q + ".ff.fc2.bias", (d,))]
        cin = d
    t += [("head.kernel", (cin, c["num_classes"])), ("head.bias", (c["num_classes"],))]
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def is_moving(name: str) -> bool:
    return name.endswith(".moving_mean") or name.endswith(".moving_variance")


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table: every tensor moved off its default so that each gradient is exercised.  Kernels are scaled by their fan-in
    (a depthwise kernel's is its k * k taps); the moving variance is kept positive."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf in ("g", "gamma"):
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        elif leaf == "moving_variance":
            a = 0.5 + rng.random(shape)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def _ln(x, P, pre):
    """cvt.py:38-43 (reduce_variance is the biased variance)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * P[pre + ".g"].reshape(-1) + P[pre + ".b"].reshape(-1)


def _dense(x, P, pre, bias=True):
    k = P[pre + ".kernel"]
    y = x @ k.reshape(k.shape[-2], k.shape[-1])
    return y + P[pre + ".bias"] if bias else y


def conv_same(x, kernel, stride, bias=None, groups=1):
    """Conv2D(padding='SAME', strides=stride) of an NHWC tensor with an HWIO kernel."""
    k = kernel.shape[0]
    pt, pb = same_pads(x.shape[1], k, stride)
    pl, pr = same_pads(x.shape[2], k, stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, kernel.permute(3, 2, 0, 1), bias, stride=stride, groups=groups).permute(0, 2, 3, 1)


def batch_norm(x, P, pre, training):
    """BatchNormalization(momentum 0.9, epsilon 1e-5) over the channel axis (cvt.py:85)."""
    if training:
        mean = x.mean(dim=(0, 1, 2))
        var = ((x - mean) ** 2).mean(dim=(0, 1, 2))
    else:
        mean, var = P[pre + ".moving_mean"], P[pre + ".moving_variance"]
    return (x - mean) * torch.rsqrt(var + EPS) * P[pre + ".gamma"] + P[pre + ".beta"]


def dw_bn(x, P, pre, stride, training, conv_out=None):
    """The depthwise convolution and the BatchNormalization of a DepthWiseConv2d (cvt.py:84-85): the input of its pointwise projection.
    conv_out, a list, receives the convolution's output."""
    y = conv_same(x, P[pre + ".dw.kernel"], stride, groups=x.shape[-1])
    if conv_out is not None:
        conv_out.append(y)
    return batch_norm(y, P, pre + ".bn", training)


def attention(x, P, pre, heads, ks, training, taps=None, tap=None):
    """cvt.py:111-127."""
    b, H, W, _ = x.shape
    kv_conv = []
    q_in, kv_in = dw_bn(x, P, pre + ".to_q", 1, training), dw_bn(x, P, pre + ".to_kv", ks, training, kv_conv)
    if taps is not None:
        taps["q_in." + tap], taps["kv_in." + tap] = q_in, kv_in
        taps["kv_conv." + tap] = kv_conv[0]     # (not a tensor the library reads back: the BatchNormalization input, for the tests of its statistics)
    inner = heads * DIM_HEAD
    q = _dense(q_in, P, pre + ".to_q.pw", bias=False).reshape(b, H * W, inner)
    kv = _dense(kv_in, P, pre + ".to_kv.pw", bias=False).reshape(b, -1, 2 * inner)
    split = lambda t: t.reshape(b, t.shape[1], heads, DIM_HEAD).permute(0, 2, 1, 3)
    q, k, v = split(q), split(kv[..., :inner]), split(kv[..., inner:])
    a = torch.softmax(q @ k.transpose(-1, -2) * DIM_HEAD ** -0.5, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(b, H, W, inner)
    return _dense(o, P, pre + ".to_out")


def mlp(x, P, pre):
    """cvt.py:67-77."""
    y = _dense(x, P, pre + ".fc1")
    y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    return _dense(y, P, pre + ".fc2")


def forward(kw: dict, P: dict, img, training=True, taps: dict | None = None):
    """CvT.call(img, training) in the dtype of its inputs; kw = the constructor kwargs.  taps, when given, receives the tensors vitx_cvt_read names."""
    x = img
    for s, (d, ek, es, pk, ks, heads, depth, mult) in enumerate(stages_of(kw)):
        pre = f"cvt_layers.{s}"
        x = conv_same(x, P[pre + ".embed.kernel"], es, P[pre + ".embed.bias"])
        x = _ln(x, P, pre + ".norm")
        if taps is not None:
            taps[f"embedded.{s}"] = x
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            x = attention(_ln(x, P, q + ".attn.norm"), P, q + ".attn", heads, ks, training, taps, f"{s}.{l}") + x
            x = mlp(_ln(x, P, q + ".ff.norm"), P, q + ".ff") + x
        if taps is not None:
            taps[f"stage.{s}"] = x
    x = x.mean(dim=(1, 2))
    if taps is not None:
        taps["pooled"] = x
    return x @ P["head.kernel"] + P["head.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, dtype=torch.float64):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in `dtype`, training=True.  The moving statistics get zeros."""
    P = {n: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), dtype=dtype, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), dtype=dtype)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().numpy(), grads, g[0].detach().numpy()
