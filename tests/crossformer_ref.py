"""Op-for-op float64 torch restatement of the reference's CrossFormer (crossformer.py:30-257) on its deterministic path (ff_dropout 0), on
parameters keyed by the library's table names.  Pinned to the reference by tests/golden/ref_cf_*.npz
(tests/test_crossformer_oracle.py); used by the GPU tier for the batches and image sizes no fixture covers.

Stated independently of the library's formulation: the cross-embed convolutions are torch's conv2d on a tensor padded explicitly by the
'SAME' rule, every 1x1 Conv2D is a matmul over the channel axis, both window partitions are plain reshape / permute, and the position bias
is built with numpy index arithmetic.  The parameter table is computed here from the constructor arguments, not read from the library.

Two behaviours of the reference are reproduced on purpose: the dynamic position bias is cut from the autograd graph (crossformer.py:163
goes through `.numpy()`), so the `dpb.*` parameters have a gradient of exactly zero; and the bias indices have row stride 2 wsz - 1 (:131)
into a table of (2 wsz + 1)^2 rows built from positions -wsz .. wsz (:159-161)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5            # crossformer.py:75
DPB_EPS = 1e-3        # Keras LayerNormalization's default epsilon (:57)
DIM_HEAD = 32         # CrossFormer never passes dim_head (:105,183,240)
MULT = 4              # :90

DEFAULTS = dict(dim=(64, 128, 256, 512), depth=(2, 2, 8, 2), global_window_size=(8, 4, 2, 1), local_window_size=7,
                cross_embed_kernel_sizes=((4, 8, 16, 32), (2, 4), (2, 4), (2, 4)), cross_embed_strides=(4, 2, 2, 2), num_classes=1000)


def _cast(v):
    return v if isinstance(v, tuple) else (v,) * 4


def stages_of(kw: dict):
    """[(dim, depth, global_wsz, local_wsz, sorted kernel sizes, widths, stride)] for the four stages (crossformer.py:34-39,235-242)."""
    c = {**DEFAULTS, **kw}
    out = []
    for d, n, g, lw, ks, st in zip(*(_cast(c[k]) for k in ("dim", "depth", "global_window_size", "local_window_size", "cross_embed_kernel_sizes",
                                                           "cross_embed_strides"))):
        ks = sorted(ks)
        widths = [int(d / (2 ** i)) for i in range(1, len(ks))]
        widths = [*widths, d - sum(widths)]
        out.append((d, n, g, lw, ks, widths, st))
    return out


def same_pads(extent: int, k: int, s: int = 1):
    """(pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), the smaller half first."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return total // 2, total - total // 2


def maps_of(kw: dict, H: int, W: int):
    out = []
    for *_, st in stages_of(kw):
        H, W = -(-H // st), -(-W // st)
        out.append((H, W))
    return out


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in attribute order, shapes as the reference holds them."""
    c = {**DEFAULTS, **kw}
    t, cin = [], 3
    for s, (d, depth, g, lw, ks, widths, st) in enumerate(stages_of(kw)):
        pre = f"crossformer_layers.{s}"
        inner, d4 = (d // DIM_HEAD) * DIM_HEAD, d // 4
        for i, (k, w) in enumerate(zip(ks, widths)):
            t += [(f"{pre}.cel.convs.{i}.kernel", (k, k, cin, w)), (f"{pre}.cel.convs.{i}.bias", (w,))]

        def attn(q):
            out = [(q + ".norm.g", (1, 1, 1, d)), (q + ".norm.b", (1, 1, 1, d)), (q + ".to_qkv.kernel", (1, 1, d, 3 * inner)),
                   (q + ".to_out.kernel", (1, 1, inner, d)), (q + ".to_out.bias", (d,))]
            for i in range(3):
                out += [(f"{q}.dpb.dense.{i}.kernel", (d4 if i else 2, d4)), (f"{q}.dpb.dense.{i}.bias", (d4,)),
                        (f"{q}.dpb.norm.{i}.gamma", (d4,)), (f"{q}.dpb.norm.{i}.beta", (d4,))]
            return out + [(q + ".dpb.dense.3.kernel", (d4, 1)), (q + ".dpb.dense.3.bias", (1,))]

        def ff(q):
            return [(q + ".norm.g", (1, 1, 1, d)), (q + ".norm.b", (1, 1, 1, d)), (q + ".fc1.kernel", (1, 1, d, d * MULT)),
                    (q + ".fc1.bias", (d * MULT,)), (q + ".fc2.kernel", (1, 1, d * MULT, d)), (q + ".fc2.bias", (d,))]
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            t += attn(q + ".short_attn") + ff(q + ".short_ff") + attn(q + ".long_attn") + ff(q + ".long_ff")
        cin = d
    t += [("to_logits.kernel", (cin, c["num_classes"])), ("to_logits.bias", (c["num_classes"],))]
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def is_dpb(name: str) -> bool:
    return ".dpb." in name


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table: every tensor moved off its default so that each gradient is exercised.  Kernels are scaled by their fan-in;
    the last Dense of a position-bias network is scaled up so that the bias is of the order of the scores (a bias the logits do not feel
    would pin nothing)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf in ("g", "gamma"):
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
            if name.endswith(".dpb.dense.3.kernel"):
                a = 2.0 * a
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def _ln(x, P, pre):
    """crossformer.py:82-87 (reduce_variance is the biased variance)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * P[pre + ".g"].reshape(-1) + P[pre + ".b"].reshape(-1)


def _dense(x, P, pre, bias=True):
    k = P[pre + ".kernel"]
    y = x @ k.reshape(k.shape[-2], k.shape[-1])
    return y + P[pre + ".bias"] if bias else y


def rel_pos_indices(wsz: int) -> np.ndarray:
    """crossformer.py:126-131: [n, n] indices, row stride 2 wsz - 1."""
    pos = np.arange(wsz)
    grid = np.stack(np.meshgrid(pos, pos, indexing="ij")).reshape(2, -1).T     # 'c i j -> (i j) c'
    rel = grid[:, None] - grid[None, :] + wsz - 1
    return (rel * np.array([2 * wsz - 1, 1])).sum(-1)


def position_bias(P, pre, wsz: int):
    """crossformer.py:159-163: the bias network on the (2 wsz + 1)^2 positions -wsz .. wsz, gathered to [n, n]; detached, as `.numpy()` does."""
    pos = np.arange(-wsz, wsz + 1)
    rel = np.stack(np.meshgrid(pos, pos, indexing="ij")).reshape(2, -1).T
    x = torch.tensor(rel.astype(np.float64), dtype=P[pre + ".dense.0.kernel"].dtype)
    for i in range(3):
        x = x @ P[f"{pre}.dense.{i}.kernel"] + P[f"{pre}.dense.{i}.bias"]
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        x = torch.relu((x - mean) * torch.rsqrt(var + DPB_EPS) * P[f"{pre}.norm.{i}.gamma"] + P[f"{pre}.norm.{i}.beta"])
    x = (x @ P[pre + ".dense.3.kernel"] + P[pre + ".dense.3.bias"]).squeeze(-1)
    return x.detach()[torch.as_tensor(rel_pos_indices(wsz))]


def to_short(x, w):
    """'b (h s1) (w s2) d -> (b h w) s1 s2 d' (crossformer.py:144)."""
    b, H, W, c = x.shape
    return x.reshape(b, H // w, w, W // w, w, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, w, w, c)


def from_short(x, b, H, W):
    """'(b h w) s1 s2 d -> b (h s1) (w s2) d' (:176)."""
    _, w, _, c = x.shape
    return x.reshape(b, H // w, W // w, w, w, c).permute(0, 1, 3, 2, 4, 5).reshape(b, H, W, c)


def to_long(x, w):
    """'b (l1 h) (l2 w) d -> (b h w) l1 l2 d' (:146)."""
    b, H, W, c = x.shape
    return x.reshape(b, w, H // w, w, W // w, c).permute(0, 2, 4, 1, 3, 5).reshape(-1, w, w, c)


def from_long(x, b, H, W):
    """'(b h w) l1 l2 d -> b (l1 h) (l2 w) d' (:178)."""
    _, w, _, c = x.shape
    return x.reshape(b, H // w, W // w, w, w, c).permute(0, 3, 1, 4, 2, 5).reshape(b, H, W, c)


def attention(x, P, pre, kind, wsz, taps=None):
    """crossformer.py:133-180."""
    b, H, W, d = x.shape
    heads = d // DIM_HEAD
    x = _ln(x, P, pre + ".norm")
    x = (to_short if kind == "short" else to_long)(x, wsz)
    qkv = _dense(x.reshape(-1, wsz * wsz, d), P, pre + ".to_qkv", bias=False)
    q, k, v = (t.reshape(t.shape[0], wsz * wsz, heads, DIM_HEAD).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    bias = position_bias(P, pre + ".dpb", wsz)
    if taps is not None:
        taps["bias." + pre] = bias
    sim = (q * DIM_HEAD ** -0.5) @ k.transpose(-1, -2) + bias
    o = torch.softmax(sim, -1) @ v
    o = o.permute(0, 2, 1, 3).reshape(-1, wsz, wsz, heads * DIM_HEAD)
    o = _dense(o, P, pre + ".to_out")
    return (from_short if kind == "short" else from_long)(o, b, H, W)


def mlp(x, P, pre):
    """crossformer.py:93-102."""
    y = _dense(_ln(x, P, pre + ".norm"), P, pre + ".fc1")
    y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    return _dense(y, P, pre + ".fc2")


def cross_embed(x, P, pre, ks, st):
    """crossformer.py:45-48: Conv2D(width_i, k_i, strides, 'SAME') per sorted kernel size, concatenated over channels."""
    xp = x.permute(0, 3, 1, 2)
    maps = []
    for i, k in enumerate(ks):
        pt, pb = same_pads(x.shape[1], k, st)
        pl, pr = same_pads(x.shape[2], k, st)
        y = F.conv2d(F.pad(xp, (pl, pr, pt, pb)), P[f"{pre}.convs.{i}.kernel"].permute(3, 2, 0, 1), P[f"{pre}.convs.{i}.bias"], stride=st)
        maps.append(y.permute(0, 2, 3, 1))
    return torch.cat(maps, dim=-1)


def forward(kw: dict, P: dict, img, taps: dict | None = None):
    """CrossFormer.call(img) in the dtype of its inputs; kw = the constructor kwargs.  taps, when given, receives the tensors
    vitx_crossformer_read names ('bias.<table prefix of the attention>' for the biases)."""
    x = img
    for s, (d, depth, g, lw, ks, widths, st) in enumerate(stages_of(kw)):
        pre = f"crossformer_layers.{s}"
        x = cross_embed(x, P, pre + ".cel", ks, st)
        if taps is not None:
            taps[f"embedded.{s}"] = x
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            x = attention(x, P, q + ".short_attn", "short", lw, taps) + x
            x = mlp(x, P, q + ".short_ff") + x
            x = attention(x, P, q + ".long_attn", "long", g, taps) + x
            x = mlp(x, P, q + ".long_ff") + x
        if taps is not None:
            taps[f"stage.{s}"] = x
    x = x.mean(dim=(1, 2))
    if taps is not None:
        taps["pooled"] = x
    return x @ P["to_logits.kernel"] + P["to_logits.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, dtype=torch.float64):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in `dtype`; a parameter the graph does not reach (dpb.*) gets zeros."""
    P = {n: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), dtype=dtype, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), dtype=dtype)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().numpy(), grads, g[0].detach().numpy()
