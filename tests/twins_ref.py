"""Op-for-op float64 torch restatement of the reference's TwinsSVT (twins_svt.py:45-268) on its deterministic path (dropout 0), on parameters
keyed by the library's table names.  Pinned to the reference by tests/golden/ref_twins_*.npz
(tests/test_twins_oracle.py); used by the GPU tier for the shapes no fixture covers.

Stated independently of the library's formulation: every 1x1 Conv2D is a matmul over the channel axis, the strided to_kv convolution and the
depthwise PEG convolution are torch's conv2d (the latter on a tensor padded explicitly by the 'SAME' rule), the window partition is plain
reshape / permute.  The parameter table is computed here from the constructor arguments, not read from the library."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5           # twins_svt.py:46
HEADS, DIM_HEAD = 8, 64   # TwinsSVT never passes heads / dim_head (twins_svt.py:118,159,193)
INNER = HEADS * DIM_HEAD
MULT = 4             # twins_svt.py:79

DEFAULTS = dict(s1_emb_dim=64, s1_patch_size=4, s1_local_patch_size=7, s1_global_k=7, s1_depth=1,
                s2_emb_dim=128, s2_patch_size=2, s2_local_patch_size=7, s2_global_k=7, s2_depth=1,
                s3_emb_dim=256, s3_patch_size=2, s3_local_patch_size=7, s3_global_k=7, s3_depth=5,
                s4_emb_dim=512, s4_patch_size=2, s4_local_patch_size=7, s4_global_k=7, s4_depth=4,
                peg_kernel_size=3, dropout=0.0)


def stages_of(kw: dict):
    """[(emb_dim, patch_size, local_patch_size, global_k, depth, has_local)] for s1..s4 (twins_svt.py:246-259)."""
    c = {**DEFAULTS, **kw}
    return [(c[f"s{i}_emb_dim"], c[f"s{i}_patch_size"], c[f"s{i}_local_patch_size"], c[f"s{i}_global_k"], c[f"s{i}_depth"], i != 4)
            for i in (1, 2, 3, 4)]


def same_pads(extent: int, k: int, s: int = 1):
    """(pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), the smaller half first."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return total // 2, total - total // 2


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in attribute order, shapes as the reference holds them."""
    c = {**DEFAULTS, **kw}
    kp = c["peg_kernel_size"]
    t, cin = [], 3
    for s, (d, p, lp, gk, depth, has_local) in enumerate(stages_of(kw)):
        pre = f"svt_layers.{s}"
        t += [(pre + ".patch_embedding.proj.kernel", (1, 1, cin * p * p, d)), (pre + ".patch_embedding.proj.bias", (d,))]

        def transformer(ti, n):
            out = []
            for l in range(n):
                q = f"{pre}.transformer.{ti}.{l}"
                ff = lambda f: [(f"{q}.{f}.norm.g", (1, 1, 1, d)), (f"{q}.{f}.norm.b", (1, 1, 1, d)), (f"{q}.{f}.fc1.kernel", (1, 1, d, d * MULT)),
                                (f"{q}.{f}.fc1.bias", (d * MULT,)), (f"{q}.{f}.fc2.kernel", (1, 1, d * MULT, d)), (f"{q}.{f}.fc2.bias", (d,))]
                attn = lambda a, kk: [(f"{q}.{a}.norm.g", (1, 1, 1, d)), (f"{q}.{a}.norm.b", (1, 1, 1, d)), (f"{q}.{a}.to_q.kernel", (1, 1, d, INNER)),
                                      (f"{q}.{a}.to_kv.kernel", (kk, kk, d, 2 * INNER)), (f"{q}.{a}.to_out.kernel", (1, 1, INNER, d)),
                                      (f"{q}.{a}.to_out.bias", (d,))]
                if has_local:
                    out += attn("local_attn", 1) + ff("ff1")
                out += attn("global_attn", gk) + ff("ff2")
            return out
        t += transformer(0, 1)
        t += [(pre + ".peg.kernel", (kp, kp, 1, d)), (pre + ".peg.bias", (d,))]
        t += transformer(1, depth)
        cin = d
    t += [("head.kernel", (cin, c["num_classes"])), ("head.bias", (c["num_classes"],))]
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table: every tensor moved off its default so that each gradient is exercised.  Kernels are scaled by their fan-in."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "g":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def _ln(x, P, pre):
    """twins_svt.py:53-58 (reduce_variance is the biased variance)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * P[pre + ".g"].reshape(-1) + P[pre + ".b"].reshape(-1)


def _dense(x, P, pre, bias=True):
    k = P[pre + ".kernel"]
    y = x @ k.reshape(k.shape[-2], k.shape[-1])
    return y + P[pre + ".bias"] if bias else y


def _heads(t):
    """'b n (h d) -> b h n d'."""
    b, n, _ = t.shape
    return t.reshape(b, n, HEADS, DIM_HEAD).permute(0, 2, 1, 3)


def _attend(q, k, v):
    a = torch.softmax(q @ k.transpose(-1, -2) * DIM_HEAD ** -0.5, -1)
    o = a @ v
    b, h, n, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(b, n, h * d)


def to_windows(x, p):
    """'b (x p1) (y p2) c -> (b x y) p1 p2 c' (twins_svt.py:141)."""
    b, H, W, c = x.shape
    return x.reshape(b, H // p, p, W // p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b * (H // p) * (W // p), p, p, c)


def from_windows(x, b, H, W):
    """'(b x y) p1 p2 c -> b (x p1) (y p2) c' (twins_svt.py:153)."""
    _, p, _, c = x.shape
    return x.reshape(b, H // p, W // p, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b, H, W, c)


def local_attention(x, P, pre, p):
    """twins_svt.py:135-156."""
    b, H, W, c = x.shape
    w = to_windows(x, p).reshape(-1, p * p, c)
    q = _heads(_dense(w, P, pre + ".to_q", bias=False))
    kv = _dense(w, P, pre + ".to_kv", bias=False)
    k, v = _heads(kv[..., :INNER]), _heads(kv[..., INNER:])
    o = _attend(q, k, v).reshape(-1, p, p, INNER)
    return _dense(from_windows(o, b, H, W), P, pre + ".to_out")


def global_attention(x, P, pre, gk):
    """twins_svt.py:175-190; to_kv is a 'valid' convolution of kernel and stride k."""
    b, H, W, c = x.shape
    q = _heads(_dense(x.reshape(b, H * W, c), P, pre + ".to_q", bias=False))
    kv = F.conv2d(x.permute(0, 3, 1, 2), P[pre + ".to_kv.kernel"].permute(3, 2, 0, 1), None, stride=gk).permute(0, 2, 3, 1)
    kv = kv.reshape(b, -1, 2 * INNER)
    k, v = _heads(kv[..., :INNER]), _heads(kv[..., INNER:])
    o = _attend(q, k, v).reshape(b, H, W, INNER)
    return _dense(o, P, pre + ".to_out")


def mlp(x, P, pre):
    """twins_svt.py:82-92."""
    y = _dense(x, P, pre + ".fc1")
    y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    return _dense(y, P, pre + ".fc2")


def transformer(x, P, pre, depth, lp, gk, has_local):
    """twins_svt.py:206-213."""
    for l in range(depth):
        q = f"{pre}.{l}"
        if has_local:
            x = local_attention(_ln(x, P, q + ".local_attn.norm"), P, q + ".local_attn", lp) + x
            x = mlp(_ln(x, P, q + ".ff1.norm"), P, q + ".ff1") + x
        x = global_attention(_ln(x, P, q + ".global_attn.norm"), P, q + ".global_attn", gk) + x
        x = mlp(_ln(x, P, q + ".ff2.norm"), P, q + ".ff2") + x
    return x


def peg(x, P, pre):
    """twins_svt.py:108-115: x + depthwise Conv2D(kernel [kp, kp, 1, d], 'SAME', stride 1) with bias."""
    k = P[pre + ".kernel"]
    kp, d = k.shape[0], k.shape[-1]
    pt, pb = same_pads(x.shape[1], kp)
    pl, pr = same_pads(x.shape[2], kp)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, k.permute(3, 2, 0, 1), P[pre + ".bias"], groups=d).permute(0, 2, 3, 1)
    return y + x


def patch_embedding(x, P, pre, p):
    """twins_svt.py:101-106: 'b (h p1) (w p2) c -> b h w (c p1 p2)' then a 1x1 convolution."""
    b, H, W, c = x.shape
    x = x.reshape(b, H // p, p, W // p, p, c).permute(0, 1, 3, 5, 2, 4).reshape(b, H // p, W // p, c * p * p)
    return _dense(x, P, pre + ".proj")


def forward(kw: dict, P: dict, img, taps: dict | None = None):
    """TwinsSVT.call(img) in the dtype of its inputs; kw = the constructor kwargs.  taps, when given, receives the tensors vitx_twins_read names."""
    x = img
    for s, (d, p, lp, gk, depth, has_local) in enumerate(stages_of(kw)):
        pre = f"svt_layers.{s}"
        x = patch_embedding(x, P, pre + ".patch_embedding", p)
        if taps is not None:
            taps[f"embedded.{s}"] = x
        x = transformer(x, P, pre + ".transformer.0", 1, lp, gk, has_local)
        if taps is not None:
            taps[f"pre_peg.{s}"] = x
        x = peg(x, P, pre + ".peg")
        if taps is not None:
            taps[f"peg.{s}"] = x
        x = transformer(x, P, pre + ".transformer.1", depth, lp, gk, has_local)
        if taps is not None:
            taps[f"stage.{s}"] = x
    x = x.mean(dim=(1, 2))
    if taps is not None:
        taps["pooled"] = x
    return x @ P["head.kernel"] + P["head.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, dtype=torch.float64):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in `dtype`."""
    P = {n: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), dtype=dtype, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), dtype=dtype)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().numpy(), grads, g[0].detach().numpy()
