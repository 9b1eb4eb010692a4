"""Op-for-op float64 torch restatement of the reference's RegionViT (regionvit.py:45-263) on its deterministic path (ff_dropout 0), on
parameters keyed by the library's table names.  Pinned to the reference by tests/golden/ref_rv_*.npz
(tests/test_regionvit_oracle.py); used by the GPU tier for the batches and image sizes no fixture covers.

Stated independently of the library's formulation: every convolution is torch's conv2d on a tensor padded explicitly by the 'SAME' rule, the
window partition with the region token in front is reshape / permute / cat, and the relative position bias is built here with numpy index
arithmetic from the embedding table ([(2 ws - 1)^2, heads], one per stage, shared by the stage's layers) and padded with a zero row and column
for the region token.  The parameter table is computed here from the constructor arguments, not read from the library.

Behaviours of the reference reproduced on purpose: the same Attention weights run on the region sequence and on the window sequences of a
layer; the same Downsample convolution runs on the local and on the region map; the window is (lh // rh, lw // rw) of the maps, not
window_size; the local tokens of the last layer never reach the logits; a stage without layers never looks its embedding up."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-3         # Keras LayerNormalization's default epsilon (regionvit.py:69,87,213,245)
DIM_HEAD = 32         # :80
HEADS = 4             # :80
MULT = 4              # :65
EMB_SCALE = 2.0       # scale of the seeded relative-position embeddings (1.0 moved the 197-token case by 5.9e-3 of its spread only)

DEFAULTS = dict(dim=(64, 128, 256, 512), depth=(2, 2, 8, 2), window_size=7, num_classes=1000, tokenize_local_3_conv=False, local_patch_size=4,
                use_peg=False)


def _cast(v):
    return v if isinstance(v, tuple) else (v,) * 4


def config_of(kw: dict) -> dict:
    c = {**DEFAULTS, **{k: v for k, v in kw.items() if k in DEFAULTS}}
    c["dim"], c["depth"] = _cast(c["dim"]), _cast(c["depth"])
    if len(c["dim"]) != 4 or len(c["depth"]) != 4:
        raise ValueError("dim and depth need to be a single value or a tuple of length 4")
    return c


def same_pads(extent: int, k: int, s: int = 1):
    """(pad_before, pad_after) of TF 'SAME': out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), the smaller half first."""
    out = -(-extent // s)
    total = max((out - 1) * s + k - extent, 0)
    return total // 2, total - total // 2


def maps_of(kw: dict, H: int, W: int):
    """[((lh, lw), (rh, rw), (wh, ww))] of the four stages; ValueError where the reference's asserts or rearranges fail."""
    c = config_of(kw)
    p = c["local_patch_size"] * c["window_size"]
    if H % p or W % p:
        raise ValueError("height and width must be divisible by region patch size")
    lh, lw, rh, rw = -(-H // 4), -(-W // 4), H // p, W // p     # the local encoder is stride 4 whatever local_patch_size says (:212-221)
    out = []
    for s in range(4):
        if s:
            lh, lw, rh, rw = -(-lh // 2), -(-lw // 2), -(-rh // 2), -(-rw // 2)
        wh, ww = lh // rh, lw // rw
        if lh % rh or lw % rw or wh == 0 or ww == 0 or lh // wh != rh or lw // ww != rw:
            raise ValueError(f"stage {s}: the region map ({rh} x {rw}) does not cut the local map ({lh} x {lw}) into windows")
        out.append(((lh, lw), (rh, rw), (wh, ww)))
    return out


def table_of(kw: dict):
    """[(name, shape, offset)]: the reference's variables in attribute order, shapes as the reference holds them."""
    c = config_of(kw)
    dims, depths, ws = c["dim"], c["depth"], c["window_size"]
    d0, inner = dims[0], HEADS * DIM_HEAD
    t = []
    if c["tokenize_local_3_conv"]:
        t += [("local_encoder.0.kernel", (3, 3, 3, d0)), ("local_encoder.0.bias", (d0,)), ("local_encoder.1.gamma", (d0,)), ("local_encoder.1.beta", (d0,)),
              ("local_encoder.3.kernel", (3, 3, d0, d0)), ("local_encoder.3.bias", (d0,)), ("local_encoder.4.gamma", (d0,)), ("local_encoder.4.beta", (d0,)),
              ("local_encoder.6.kernel", (3, 3, d0, d0)), ("local_encoder.6.bias", (d0,))]
    else:
        t += [("local_encoder.kernel", (8, 8, 3, d0)), ("local_encoder.bias", (d0,))]
    p = c["local_patch_size"] * ws
    t += [("region_encoder.1.kernel", (1, 1, 3 * p * p, d0)), ("region_encoder.1.bias", (d0,))]
    cin = d0
    for s, (d, depth) in enumerate(zip(dims, depths)):
        pre = f"region_layers.{s}"
        if s:
            t += [(pre + ".down.conv.kernel", (3, 3, cin, d)), (pre + ".down.conv.bias", (d,))]
            if c["use_peg"]:
                t += [(pre + ".peg.proj.kernel", (3, 3, 1, d)), (pre + ".peg.proj.bias", (d,))]
        t += [(pre + ".transformer.local_rel_pos_bias", ((2 * ws - 1) ** 2, HEADS))]
        for l in range(depth):
            q = f"{pre}.transformer.{l}"
            t += [(q + ".attn.norm.gamma", (d,)), (q + ".attn.norm.beta", (d,)), (q + ".attn.to_qkv.kernel", (d, 3 * inner)),
                  (q + ".attn.to_out.kernel", (inner, d)), (q + ".attn.to_out.bias", (d,)),
                  (q + ".ff.norm.gamma", (d,)), (q + ".ff.norm.beta", (d,)), (q + ".ff.fc1.kernel", (d, d * MULT)), (q + ".ff.fc1.bias", (d * MULT,)),
                  (q + ".ff.fc2.kernel", (d * MULT, d)), (q + ".ff.fc2.bias", (d,))]
        cin = d
    t += [("to_logits.norm.gamma", (cin,)), ("to_logits.norm.beta", (cin,)), ("to_logits.kernel", (cin, c["num_classes"])),
          ("to_logits.bias", (c["num_classes"],))]
    out, off = [], 0
    for n, s in t:
        out.append((n, s, off))
        off += int(np.prod(s))
    return out


def is_embedding(name: str) -> bool:
    return name.endswith(".local_rel_pos_bias")


def init_params(table, seed: int = 1) -> dict:
    """Seeded weights for a table: every tensor moved off its default so that each gradient is exercised.  Kernels are scaled by their fan-in;
    the relative-position embeddings are EMB_SCALE * N(0, 1): of the order of the scores, so that the logits feel them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape, _ in table:
        leaf = name.split(".")[-1]
        if leaf == "gamma":
            a = 1.0 + 0.2 * rng.standard_normal(shape)
        elif leaf == "kernel":
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[:-1])))
        elif leaf == "local_rel_pos_bias":
            a = EMB_SCALE * rng.standard_normal(shape)
        else:
            a = 0.2 * rng.standard_normal(shape)
        out[name] = a.astype(np.float32).astype(np.float64)   # values a float32 engine holds exactly
    return out


def bias_indices(wh: int, ww: int, ws: int) -> np.ndarray:
    """[wh ww, wh ww] rows of the embedding table: (dh + ws - 1) + (dw + ws - 1) (2 ws - 1) for token i = (y1, x1) against j = (y2, x2),
    dh = y1 - y2, dw = x1 - x2 (regionvit.py:144-152)."""
    n = wh * ww
    out = np.empty((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            dh, dw = i // ww - j // ww, i % ww - j % ww
            out[i, j] = (dh + ws - 1) + (dw + ws - 1) * (2 * ws - 1)
    return out


def position_bias(emb, wh: int, ww: int, ws: int):
    """[heads, 1 + n, 1 + n]: the table gathered per head, one zero row and column in front for the region token (:153-155)."""
    if wh > ws or ww > ws:
        raise ValueError(f"a {wh} x {ww} window leaves the table of window_size = {ws}")
    b = emb[torch.as_tensor(bias_indices(wh, ww, ws))]      # [n, n, heads]
    return F.pad(b.permute(2, 0, 1), (1, 0, 1, 0))


def _kln(x, P, pre):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + LN_EPS) * P[pre + ".gamma"] + P[pre + ".beta"]


def _gelu(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def _conv(x, P, pre, k, st, groups=1):
    pt, pb = same_pads(x.shape[1], k, st)
    pl, pr = same_pads(x.shape[2], k, st)
    w = P[pre + ".kernel"]
    w = w.permute(3, 2, 0, 1) if groups == 1 else w.permute(3, 2, 0, 1).reshape(w.shape[3], 1, k, k)
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w, P[pre + ".bias"], stride=st, groups=groups)
    return y.permute(0, 2, 3, 1)


def attention(x, P, pre, bias=None):
    """regionvit.py:93-116 on [sequences, n, d]."""
    s, n, d = x.shape
    qkv = _kln(x, P, pre + ".norm") @ P[pre + ".to_qkv.kernel"]
    q, k, v = (t.reshape(s, n, HEADS, DIM_HEAD).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    sim = (q * DIM_HEAD ** -0.5) @ k.transpose(-1, -2)
    if bias is not None:
        sim = sim + bias
    o = (torch.softmax(sim, -1) @ v).permute(0, 2, 1, 3).reshape(s, n, HEADS * DIM_HEAD)
    return o @ P[pre + ".to_out.kernel"] + P[pre + ".to_out.bias"]


def mlp(x, P, pre):
    y = _gelu(_kln(x, P, pre + ".norm") @ P[pre + ".fc1.kernel"] + P[pre + ".fc1.bias"])
    return y @ P[pre + ".fc2.kernel"] + P[pre + ".fc2.bias"]


def to_windows(local, region):
    """[(b rh rw), 1 + wh ww, d]: every window's tokens behind its region token (:163-168)."""
    b, lh, lw, d = local.shape
    rh, rw = region.shape[1:3]
    wh, ww = lh // rh, lw // rw
    win = local.reshape(b, rh, wh, rw, ww, d).permute(0, 1, 3, 2, 4, 5).reshape(b * rh * rw, wh * ww, d)
    return torch.cat([region.reshape(b * rh * rw, 1, d), win], dim=1)


def from_windows(x, b, lh, lw, rh, rw):
    """(local [b, lh, lw, d], region [b, rh, rw, d]) of [(b rh rw), 1 + wh ww, d] (:175-177)."""
    d = x.shape[-1]
    wh, ww = lh // rh, lw // rw
    local = x[:, 1:].reshape(b, rh, rw, wh, ww, d).permute(0, 1, 3, 2, 4, 5).reshape(b, lh, lw, d)
    return local, x[:, 0].reshape(b, rh, rw, d)


def r2l(local, region, P, pre, depth, ws, taps=None):
    """regionvit.py:135-182."""
    b, lh, lw, d = local.shape
    rh, rw = region.shape[1:3]
    wh, ww = lh // rh, lw // rw
    if lh % rh or lw % rw or lh // wh != rh or lw // ww != rw:
        raise ValueError("the region map does not cut the local map into windows")
    bias = position_bias(P[pre + ".local_rel_pos_bias"], wh, ww, ws) if depth else None
    if taps is not None and depth:
        taps["bias." + pre] = bias
    for l in range(depth):
        q = f"{pre}.{l}"
        rs = region.reshape(b, rh * rw, d)
        region = (attention(rs, P, q + ".attn") + rs).reshape(b, rh, rw, d)
        x = to_windows(local, region)
        x = attention(x, P, q + ".attn", bias) + x
        x = mlp(x, P, q + ".ff") + x
        local, region = from_windows(x, b, lh, lw, rh, rw)
    return local, region


def forward(kw: dict, P: dict, img, taps: dict | None = None):
    """RegionViT.call(img) in the dtype of its inputs; kw = the constructor kwargs."""
    c = config_of(kw)
    b, H, W, C = img.shape
    maps_of(kw, H, W)
    if c["tokenize_local_3_conv"]:
        x = _gelu(_kln(_conv(img, P, "local_encoder.0", 3, 2), P, "local_encoder.1"))
        x = _gelu(_kln(_conv(x, P, "local_encoder.3", 3, 2), P, "local_encoder.4"))
        local = _conv(x, P, "local_encoder.6", 3, 1)
    else:
        local = _conv(img, P, "local_encoder", 8, 4)
    p = c["local_patch_size"] * c["window_size"]
    rows = img.reshape(b, H // p, p, W // p, p, C).permute(0, 1, 3, 5, 2, 4).reshape(b, H // p, W // p, C * p * p)   # 'b h w (c p1 p2)'
    region = rows @ P["region_encoder.1.kernel"].reshape(C * p * p, -1) + P["region_encoder.1.bias"]
    for s, depth in enumerate(c["depth"]):
        pre = f"region_layers.{s}"
        if s:
            local, region = _conv(local, P, pre + ".down.conv", 3, 2), _conv(region, P, pre + ".down.conv", 3, 2)
            if c["use_peg"]:
                local = _conv(local, P, pre + ".peg.proj", 3, 1, groups=local.shape[-1]) + local
        local, region = r2l(local, region, P, pre + ".transformer", depth, c["window_size"], taps)
        if taps is not None:
            taps[f"local.{s}"], taps[f"region.{s}"] = local, region
    x = _kln(region.mean(dim=(1, 2)), P, "to_logits.norm")
    return x @ P["to_logits.kernel"] + P["to_logits.bias"]


def forward_backward(kw: dict, params: dict, img: np.ndarray, dlogits: np.ndarray, dtype=torch.float64):
    """(logits, {name: d(sum(logits * dlogits))/d(param)}, d/d(img)) in `dtype`; a parameter the graph does not reach gets zeros."""
    P = {n: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for n, v in params.items()}
    x = torch.tensor(np.asarray(img, np.float64), dtype=dtype, requires_grad=True)
    logits = forward(kw, P, x)
    loss = (logits * torch.tensor(np.asarray(dlogits, np.float64), dtype=dtype)).sum()
    names = list(P)
    g = torch.autograd.grad(loss, [x] + [P[n] for n in names], allow_unused=True)
    grads = {n: (t.detach().numpy() if t is not None else np.zeros(np.shape(params[n]))) for n, t in zip(names, g[1:])}
    return logits.detach().numpy(), grads, g[0].detach().numpy()
