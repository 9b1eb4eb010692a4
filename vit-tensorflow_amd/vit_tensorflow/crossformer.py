"""Drop-in for vit_tensorflow/crossformer.py: `CrossFormer(...)` (crossformer.py:205-257).  The cross-scale embeddings, the short and the
dilated ("long") window partitions, the biased window attention, the MLPs and the head run in HIP behind the C ABI (csrc/crossformer.hip,
csrc/crossformer_ops.hip, the BIAS form of csrc/attn_lsa.hip through the nest_block form of csrc/engine.hip); parameters are in the order of
DESIGN.md section 23, with the shapes the reference's variables have (every 1x1 Conv2D kernel is [1, 1, in, out], a cross-embed kernel
[k, k, in, width], the position-bias network's Dense kernels [in, out]).

The reference's constructor takes no image size and no parameter depends on one: the native handle is created at the first call from the
image's H x W, and created again (weights kept) when H x W changes or a larger batch arrives.  `image_size=` (an int or an (H, W) pair)
creates it eagerly.

The dynamic position bias receives no gradient in the reference (crossformer.py:163 leaves the tape through `.numpy()`): the gradients of
the `dpb.*` variables are returned as exact zeros.  The bias is evaluated on the device whenever the weights change.

Only the deterministic path exists: `ff_dropout == 0`, where `training=True` (the reference's default) and `training=False` compute the same
thing.  `ff_dropout > 0` with a truthy `training` raises NotImplementedError.  `attn_dropout` is accepted and unused, as in the reference
(Attention never applies it)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._composite import ImageSizedComposite, NativeComposite


def cast_tuple(val, length=1):
    """crossformer.py:11-12."""
    return val if isinstance(val, tuple) else ((val,) * length)


class CrossFormer(ImageSizedComposite):
    _PREFIX, _NAME = "vitx_crossformer", "CrossFormer"

    def __init__(self, dim=(64, 128, 256, 512), depth=(2, 2, 8, 2), global_window_size=(8, 4, 2, 1), local_window_size=7,
                 cross_embed_kernel_sizes=((4, 8, 16, 32), (2, 4), (2, 4), (2, 4)), cross_embed_strides=(4, 2, 2, 2), num_classes=1000,
                 attn_dropout=0.0, ff_dropout=0.0, **kwargs):
        """The reference's arguments (crossformer.py:206-216), each a scalar or a 4-tuple as cast_tuple allows.  Refused with ValueError, at
        construction or -- where the image decides -- at the call: a tuple whose length is not 4 (the reference's asserts); a stage map that
        its local or global window does not divide (the reference fails inside einops); dim < 32 (heads = dim // 32 would be 0); a window of
        more than 288 tokens; compute='bf16' with a stage width that is no multiple of 64.

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        image_size=int|(H, W) (create the native handle now instead of at the first call), window_attn=None|True|False (the one-wave-per-window
        attention kernels: bf16 mode, at most 64 tokens; None: where they measured faster than the BIAS form of the small-head kernels --
        DESIGN.md section 23; True: wherever they apply; False: nowhere)."""
        compute, max_batch, device, seed, image_size, window_attn = self._pop_extras(kwargs, image_size=None, window_attn=None)
        cols = dict(dim=dim, depth=depth, global_window_size=global_window_size, local_window_size=local_window_size,
                    cross_embed_kernel_sizes=cross_embed_kernel_sizes, cross_embed_strides=cross_embed_strides)
        cols = {k: cast_tuple(v, 4) for k, v in cols.items()}
        for k, v in cols.items():
            if len(v) != 4:
                raise ValueError(f"{k} must be a scalar or a tuple of 4 (crossformer.py:225-230), got {len(v)} entries")
        try:
            kernels = [tuple(int(k) for k in ks) for ks in cols["cross_embed_kernel_sizes"]]
        except TypeError:
            raise ValueError("cross_embed_kernel_sizes must hold one sequence of kernel sizes per stage") from None
        if any(not 1 <= len(ks) <= N.CF_MAX_SCALES for ks in kernels):
            raise ValueError(f"1 to {N.CF_MAX_SCALES} cross_embed_kernel_sizes per stage")
        dims = tuple(int(d) for d in cols["dim"])
        if compute == "bf16" and all(d >= 32 for d in dims) and any(d % 64 for d in dims):
            raise ValueError(f"compute='bf16' needs every stage's dim to be a multiple of 64 (use 'fp32' or 'bf16x3' otherwise); got {dims}")
        cfg = N.CrossFormerConfig()
        cfg.num_classes = int(num_classes)
        for i in range(4):
            cfg.dim[i], cfg.depth[i] = dims[i], int(cols["depth"][i])
            cfg.global_window_size[i], cfg.local_window_size[i] = int(cols["global_window_size"][i]), int(cols["local_window_size"][i])
            cfg.strides[i] = int(cols["cross_embed_strides"][i])
            cfg.n_kernels[i] = len(kernels[i])
            for j, k in enumerate(kernels[i]):
                cfg.kernel_sizes[i][j] = k
        cfg.ln_eps = 1e-5   # crossformer.py:75
        cfg.window_attn = 0 if window_attn is None else (1 if window_attn else -1)
        self.num_classes, self.dim, self.depth = int(num_classes), dims, tuple(int(v) for v in cols["depth"])
        self.global_window_size = tuple(int(v) for v in cols["global_window_size"])
        self.local_window_size = tuple(int(v) for v in cols["local_window_size"])
        self.cross_embed_kernel_sizes, self.cross_embed_strides = tuple(kernels), tuple(int(v) for v in cols["cross_embed_strides"])
        self.attn_dropout, self.ff_dropout = float(attn_dropout), float(ff_dropout)
        # (no image yet: no parameter depends on one)
        self._start(cfg, self._refused_as_value_error(N.crossformer_param_table, cfg), compute, max_batch, device, seed)
        self._eager_handle(image_size, max_batch)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNorm / LayerNormalization ones / zeros (crossformer.py:79-80)
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("g", "gamma"))

    # ---- geometry
    def maps_of(self, H: int, W: int):
        """[(H_s, W_s)] of the four stages for an H x W image ('SAME': ceil(extent / stride)); ValueError where a stage's local or global
        window does not divide its map."""
        cfg = N.CrossFormerConfig.from_buffer_copy(self._cfg)
        cfg.image_h, cfg.image_w = int(H), int(W)
        self._refused_as_value_error(N.crossformer_param_table, cfg)
        out = []
        for s in self.cross_embed_strides:
            H, W = -(-H // s), -(-W // s)
            out.append((H, W))
        return out

    _check_image = maps_of

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """CrossFormer.call(x, training=True) (crossformer.py:250-257).  img: NHWC numpy or torch."""
        if training and self.ff_dropout > 0:
            raise NotImplementedError(f"CrossFormer(ff_dropout={self.ff_dropout}) with training=True needs the Dropout masks of crossformer.py:97; "
                                      "they are not built.  Call with training=False, or construct with ff_dropout=0.0 (then training=True is "
                                      "the deterministic path).")
        x, proto = self._nhwc(img)
        return self._forward(self._ensure_handle(*x.shape[:3]), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'embedded.<s>' (stage s's cross-scale embedding) and 'stage.<s>' (its output), each
        [b, H_s, W_s, dim_s]; 'pooled' [b, dim_4]; 'bias.<s>.<l>.short' / 'bias.<s>.<l>.long': the [n, n] position bias that layer l's short
        / long attention adds to its scores (crossformer.py:163)."""
        b, H, W, _ = self._read_shape()
        maps = self.maps_of(H, W)
        cap = max([b * h * w * d for (h, w), d in zip(maps, self.dim)] + [max(max(self.global_window_size), max(self.local_window_size)) ** 4])
        out = self._read_raw(which, cap)
        if which == "pooled":
            return out.reshape(b, -1)
        if which.startswith("bias."):
            n = int(round(np.sqrt(out.size)))
            return out.reshape(n, n)
        h, w = maps[int(which.split(".")[1])]
        return out.reshape(b, h, w, -1)

    def partition(self, x, g: int, inverse: bool = False) -> np.ndarray:
        """The dilated partition kernel on a host tensor (tests, bisecting).  x [b, H, W, c] -> [(b h w), g * g, c] with h = H // g, w = W // g
        ('b (l1 h) (l2 w) c -> (b h w) (l1 l2) c', crossformer.py:146); inverse=True: the way back (:178) -- x then holds the tokens, still
        shaped [b, H, W, c].  Needs the native handle (a call before it, or image_size=)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        b, H, W, c = x.shape
        out = np.empty_like(x)
        N.check(self._native("partition")(self._ensure_handle(1), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), b, H, W, int(g), c,
                                          int(bool(inverse))))
        return out if inverse else out.reshape(b * (H // g) * (W // g), g * g, c)

    def window_attention(self, qkv, d_o, bias, tail_rows: int = 0, tail_value: float = 0.0, window_kernel: bool = True):
        """The biased attention kernels alone on bf16 storage (tests, bisecting): qkv [b, n, 3, h, 32], d_o [b, n, h * 32], bias [n, n] ->
        (o [b, n, h * 32], lse [b, h, n], dqkv [b, n, 3, h, 32], o_tail, dqkv_tail).  Every device buffer carries tail_rows extra rows filled
        with tail_value (NaN allowed); the tails of the two output buffers come back as they are after the run.  window_kernel: the
        one-wave-per-window kernels (n <= 64), else the BIAS form of the small-head kernels.  Needs the native handle."""
        qkv, d_o = np.ascontiguousarray(qkv, dtype=np.float32), np.ascontiguousarray(d_o, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        b, n, _, h, dh = qkv.shape
        assert dh == 32 and d_o.shape == (b, n, h * 32) and bias.shape == (n, n)
        rows = b * n + int(tail_rows)
        o, lse, dqkv = np.empty((rows, h * 32), np.float32), np.empty((b, h, n), np.float32), np.empty((rows, 3 * h * 32), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(self._native("window_attn")(self._ensure_handle(1), p(qkv), p(d_o), p(bias), b, n, h, int(tail_rows), float(tail_value),
                                            int(bool(window_kernel)), p(o), p(lse), p(dqkv)))
        return (o[:b * n].reshape(b, n, h * 32), lse, dqkv[:b * n].reshape(b, n, 3, h, 32), o[b * n:], dqkv[b * n:])

    apply_gradients = NativeComposite.optimizer_step
