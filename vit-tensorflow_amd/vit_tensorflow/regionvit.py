"""Drop-in for vit_tensorflow/regionvit.py: `RegionViT(...)` (regionvit.py:184-263).  The two encoders, the shared Downsample, the PEG, the window
partition with every window's region token in front, the attention with the stage's learned per-head position bias, the MLPs and the head run
in HIP behind the C ABI (csrc/regionvit.hip, csrc/regionvit_ops.hip, csrc/attn_window.hip and the BIAS form of csrc/attn_lsa.hip through the
nest_block form of csrc/engine.hip); parameters are in the order of DESIGN.md section 26, with the shapes the reference's variables have (a
Conv2D kernel [k, k, in, out], a Dense kernel [in, out], the Embedding [(2 window_size - 1)^2, 4]).

The reference's constructor takes no image size and no parameter depends on one: the native handle is created at the first call from the
image's H x W, and created again (weights kept) when H x W changes or a larger batch arrives.  `image_size=` (an int or an (H, W) pair)
creates it eagerly.

The window of a stage is (local map // region map), not window_size: a 28 x 56 image at window_size 7 runs windows of 7x7, 4x7, 2x4 and 1x2.
`local_rel_pos_bias` is trained: its gradient is the sum over images, windows and the stage's layers of dS, gathered through the index.  As in
the reference, the local tokens behind the last layer reach nothing (that layer gives its embedding an exactly zero gradient) and a stage
without layers gives its embedding zeros.

Only the deterministic path exists: `ff_dropout == 0`, where `training=True` (the reference's default) and `training=False` compute the same
thing.  `ff_dropout > 0` with a truthy `training` raises NotImplementedError.  `attn_dropout` is accepted and unused, as in the reference."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._composite import ImageSizedComposite, NativeComposite


def cast_tuple(val, length=1):
    """regionvit.py:17-18."""
    return val if isinstance(val, tuple) else ((val,) * length)


class RegionViT(ImageSizedComposite):
    _PREFIX, _NAME = "vitx_regionvit", "RegionViT"

    def __init__(self, dim=(64, 128, 256, 512), depth=(2, 2, 8, 2), window_size=7, num_classes=1000, tokenize_local_3_conv=False,
                 local_patch_size=4, use_peg=False, attn_dropout=0.0, ff_dropout=0.0, **kwargs):
        """The reference's arguments (regionvit.py:185-195); dim and depth a scalar or a 4-tuple as cast_tuple allows.  Refused with ValueError,
        at construction or -- where the image decides -- at the call: a tuple whose length is not 4 (the reference's asserts); an image the
        region patch (local_patch_size * window_size) does not divide (:251); a stage whose region map does not cut its local map into
        windows (the reference's rearrange fails there); a window larger than window_size (the index leaves the table); a window plus its
        region token, or a region sequence, of more than 288 tokens; compute='bf16' with a stage width that is no multiple of 64.
        A batch whose (images x windows) of a stage with layers exceeds 65535 -- batch 1024 at 224 pixels and window_size 7 -- is refused at the
        call with VitxError (the attention kernels put the sequence on the grid's z axis).

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        image_size=int|(H, W) (create the native handle now instead of at the first call), window_attn=None|True|False (the one-wave-per-window
        attention kernels for the window sequences: bf16 mode, at most 64 tokens; None: the measured default -- DESIGN.md section 26; True:
        wherever they apply; False: nowhere)."""
        compute, max_batch, device, seed, image_size, window_attn = self._pop_extras(kwargs, image_size=None, window_attn=None)
        dims, depths = cast_tuple(dim, 4), cast_tuple(depth, 4)
        if len(dims) != 4:
            raise ValueError(f"dim needs to be a single value or a tuple of length 4 (regionvit.py:199), got {len(dims)} entries")
        if len(depths) != 4:
            raise ValueError(f"depth needs to be a single value or a tuple of length 4 (regionvit.py:200), got {len(depths)} entries")
        dims, depths = tuple(int(d) for d in dims), tuple(int(d) for d in depths)
        if compute == "bf16" and any(d % 64 for d in dims):
            raise ValueError(f"compute='bf16' needs every stage's dim to be a multiple of 64 (use 'fp32' or 'bf16x3' otherwise); got {dims}")
        cfg = N.RegionViTConfig()
        cfg.num_classes = int(num_classes)
        for i in range(4):
            cfg.dim[i], cfg.depth[i] = dims[i], depths[i]
        cfg.window_size, cfg.local_patch_size = int(window_size), int(local_patch_size)
        cfg.tokenize_local_3_conv, cfg.use_peg = int(bool(tokenize_local_3_conv)), int(bool(use_peg))
        cfg.ln_eps = 1e-3   # Keras LayerNormalization's default
        cfg.window_attn = 0 if window_attn is None else (1 if window_attn else -1)
        self.num_classes, self.dim, self.depth = int(num_classes), dims, depths
        self.window_size, self.local_patch_size = int(window_size), int(local_patch_size)
        self.region_patch_size = self.local_patch_size * self.window_size
        self.tokenize_local_3_conv, self.use_peg = bool(tokenize_local_3_conv), bool(use_peg)
        self.attn_dropout, self.ff_dropout = float(attn_dropout), float(ff_dropout)
        # (no image yet: no parameter depends on one)
        self._start(cfg, self._refused_as_value_error(N.regionvit_param_table, cfg), compute, max_batch, device, seed)
        self._eager_handle(image_size, max_batch)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNormalization ones / zeros; Embedding uniform(-0.05, 0.05)
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("gamma",), draws={"local_rel_pos_bias": lambda r, n: r.uniform(-0.05, 0.05, n)})

    # ---- geometry
    def maps_of(self, H: int, W: int):
        """[((lh, lw), (rh, rw), (wh, ww))] of the four stages for an H x W image: local map, region map, window; ValueError for an image
        the model cannot take."""
        cfg = N.RegionViTConfig.from_buffer_copy(self._cfg)
        cfg.image_h, cfg.image_w = int(H), int(W)
        self._refused_as_value_error(N.regionvit_param_table, cfg)
        p = self.region_patch_size
        lh, lw, rh, rw = -(-H // 4), -(-W // 4), H // p, W // p
        out = []
        for s in range(4):
            if s:
                lh, lw, rh, rw = -(-lh // 2), -(-lw // 2), -(-rh // 2), -(-rw // 2)
            out.append(((lh, lw), (rh, rw), (lh // rh, lw // rw)))
        return out

    _check_image = maps_of

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """RegionViT.call(x, training=True) (regionvit.py:249-263).  img: NHWC numpy or torch."""
        if training and self.ff_dropout > 0:
            raise NotImplementedError(f"RegionViT(ff_dropout={self.ff_dropout}) with training=True needs the Dropout masks of regionvit.py:72; "
                                      "they are not built.  Call with training=False, or construct with ff_dropout=0.0 (then training=True is "
                                      "the deterministic path).")
        x, proto = self._nhwc(img)
        return self._forward(self._ensure_handle(*x.shape[:3]), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'local.<s>' [b, lh_s, lw_s, dim_s] and 'region.<s>' [b, rh_s, rw_s, dim_s] (the maps
        behind stage s), 'bias.<s>' [4, n, n] (the stage's position bias as its attention adds it, n = 1 + window tokens), 'pooled' [b, dim_4]."""
        b, H, W, _ = self._read_shape()
        maps = self.maps_of(H, W)
        cap = max([b * lh * lw * d for ((lh, lw), _, _), d in zip(maps, self.dim)] + [4 * (1 + wh * ww) ** 2 for _, _, (wh, ww) in maps])
        out = self._read_raw(which, cap)
        if which == "pooled":
            return out.reshape(b, -1)
        s = int(which.split(".")[1])
        if which.startswith("bias."):
            n = 1 + maps[s][2][0] * maps[s][2][1]
            return out.reshape(4, n, n)
        h, w = maps[s][0] if which.startswith("local.") else maps[s][1]
        return out.reshape(b, h, w, -1)

    def partition(self, region, local) -> np.ndarray:
        """The window partition kernel on host tensors (tests, bisecting): region [b, rh, rw, c] and local [b, rh * wh, rw * ww, c] ->
        tokens [(b rh rw), 1 + wh * ww, c], every window's region token in front (regionvit.py:163-168).  Needs the native handle."""
        region, local = np.ascontiguousarray(region, dtype=np.float32), np.ascontiguousarray(local, dtype=np.float32)
        b, rh, rw, c = region.shape
        wh, ww = local.shape[1] // rh, local.shape[2] // rw
        assert local.shape == (b, rh * wh, rw * ww, c)
        tokens = np.empty((b * rh * rw, 1 + wh * ww, c), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(self._native("partition")(self._ensure_handle(1), p(region), p(local), p(tokens), b, rh, rw, wh, ww, c, 0))
        return tokens

    def unpartition(self, tokens, b: int, rh: int, rw: int, wh: int, ww: int):
        """The way back (:175-177): tokens [(b rh rw), 1 + wh * ww, c] -> (region [b, rh, rw, c], local [b, rh * wh, rw * ww, c])."""
        tokens = np.ascontiguousarray(tokens, dtype=np.float32)
        c = tokens.shape[-1]
        assert tokens.shape == (b * rh * rw, 1 + wh * ww, c)
        region, local = np.empty((b, rh, rw, c), np.float32), np.empty((b, rh * wh, rw * ww, c), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(self._native("partition")(self._ensure_handle(1), p(region), p(local), p(tokens), b, rh, rw, wh, ww, c, 1))
        return region, local

    def attention(self, qkv, d_o, bias, tail_rows: int = 0, tail_value: float = 0.0, window_kernel: bool = True):
        """One biased attention with a per-head bias, alone, on bf16 storage (tests, bisecting): qkv [b, n, 3, h, 32], d_o [b, n, h * 32],
        bias [h, n, n] -> (o [b, n, h * 32], lse [b, h, n], dqkv [b, n, 3, h, 32], dbias [h, n, n], o_tail, dqkv_tail); dbias is the sum over
        the b sequences of dS.  Every device buffer carries tail_rows extra rows filled with tail_value (NaN allowed); the tails of the two
        output buffers come back as they are after the run.  window_kernel: the one-wave-per-window kernels (n <= 64), else the BIAS form of
        the small-head kernels.  Needs the native handle."""
        qkv, d_o = np.ascontiguousarray(qkv, dtype=np.float32), np.ascontiguousarray(d_o, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        b, n, _, h, dh = qkv.shape
        assert dh == 32 and d_o.shape == (b, n, h * 32) and bias.shape == (h, n, n)
        rows = b * n + int(tail_rows)
        o, lse, dqkv = np.empty((rows, h * 32), np.float32), np.empty((b, h, n), np.float32), np.empty((rows, 3 * h * 32), np.float32)
        dbias = np.empty((h, n, n), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(self._native("attn")(self._ensure_handle(1), p(qkv), p(d_o), p(bias), b, n, h, int(tail_rows), float(tail_value),
                                     int(bool(window_kernel)), p(o), p(lse), p(dqkv), p(dbias)))
        return (o[:b * n].reshape(b, n, h * 32), lse, dqkv[:b * n].reshape(b, n, 3, h, 32), dbias, o[b * n:], dqkv[b * n:])

    apply_gradients = NativeComposite.optimizer_step
