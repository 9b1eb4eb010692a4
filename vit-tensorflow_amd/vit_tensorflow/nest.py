"""Drop-in for vit_tensorflow/nest.py: `NesT(...)` (nest.py:150-216).  The patch embedding, the block partition with its positional add, the
transformer blocks on the (b * blocks^2) block-local sequences, the aggregation (Conv2D 3x3 'SAME', channel LayerNorm, MaxPool2D 3/2 'SAME')
and the head run in HIP behind the C ABI (csrc/nest.hip, csrc/nest_ops.hip, the plain mode of csrc/attn_lsa.hip); parameters are in the order of
DESIGN.md section 20, with the shapes the reference's variables have (every 1x1 Conv2D kernel is [1, 1, in, out]).

Only the deterministic path exists: `dropout == 0`, where `training=True` (the reference's default) and `training=False` compute the same thing.
`dropout > 0` with a truthy `training` raises NotImplementedError."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from ._composite import NativeComposite, as_host, like


def cast_tuple(val, depth):
    return val if isinstance(val, tuple) else ((val,) * depth)


class NesT(NativeComposite):
    _PREFIX, _NAME = "vitx_nest", "NesT"

    def __init__(self, image_size, patch_size, num_classes, dim, heads, num_hierarchies, block_repeats, mlp_mult=4, dropout=0.0, **kwargs):
        """The reference's arguments (nest.py:151-160).  Refused with ValueError: an image_size that patch_size does not divide (the reference's
        assertion text, nest.py:163); a feature map that 2^(num_hierarchies - 1) does not divide (the reference fails there inside einops at call
        time); a block_repeats tuple whose length is not num_hierarchies (the reference's zip, nest.py:187, silently builds fewer levels).

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        conv_chunk=int (images per im2col pass of an aggregation; default: sized from a fixed workspace), small_attn=None|True|False (the plain
        small-head attention kernels for dim_head 16 / 32 and at most 288 tokens; None: where they measured faster than the materialised path,
        which is the bf16 mode -- DESIGN.md section 20; True: wherever they apply; False: nowhere)."""
        compute, max_batch, device, seed, conv_chunk, small_attn = (kwargs.pop(k, v) for k, v in (
            ("compute", "fp32"), ("max_batch", None), ("device", 0), ("seed", None), ("conv_chunk", 0), ("small_attn", None)))
        if kwargs:
            raise TypeError(f"NesT() got an unexpected keyword argument '{next(iter(kwargs))}'")
        assert compute in ("fp32", "bf16", "bf16x3"), "compute must be 'fp32' (parity), 'bf16' (throughput) or 'bf16x3'"
        if image_size % patch_size != 0:
            raise ValueError("Image dimensions must be divisible by the patch size.")
        fmap, blocks = image_size // patch_size, 2 ** (num_hierarchies - 1)
        if num_hierarchies < 1 or num_hierarchies > 8:
            raise ValueError("num_hierarchies must be in [1, 8]")
        if fmap % blocks != 0:
            raise ValueError(f"the feature map ({fmap} x {fmap}) must be divisible by 2^(num_hierarchies - 1) = {blocks}: the block partition "
                             "'b (b1 h) (b2 w) c' (nest.py:209) needs it")
        repeats = cast_tuple(block_repeats, num_hierarchies)
        if len(repeats) != num_hierarchies:
            raise ValueError(f"block_repeats has {len(repeats)} entries for num_hierarchies = {num_hierarchies} (the reference's zip would "
                             "silently build fewer levels, nest.py:187)")
        cfg = N.NesTConfig()
        for k, v in dict(image_size=image_size, patch_size=patch_size, num_classes=num_classes, dim=dim, heads=heads,
                         num_hierarchies=num_hierarchies, mlp_mult=mlp_mult, conv_chunk=conv_chunk).items():
            setattr(cfg, k, int(v))
        for i, r in enumerate(repeats):
            cfg.block_repeats[i] = int(r)
        cfg.ln_eps = 1e-5   # nest.py:29
        cfg.small_attn = 0 if small_attn is None else (1 if small_attn else -1)
        cfg.compute = {"fp32": N.COMPUTE_FP32, "bf16": N.COMPUTE_BF16, "bf16x3": N.COMPUTE_BF16X3}[compute]
        cfg.max_batch = int(max_batch or 0)
        cfg.device_id = int(device)
        self._cfg = cfg
        self.compute = compute
        self.image_size, self.patch_size, self.num_classes, self.dim = int(image_size), int(patch_size), int(num_classes), int(dim)
        self.num_hierarchies, self.block_repeats, self.dropout = int(num_hierarchies), tuple(int(r) for r in repeats), float(dropout)
        self.seq_len = (fmap // blocks) ** 2
        self._handle = None
        try:
            self._table, self._n = N.nest_param_table(cfg)
        except N.VitxError as e:
            raise ValueError(e.message) from None
        self._blob = np.zeros(self._n, dtype=np.float32)
        self._device_newer = False
        self._init_weights(np.random.default_rng(seed))

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNorm ones / zeros (nest.py:33-34); pos_emb standard normal (nest.py:129)
    def _init_weights(self, rng: np.random.Generator) -> None:
        for name, shape, off in self._table:
            n = int(np.prod(shape))
            leaf = name.split(".")[-1]
            if leaf == "pos_emb":
                v = rng.standard_normal(n)
            elif leaf == "kernel":
                recv = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
                lim = math.sqrt(6.0 / (recv * shape[-2] + recv * shape[-1]))
                v = rng.uniform(-lim, lim, n)
            elif leaf == "g":
                v = np.ones(n)
            else:  # bias / b
                v = np.zeros(n)
            self._blob[off:off + n] = v.astype(np.float32)

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """NesT.call(img, training=True) (nest.py:202-216).  img: NHWC numpy or torch of exactly the constructed image_size."""
        if training and self.dropout > 0:
            raise NotImplementedError(f"NesT(dropout={self.dropout}) with training=True needs the Dropout masks of nest.py:68,70,90; they are not "
                                      "built.  Call with training=False, or construct with dropout=0.0 (then training=True is the deterministic path).")
        x, proto = as_host(img)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("expected NHWC images [b, H, W, 3]")
        b, H, W, _c = x.shape
        if (H, W) != (self.image_size, self.image_size):
            raise ValueError(f"NesT was built for image_size {self.image_size}; got images of {(H, W)} (the positional embeddings and the block "
                             "partition belong to the constructed size)")
        h = self._ensure_handle(b)
        self._img_shape = (b, H, W, 3)
        out = np.empty((b, self.num_classes), dtype=np.float32)
        N.check(N.lib().vitx_nest_forward(h, x.ctypes.data_as(C.c_void_p), b, out.ctypes.data_as(C.c_void_p)))
        return like(out, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'embedded' [b, f, f, dim], 'level.<i>' [b, f_i, f_i, d_i] (the level's output after
        un-blocking, before aggregation), 'aggregated.<i>' [b, f_i / 2, f_i / 2, d_{i+1}], 'pooled' [b, d_last]."""
        if self._handle is None:
            raise N.VitxError(N.ERR_STATE, "read requires a preceding forward")
        b = self._img_shape[0]
        fmap = self.image_size // self.patch_size
        cap = b * fmap * fmap * self.dim * 2
        buf, n = np.empty(cap, dtype=np.float32), C.c_int64()
        N.check(N.lib().vitx_nest_read(self._handle, which.encode(), buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        out = buf[:n.value]
        if which == "pooled":
            return out.reshape(b, -1)
        i = 0 if which == "embedded" else int(which.split(".")[1])
        f = (fmap >> i) if not which.startswith("aggregated") else (fmap >> (i + 1))
        return out.reshape(b, f, f, -1)

    def profile(self, fn):
        """Runs fn() between vitx_nest_profile_begin / _end: {class: (launches, total_ms)}."""
        h = self._ensure_handle(1)
        N.check(N.lib().vitx_nest_profile_begin(h))
        try:
            fn()
        finally:
            stats, n = (N.KernelStat * 256)(), C.c_int32()
            N.check(N.lib().vitx_nest_profile_end(h, stats, 256, C.byref(n)))
        return {stats[i].name.decode(): (int(stats[i].launches), float(stats[i].total_ms)) for i in range(min(n.value, 256))}

    apply_gradients = NativeComposite.optimizer_step
