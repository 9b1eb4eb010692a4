"""Drop-in for vit_tensorflow/nest.py: `NesT(...)` (nest.py:150-216).  The patch embedding, the block partition with its positional add, the
transformer blocks on the (b * blocks^2) block-local sequences, the aggregation (Conv2D 3x3 'SAME', channel LayerNorm, MaxPool2D 3/2 'SAME')
and the head run in HIP behind the C ABI (csrc/nest.hip, csrc/nest_ops.hip, the plain mode of csrc/attn_lsa.hip); parameters are in the order of
DESIGN.md section 20, with the shapes the reference's variables have (every 1x1 Conv2D kernel is [1, 1, in, out]).

Only the deterministic path exists: `dropout == 0`, where `training=True` (the reference's default) and `training=False` compute the same thing.
`dropout > 0` with a truthy `training` raises NotImplementedError."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._composite import NativeComposite


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
        compute, max_batch, device, seed, conv_chunk, small_attn = self._pop_extras(kwargs, conv_chunk=0, small_attn=None)
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
        self.image_size, self.patch_size, self.num_classes, self.dim = int(image_size), int(patch_size), int(num_classes), int(dim)
        self.num_hierarchies, self.block_repeats, self.dropout = int(num_hierarchies), tuple(int(r) for r in repeats), float(dropout)
        self.seq_len = (fmap // blocks) ** 2
        self._start(cfg, self._refused_as_value_error(N.nest_param_table, cfg), compute, max_batch, device, seed)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNorm ones / zeros (nest.py:33-34); pos_emb standard normal (nest.py:129)
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("g",), draws={"pos_emb": lambda rng, n: rng.standard_normal(n)})

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """NesT.call(img, training=True) (nest.py:202-216).  img: NHWC numpy or torch of exactly the constructed image_size."""
        if training and self.dropout > 0:
            raise NotImplementedError(f"NesT(dropout={self.dropout}) with training=True needs the Dropout masks of nest.py:68,70,90; they are not "
                                      "built.  Call with training=False, or construct with dropout=0.0 (then training=True is the deterministic path).")
        x, proto = self._nhwc(img)
        b, H, W, _c = x.shape
        if (H, W) != (self.image_size, self.image_size):
            raise ValueError(f"NesT was built for image_size {self.image_size}; got images of {(H, W)} (the positional embeddings and the block "
                             "partition belong to the constructed size)")
        return self._forward(self._ensure_handle(b), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'embedded' [b, f, f, dim], 'level.<i>' [b, f_i, f_i, d_i] (the level's output after
        un-blocking, before aggregation), 'aggregated.<i>' [b, f_i / 2, f_i / 2, d_{i+1}], 'pooled' [b, d_last]."""
        b = self._read_shape()[0]
        fmap = self.image_size // self.patch_size
        out = self._read_raw(which, b * fmap * fmap * self.dim * 2)
        if which == "pooled":
            return out.reshape(b, -1)
        i = 0 if which == "embedded" else int(which.split(".")[1])
        f = (fmap >> i) if not which.startswith("aggregated") else (fmap >> (i + 1))
        return out.reshape(b, f, f, -1)

    apply_gradients = NativeComposite.optimizer_step
