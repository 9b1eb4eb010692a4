"""Drop-in for vit_tensorflow/twins_svt.py: `TwinsSVT(...)` (twins_svt.py:215-268).  The patch embeddings, the window partition, the local
and global attention pairs, the PEG and the head run in HIP behind the C ABI (csrc/twins.hip, csrc/twins_ops.hip, the global_k block form of
csrc/engine.hip); parameters are in the order of DESIGN.md section 21, with the shapes the reference's variables have (every 1x1 Conv2D
kernel is [1, 1, in, out], to_kv of a global attention [k, k, in, 1024], the PEG kernel [kp, kp, 1, dim]).

The reference's constructor takes no image size and no parameter depends on one: the native handle is created at the first call from the
image's H x W, and created again (weights kept) when H x W changes or a larger batch arrives.  `image_size=` (an int or an (H, W) pair)
creates it eagerly.

Only the deterministic path exists: `dropout == 0`, where `training=True` (the reference's default) and `training=False` compute the same
thing.  `dropout > 0` with a truthy `training` raises NotImplementedError."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._composite import ImageSizedComposite, NativeComposite


class TwinsSVT(ImageSizedComposite):
    _PREFIX, _NAME = "vitx_twins", "TwinsSVT"

    def __init__(self, num_classes,
                 s1_emb_dim=64, s1_patch_size=4, s1_local_patch_size=7, s1_global_k=7, s1_depth=1,
                 s2_emb_dim=128, s2_patch_size=2, s2_local_patch_size=7, s2_global_k=7, s2_depth=1,
                 s3_emb_dim=256, s3_patch_size=2, s3_local_patch_size=7, s3_global_k=7, s3_depth=5,
                 s4_emb_dim=512, s4_patch_size=2, s4_local_patch_size=7, s4_global_k=7, s4_depth=4,
                 peg_kernel_size=3, dropout=0.0, **kwargs):
        """The reference's arguments (twins_svt.py:216-240).  Refused with ValueError, at construction or -- where the image decides -- at the
        call: a map that a stage's patch_size, its local_patch_size (stages 1-3) or its global_k does not divide (the reference's 'valid'
        to_kv convolution silently drops the rows and columns past the last whole window; that is refused, not reproduced); an even
        peg_kernel_size; compute='bf16' with an emb_dim that is no multiple of 64.

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        image_size=int|(H, W) (create the native handle now instead of at the first call), fused_global_attn=None|True|False (the few-key
        attention kernels of the global pairs: bf16 mode, at most 64 keys; None: where they measured faster than the materialised path --
        DESIGN.md section 21; True: wherever they apply; False: nowhere)."""
        compute, max_batch, device, seed, image_size, fused_global_attn = self._pop_extras(kwargs, image_size=None, fused_global_attn=None)
        a = dict(locals())
        stages = [tuple(int(a[f"s{i}_{k}"]) for k in ("emb_dim", "patch_size", "local_patch_size", "global_k", "depth")) for i in (1, 2, 3, 4)]
        if int(peg_kernel_size) <= 0 or int(peg_kernel_size) % 2 == 0:
            raise ValueError(f"peg_kernel_size must be odd, got {peg_kernel_size}: an even 'SAME' kernel pads unevenly and is not built")
        if compute == "bf16" and any(s[0] % 64 for s in stages):
            raise ValueError("compute='bf16' needs every stage's emb_dim to be a multiple of 64 (use 'fp32' or 'bf16x3' otherwise); got "
                             f"{tuple(s[0] for s in stages)}")
        cfg = N.TwinsConfig()
        cfg.num_classes = int(num_classes)
        for i, s in enumerate(stages):
            cfg.emb_dim[i], cfg.patch_size[i], cfg.local_patch_size[i], cfg.global_k[i], cfg.depth[i] = s
        cfg.peg_kernel_size = int(peg_kernel_size)
        cfg.ln_eps = 1e-5   # twins_svt.py:46
        cfg.fused_global_attn = 0 if fused_global_attn is None else (1 if fused_global_attn else -1)
        self.num_classes, self.stages, self.peg_kernel_size, self.dropout = int(num_classes), stages, int(peg_kernel_size), float(dropout)
        # (no image yet: no parameter depends on one)
        self._start(cfg, self._refused_as_value_error(N.twins_param_table, cfg), compute, max_batch, device, seed)
        self._eager_handle(image_size, max_batch)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNorm ones / zeros (twins_svt.py:50-51)
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("g",))

    # ---- geometry
    def maps_of(self, H: int, W: int):
        """[(H_s, W_s)] of the four stages for an H x W image; ValueError where a stage's patch_size, local_patch_size or global_k does not divide."""
        cfg = N.TwinsConfig.from_buffer_copy(self._cfg)
        cfg.image_h, cfg.image_w = int(H), int(W)
        self._refused_as_value_error(N.twins_param_table, cfg)
        out = []
        for d, p, lp, gk, depth in self.stages:
            H, W = H // p, W // p
            out.append((H, W))
        return out

    _check_image = maps_of

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """TwinsSVT.call(x, training=True) (twins_svt.py:266-268).  img: NHWC numpy or torch."""
        if training and self.dropout > 0:
            raise NotImplementedError(f"TwinsSVT(dropout={self.dropout}) with training=True needs the Dropout masks of twins_svt.py:85,87,132,172; "
                                      "they are not built.  Call with training=False, or construct with dropout=0.0 (then training=True is the "
                                      "deterministic path).")
        x, proto = self._nhwc(img)
        return self._forward(self._ensure_handle(*x.shape[:3]), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'embedded.<s>' (stage s's patch embedding), 'pre_peg.<s>' / 'peg.<s>' (in front of / behind
        its PEG), 'stage.<s>' (its output), each [b, H_s, W_s, emb_dim_s]; 'pooled' [b, emb_dim_4]."""
        b, H, W, _ = self._read_shape()
        maps = self.maps_of(H, W)
        out = self._read_raw(which, b * max(h * w * s[0] for (h, w), s in zip(maps, self.stages)))
        if which == "pooled":
            return out.reshape(b, -1)
        h, w = maps[int(which.split(".")[1])]
        return out.reshape(b, h, w, -1)

    apply_gradients = NativeComposite.optimizer_step
