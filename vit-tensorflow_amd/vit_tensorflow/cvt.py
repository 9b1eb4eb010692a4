"""Drop-in for vit_tensorflow/cvt.py: `CvT(...)` (cvt.py:149-202).  The convolutional embeddings, the depthwise-convolution + BatchNormalization
projections, the attention, the MLPs and the head run in HIP behind the C ABI (csrc/cvt.hip, csrc/cvt_ops.hip, the conv_proj block form of
csrc/engine.hip); parameters are in the order of DESIGN.md section 22, with the shapes the reference's variables have (the embedding kernel is
[k, k, in, out], a depthwise kernel [k, k, 1, dim], every 1x1 Conv2D kernel [1, 1, in, out], BatchNormalization's four vectors [dim]).

The reference's constructor takes no image size and no parameter depends on one: the native handle is created at the first call from the
image's H x W, and created again (weights kept) when H x W changes or a larger batch arrives.  `image_size=` (an int or an (H, W) pair)
creates it eagerly.

BatchNormalization (cvt.py:85).  `training=True` -- the reference's default, and what its usage runs -- normalises every projection input with
the mean and the biased variance over all positions of the call's whole batch, forward and backward: the logits of an image depend on the
other images of its batch.  `training=False` normalises with `moving_mean` / `moving_variance` as loaded through `load_state_dict` /
`set_weights`; it is forward only, and a `backward` after it raises NotImplementedError.  NOT BUILT: the library never updates the moving
statistics.  The update rule cannot be pinned here -- TensorFlow 2's fused kernel feeds the Bessel-corrected batch variance into the moving
average, Keras 3 the biased one -- so a training forward leaves them as they are, their gradients are reported as zeros, and
`trainable_variables` / `trainable_weights` leave them out (`weights`, `state_dict`, `save_weights` keep them).

Only the deterministic path exists: `dropout > 0` with a truthy `training` raises NotImplementedError."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._composite import ImageSizedComposite, NativeComposite, _Weight

_STAGE_KEYS = ("emb_dim", "emb_kernel", "emb_stride", "proj_kernel", "kv_proj_stride", "heads", "depth", "mlp_mult")
_MOVING = ("moving_mean", "moving_variance")


class CvT(ImageSizedComposite):
    _PREFIX, _NAME = "vitx_cvt", "CvT"

    def __init__(self, num_classes,
                 s1_emb_dim=64, s1_emb_kernel=7, s1_emb_stride=4, s1_proj_kernel=3, s1_kv_proj_stride=2, s1_heads=1, s1_depth=1, s1_mlp_mult=4,
                 s2_emb_dim=192, s2_emb_kernel=3, s2_emb_stride=2, s2_proj_kernel=3, s2_kv_proj_stride=2, s2_heads=3, s2_depth=2, s2_mlp_mult=4,
                 s3_emb_dim=384, s3_emb_kernel=3, s3_emb_stride=2, s3_proj_kernel=3, s3_kv_proj_stride=2, s3_heads=6, s3_depth=10, s3_mlp_mult=4,
                 dropout=0.0, **kwargs):
        """The reference's arguments (cvt.py:150-177).  Refused with ValueError: compute='bf16' with an emb_dim that is no multiple of 64;
        sizes that are not positive.

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        image_size=int|(H, W) (create the native handle now instead of at the first call), fused_attn=None|True|False (the fused attention
        kernels of the bf16 mode: few-key for at most 64 keys, many-key for 65 .. 320; None: per class, where they measured faster than the
        materialised path -- DESIGN.md section 22; True: wherever they apply; False: nowhere.  More keys -- stage 1 of the usage has 784 --
        and the fp32 / bf16x3 modes run the materialised attention)."""
        compute, max_batch, device, seed, image_size, fused_attn = self._pop_extras(kwargs, image_size=None, fused_attn=None)
        a = dict(locals())
        stages = [tuple(int(a[f"s{i}_{k}"]) for k in _STAGE_KEYS) for i in (1, 2, 3)]
        if compute == "bf16" and any(s[0] % 64 for s in stages):
            raise ValueError("compute='bf16' needs every stage's emb_dim to be a multiple of 64 (use 'fp32' or 'bf16x3' otherwise); got "
                             f"{tuple(s[0] for s in stages)}")
        cfg = N.CvTConfig()
        cfg.num_classes = int(num_classes)
        for i, s in enumerate(stages):
            (cfg.emb_dim[i], cfg.emb_kernel[i], cfg.emb_stride[i], cfg.proj_kernel[i], cfg.kv_proj_stride[i], cfg.heads[i], cfg.depth[i],
             cfg.mlp_mult[i]) = s
        cfg.ln_eps = cfg.bn_eps = 1e-5   # cvt.py:31,85
        cfg.fused_attn = 0 if fused_attn is None else (1 if fused_attn else -1)
        self.num_classes, self.stages, self.dropout = int(num_classes), stages, float(dropout)
        self._last_training = True
        # (no image yet: no parameter depends on one)
        self._start(cfg, self._refused_as_value_error(N.cvt_param_table, cfg), compute, max_batch, device, seed)
        self._eager_handle(image_size, max_batch)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform with the kernel's own fans, zeros; LayerNorm and BatchNormalization ones / zeros,
    # moving statistics 0 / 1
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("g", "gamma", "moving_variance"))

    # ---- the moving statistics are state, not trainable variables
    @property
    def trainable_variables(self):
        return [_Weight(self, n, s, o) for n, s, o in self._table if n.split(".")[-1] not in _MOVING]

    trainable_weights = trainable_variables

    # ---- geometry
    def maps_of(self, H: int, W: int):
        """[((H_s, W_s), (kv H_s, kv W_s))] of the three stages for an H x W image ('SAME': every extent is ceil(in / stride))."""
        out = []
        for d, ek, es, pk, ks, heads, depth, mult in self.stages:
            H, W = -(-H // es), -(-W // es)
            out.append(((H, W), (-(-H // ks), -(-W // ks))))
        return out

    def _check_image(self, H: int, W: int) -> None:
        if H <= 0 or W <= 0:
            raise ValueError("image height and width must be positive")

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """CvT.call(img, training=True) (cvt.py:200-202).  img: NHWC numpy or torch."""
        if training and self.dropout > 0:
            raise NotImplementedError(f"CvT(dropout={self.dropout}) with training=True needs the Dropout masks of cvt.py:70,72,108; they are not "
                                      "built.  Call with training=False, or construct with dropout=0.0 (then training=True is the deterministic "
                                      "path).")
        x, proto = self._nhwc(img)
        h = self._ensure_handle(*x.shape[:3])
        self._last_training = bool(training)
        return self._forward(h, x, proto, 1 if training else 0)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def backward(self, dlogits, want_dimg: bool = False):
        """VJP of the last training forward.  Returns ({name: grad}, dimg | None); the moving statistics' entries are zeros."""
        if self._handle is not None and not self._last_training:
            raise NotImplementedError("CvT: the last forward ran with training=False -- BatchNormalization on the moving statistics is forward "
                                      "only; call with training=True (batch statistics) before backward")
        return super().backward(dlogits, want_dimg)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'embedded.<s>' (stage s's embedding behind its LayerNorm) and 'stage.<s>' (its output),
        [b, H_s, W_s, emb_dim_s]; 'q_in.<s>.<l>' [b, H_s, W_s, emb_dim_s] and 'kv_in.<s>.<l>' [b, kv H_s, kv W_s, emb_dim_s] (the inputs of
        layer l's pointwise projections, behind BatchNormalization); 'pooled' [b, emb_dim_3]."""
        b, H, W, _ = self._read_shape()
        maps = self.maps_of(H, W)
        out = self._read_raw(which, b * max(h * w * s[0] for ((h, w), _kv), s in zip(maps, self.stages)))
        if which == "pooled":
            return out.reshape(b, -1)
        full, kv = maps[int(which.split(".")[1])]
        h, w = kv if which.startswith("kv_in.") else full
        return out.reshape(b, h, w, -1)

    apply_gradients = NativeComposite.optimizer_step
