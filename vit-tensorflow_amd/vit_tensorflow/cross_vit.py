"""Drop-in for vit_tensorflow/cross_vit.py: `CrossViT(...)` with the reference's constructor (cross_vit.py:233-253) and
`__call__(img, training=True)` (cross_vit.py:290-301).  Both encoders' blocks, the final norms, the cross-attention layers and the
heads run in HIP behind the C ABI (csrc/cross_vit.hip); parameters are in the order of DESIGN.md section 7."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._composite import NativeComposite, as_host


class CrossViT(NativeComposite):
    _PREFIX, _NAME = "vitx_crossvit", "CrossViT"

    def __init__(self, image_size, num_classes, sm_dim, lg_dim, sm_patch_size=12, sm_enc_depth=1, sm_enc_heads=8, sm_enc_mlp_dim=2048,
                 sm_enc_dim_head=64, lg_patch_size=16, lg_enc_depth=4, lg_enc_heads=8, lg_enc_mlp_dim=2048, lg_enc_dim_head=64,
                 cross_attn_depth=2, cross_attn_heads=8, cross_attn_dim_head=64, depth=3, dropout=0.1, emb_dropout=0.1,
                 compute="fp32", max_batch=None, device=0, seed=None):
        """Same arguments as the reference.  Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int,
        seed=int (the initialisers' generator)."""
        assert image_size % sm_patch_size == 0, 'Image dimensions must be divisible by the patch size.'   # cross_vit.py:208
        assert image_size % lg_patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        assert compute in ("fp32", "bf16", "bf16x3"), "compute must be 'fp32' (parity), 'bf16' (throughput) or 'bf16x3'"
        cfg = N.CrossViTConfig()
        for k, v in dict(image_size=image_size, num_classes=num_classes, sm_dim=sm_dim, lg_dim=lg_dim, sm_patch_size=sm_patch_size,
                         sm_enc_depth=sm_enc_depth, sm_enc_heads=sm_enc_heads, sm_enc_mlp_dim=sm_enc_mlp_dim, sm_enc_dim_head=sm_enc_dim_head,
                         lg_patch_size=lg_patch_size, lg_enc_depth=lg_enc_depth, lg_enc_heads=lg_enc_heads, lg_enc_mlp_dim=lg_enc_mlp_dim,
                         lg_enc_dim_head=lg_enc_dim_head, cross_attn_depth=cross_attn_depth, cross_attn_heads=cross_attn_heads,
                         cross_attn_dim_head=cross_attn_dim_head, depth=depth).items():
            setattr(cfg, k, int(v))
        cfg.dropout, cfg.emb_dropout = float(dropout), float(emb_dropout)
        cfg.ln_eps = 1e-3   # Keras LayerNormalization default
        self.image_size, self.num_classes = image_size, num_classes
        self.sm_patch_size, self.lg_patch_size = sm_patch_size, lg_patch_size
        self._start(cfg, N.crossvit_param_table(cfg), compute, max_batch, device, seed)

    # ---- initialisers: tf.random.normal (cross_vit.py:216-217), Keras Dense glorot_uniform / zeros, LayerNormalization ones / zeros
    def _init_weights(self, rng: np.random.Generator) -> None:
        normal = lambda rng, n: rng.standard_normal(n)
        self._fill_blob(rng, ones=("gamma",), draws={"pos_embedding": normal, "cls_token": normal})

    # ---- forward
    def __call__(self, img, training=True, seed=None, **_):
        """CrossViT.call(img, training=True) (cross_vit.py:290).  img: NHWC numpy or torch; H and W at most image_size and divisible
        by both patch sizes (the position embeddings are sliced, cross_vit.py:226)."""
        x, proto = as_host(img)
        assert x.ndim == 4 and x.shape[3] == 3, "expected NHWC images [b, H, W, 3]"
        b, H, W, _ = x.shape
        for p in (self.sm_patch_size, self.lg_patch_size):
            assert H % p == 0 and W % p == 0, 'Image dimensions must be divisible by the patch size.'
        seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        return self._forward(self._ensure_handle(b), x, proto, H, W, 1 if training else 0, seed)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'sm_tokens' / 'lg_tokens' [b, n, dim], 'sm_logits' / 'lg_logits' [b, num_classes]."""
        b, H, W, _ = self._read_shape()
        out = self._read_raw(which, b * max(self.num_classes, max((H // p) * (W // p) + 1 for p in (self.sm_patch_size, self.lg_patch_size)) *
                                            max(self._cfg.sm_dim, self._cfg.lg_dim)))
        if which.endswith("_logits"):
            return out.reshape(b, self.num_classes)
        dim = self._cfg.sm_dim if which.startswith("sm") else self._cfg.lg_dim
        return out.reshape(b, -1, dim)
