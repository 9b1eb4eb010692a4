"""Drop-in for vit_tensorflow/vit_for_small_dataset.py: `ViT(...)` (vit_for_small_dataset.py:159-215) -- a ViT whose patch embedding is SPT
(shifted patch tokenization: the image concatenated with its four one-pixel shifts, unfolded, LayerNorm, Dense; :142-157) and whose attention
is LSA (locality self-attention: softmax scale exp(temperature) with a learned per-layer scalar, diagonal masked; :88-121) -- and the
stand-alone `SPT(dim, patch_size)` layer, on the MI355X engine (csrc/spt.hip, csrc/attn_lsa.hip)."""
import ctypes as C

import numpy as np

from ._model import VitxModel, pair  # noqa: F401
from . import _native as N


def _refuse(what):
    def f(self, *a, **k):
        raise NotImplementedError(f"vit_for_small_dataset.ViT: {what}")
    return f


class _NoWrapperSurface:
    """The pieces the MAE / SimMIM / MPP / distillation / efficient wrappers reach into (patch_embedding.layers, transformer, mlp_head).  They
    assume the plain patch Dense and plain attention: refused instead of computing something else."""

    def __init__(self, name):
        self._name = name

    def _fail(self, *a, **k):
        raise NotImplementedError(f"vit_for_small_dataset.ViT.{self._name}: the wrappers (MAE, SimMIM, MPP, distill, efficient) are not supported "
                                  "around this model (SPT / LSA differ from the patch Dense and attention they borrow)")

    __call__ = _fail
    backward = _fail

    def __getattr__(self, item):
        self._fail()


class ViT(VitxModel):
    _variant = N.VARIANT_VIT

    def __init__(self, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, pool='cls', dim_head=64, dropout=0.0, emb_dropout=0.0,
                 **engine_kwargs):
        """Same arguments as the reference (vit_for_small_dataset.py:160-172).  Engine-only keyword extras as for vit.ViT."""
        ph, pw = pair(patch_size)
        assert ph == pw, 'SPT takes one patch_size for both p1 and p2 (vit_for_small_dataset.py:147): the patch must be square'
        self._init_common(image_size=image_size, patch_size=patch_size, num_classes=num_classes, dim=dim, depth=depth, heads=heads,
                          mlp_dim=mlp_dim, pool=pool, dim_head=dim_head, dropout=dropout, emb_dropout=emb_dropout, small_dataset=1,
                          **engine_kwargs)
        self.transformer = _NoWrapperSurface("transformer")
        self.patch_embedding = _NoWrapperSurface("patch_embedding")
        self.mlp_head = _NoWrapperSurface("mlp_head")

    # ---- not provided (and not tested) on this model: refuse instead of misbehaving
    forward_patches = _refuse("forward_patches: the model takes images (SPT shifts the image, not patch rows)")
    comm_init = _refuse("data parallel is not supported")
    apply_gradients = _refuse("no in-library optimizer step")


class SPT:
    """`SPT(dim, patch_size)(img)` (vit_for_small_dataset.py:142-157): [b, H, W, 3] -> [b, (H / p) * (W / p), dim].  Forward only.  Holds
    LayerNorm gamma / beta [5 p p 3] and the Dense kernel / bias; the device plan is built for the first image's size and rebuilt when a
    larger image or batch arrives."""

    def __init__(self, dim, patch_size, compute="fp32", seed=None, channels=3):
        assert isinstance(patch_size, int), 'SPT takes one patch_size for both p1 and p2'
        self.dim, self.patch_size, self.compute, self._channels = int(dim), int(patch_size), compute, int(channels)
        feat = 5 * patch_size * patch_size * channels
        rng = np.random.default_rng(seed)
        lim = np.sqrt(6.0 / (feat + dim))
        self._w = {"norm.gamma": np.ones(feat, np.float32), "norm.beta": np.zeros(feat, np.float32),
                   "kernel": rng.uniform(-lim, lim, (feat, dim)).astype(np.float32), "bias": np.zeros(dim, np.float32)}
        self._model = None

    @property
    def weights(self):
        """[gamma, beta, kernel, bias] in the reference's layer order (LayerNormalization, Dense)."""
        return [self._w[k].copy() for k in ("norm.gamma", "norm.beta", "kernel", "bias")]

    def get_weights(self):
        return self.weights

    def set_weights(self, weights):
        for k, a in zip(("norm.gamma", "norm.beta", "kernel", "bias"), weights):
            a = np.asarray(a, np.float32)
            assert a.shape == self._w[k].shape, f"{k}: expected shape {self._w[k].shape}, got {a.shape}"
            self._w[k] = a.copy()
        if self._model is not None:
            self._load()

    def _load(self):
        sd = self._model.state_dict()
        for k, a in self._w.items():
            sd["patch_embedding." + k] = a
        self._model.load_state_dict(sd)

    def __call__(self, img, training=True, **_):
        x, proto = VitxModel._as_host(img)
        assert x.ndim == 4 and x.shape[3] == self._channels, "expected NHWC images [b, H, W, C]"
        b, H, W, _c = x.shape
        p = self.patch_size
        assert H % p == 0 and W % p == 0, 'Image dimensions must be divisible by the patch size.'
        m = self._model
        if m is None or H > m._cfg.image_h or W > m._cfg.image_w:
            ih, iw = (H, W) if m is None else (max(H, m._cfg.image_h), max(W, m._cfg.image_w))
            # a depth-0 handle: only its tokenizer is used
            m = self._model = ViT(image_size=(ih, iw), patch_size=p, num_classes=1, dim=self.dim, depth=0, heads=1, mlp_dim=self.dim,
                                  dim_head=64, compute=self.compute, channels=self._channels, seed=0)
            self._load()
        h = m._ensure_handle(b)
        out = np.empty((b, (H // p) * (W // p), self.dim), dtype=np.float32)
        N.check(N.lib().vitx_spt_forward(h, x.ctypes.data_as(C.c_void_p), b, H, W, out.ctypes.data_as(C.c_void_p)))
        return VitxModel._like(out, proto)

    call = __call__
