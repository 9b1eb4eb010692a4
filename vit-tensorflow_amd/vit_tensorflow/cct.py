"""Drop-in for vit_tensorflow/cct.py: `CCT(...)` (cct.py:307-345) and the factories `cct_2 ... cct_16` (cct.py:16-61).  The convolutional
tokenizer (Conv2D 'SAME' without bias, ReLU, MaxPool2D 'SAME'), the encoder blocks in the CCT form (the MLP residual leaves from the
normalised stream, cct.py:165-172), the final norm, sequence pooling and fc run in HIP behind the C ABI (csrc/cct.hip, csrc/cct_tok.hip);
parameters are in the order of DESIGN.md section 18.

Only the deterministic path exists: `CCT.__call__(img, training=None)` with `training` falsy, which is what the reference computes there
(Keras hands `training` down to every nested layer, so neither the attention dropout at 0.1 nor the stochastic depth at 0.1 that CCT
hard-wires is active).  `training=True` needs both and raises NotImplementedError."""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._composite import NativeComposite


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


# Pre-defined CCT Models
__all__ = ['cct_2', 'cct_4', 'cct_6', 'cct_7', 'cct_8', 'cct_14', 'cct_16']


def cct_2(*args, **kwargs):
    return _cct(num_layers=2, num_heads=2, mlp_ratio=1, embedding_dim=128, *args, **kwargs)


def cct_4(*args, **kwargs):
    return _cct(num_layers=4, num_heads=2, mlp_ratio=1, embedding_dim=128, *args, **kwargs)


def cct_6(*args, **kwargs):
    return _cct(num_layers=6, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_7(*args, **kwargs):
    return _cct(num_layers=7, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_8(*args, **kwargs):
    return _cct(num_layers=8, num_heads=4, mlp_ratio=2, embedding_dim=256, *args, **kwargs)


def cct_14(*args, **kwargs):
    return _cct(num_layers=14, num_heads=6, mlp_ratio=3, embedding_dim=384, *args, **kwargs)


def cct_16(*args, **kwargs):
    return _cct(num_layers=16, num_heads=6, mlp_ratio=3, embedding_dim=384, *args, **kwargs)


def _cct(num_layers, num_heads, mlp_ratio, embedding_dim, kernel_size=3, stride=None, *args, **kwargs):
    stride = stride if stride is not None else max(1, (kernel_size // 2) - 1)   # cct.py:54
    return CCT(num_layers=num_layers, num_heads=num_heads, mlp_ratio=mlp_ratio, embedding_dim=embedding_dim, kernel_size=kernel_size,
               stride=stride, *args, **kwargs)


def same_out(extent: int, stride: int) -> int:
    """Output extent of a 'SAME' convolution / pooling: ceil(extent / stride)."""
    return -(-int(extent) // int(stride))


def sequence_length(img_size, n_conv_layers=1, stride=2, pooling_stride=2) -> int:
    """Tokenizer.sequence_length (cct.py:204-209) from the 'SAME' geometry instead of a run on zeros."""
    h, w = pair(img_size)
    for _ in range(n_conv_layers):
        h, w = same_out(same_out(h, stride), pooling_stride), same_out(same_out(w, stride), pooling_stride)
    return h * w


class CCT(NativeComposite):
    _PREFIX, _NAME = "vitx_cct", "CCT"

    def __init__(self, img_size=224, embedding_dim=768, n_input_channels=3, n_conv_layers=1, kernel_size=7, stride=2, pooling_kernel_size=3,
                 pooling_stride=2, *args, **kwargs):
        """Same arguments as the reference: the eight above (cct.py:308-317) and, through **kwargs, TransformerClassifier's num_layers=12,
        num_heads=12, mlp_ratio=4.0, num_classes=1000, positional_embedding='sine' (cct.py:217-230).  As in the reference, dropout_rate,
        attention_dropout and stochastic_depth_rate are hard-wired (0, 0.1, 0.1: passing one of the last two raises TypeError, cct.py:336-338),
        and unknown keywords (`padding`, `pooling_padding`, the usage example's `mlp_radio`) are swallowed.

        positional_embedding='sine' is the reference's default, and the reference cannot run it: sinusoidal_embedding assigns into a tensor
        (cct.py:271-272) and raises.  Here it is the table evidently meant -- p / 10000^(2 (i // 2) / dim), sin on even and cos on odd columns --
        as a constant that is not part of the weights.

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        conv_chunk=int (images per im2col pass of the tokenizer; default: sized from a fixed workspace)."""
        compute, max_batch, device, seed, conv_chunk = self._pop_extras(kwargs, strict=False, conv_chunk=0)   # (the rest: _classifier_kwargs)
        if args:   # cct.py:330-339 passes them behind its own keywords: the first one lands on seq_pool
            raise TypeError("TransformerClassifier() got multiple values for argument 'seq_pool'")
        cls_kw = self._classifier_kwargs(**kwargs)
        pe = cls_kw["positional_embedding"]
        pe = pe if pe in ('sine', 'learnable', 'none') else 'sine'   # cct.py:233-234
        img_height, img_width = pair(img_size)
        cfg = N.CCTConfig()
        for k, v in dict(img_height=img_height, img_width=img_width, n_input_channels=n_input_channels, embedding_dim=embedding_dim,
                         n_conv_layers=n_conv_layers, kernel_size=kernel_size, stride=stride, pooling_kernel_size=pooling_kernel_size,
                         pooling_stride=pooling_stride, num_layers=cls_kw["num_layers"], num_heads=cls_kw["num_heads"],
                         dim_feedforward=int(embedding_dim * cls_kw["mlp_ratio"]), num_classes=cls_kw["num_classes"],
                         positional_embedding=N.CCT_POS[pe], in_planes=64, conv_chunk=conv_chunk).items():
            setattr(cfg, k, int(v))
        cfg.ln_eps = 1e-3   # Keras LayerNormalization default
        self.img_size = (int(img_height), int(img_width))
        self.n_input_channels = int(n_input_channels)
        self.num_classes = int(cls_kw["num_classes"])
        self.positional_embedding = pe
        self.embedding_dim = int(embedding_dim)
        table = N.cct_param_table(cfg)
        self.sequence_length = N.cct_sequence_length(cfg)
        self._start(cfg, table, compute, max_batch, device, seed)

    @staticmethod
    def _classifier_kwargs(num_layers=12, num_heads=12, mlp_ratio=4.0, num_classes=1000, positional_embedding='sine', **swallowed):
        """What reaches TransformerClassifier.__init__ (cct.py:330-339): CCT passes sequence_length, embedding_dim, seq_pool, dropout_rate,
        attention_dropout and stochastic_depth_rate itself, so a caller's copy of one of them is a duplicate keyword there."""
        for k in ("seq_pool", "dropout_rate", "attention_dropout", "stochastic_depth_rate", "sequence_length"):
            if k in swallowed:
                raise TypeError(f"TransformerClassifier() got multiple values for keyword argument '{k}'")
        return dict(num_layers=num_layers, num_heads=num_heads, mlp_ratio=mlp_ratio, num_classes=num_classes,
                    positional_embedding=positional_embedding)

    # ---- initialisers: Keras Conv2D / Dense glorot_uniform, zeros; LayerNormalization ones / zeros; truncated normal, stddev 0.2 (cct.py:252)
    def _init_weights(self, rng: np.random.Generator) -> None:
        def truncated_normal(rng, n):
            v = rng.standard_normal(n)
            bad = np.abs(v) > 2.0
            while bad.any():   # tf.random.truncated_normal: values beyond two standard deviations are redrawn
                v[bad] = rng.standard_normal(int(bad.sum()))
                bad = np.abs(v) > 2.0
            return 0.2 * v
        self._fill_blob(rng, ones=("gamma",), draws={"positional_emb": truncated_normal})

    # ---- forward
    def __call__(self, img, training=None, **kwargs):
        """CCT.call(img, training=None) (cct.py:342-345).  img: NHWC numpy or torch of exactly the constructed img_size."""
        if training:
            raise NotImplementedError("CCT(training=True) needs dropout on the attention probabilities (rate 0.1, cct.py:132) and per-sample "
                                      "stochastic depth (rates up to 0.1, cct.py:74-91,161,170); neither is built.  Only the deterministic path "
                                      "(training falsy) is supported.")
        x, proto = self._nhwc(img, self.n_input_channels)
        b, H, W, _c = x.shape
        if (H, W) != self.img_size:
            raise ValueError(f"CCT was built for img_size {self.img_size}; got images of {(H, W)} (the positional embedding and the sequence "
                             "length belong to the constructed size)")
        return self._forward(self._ensure_handle(b), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'tokens' / 'encoded' [b, n, dim], 'pool_weights' [b, n], 'pooled' [b, dim]."""
        b = self._read_shape()[0]
        out = self._read_raw(which, b * self.sequence_length * self.embedding_dim)
        return out.reshape(b, -1, self.embedding_dim) if which in ("tokens", "encoded") else out.reshape(b, -1)

    apply_gradients = NativeComposite.optimizer_step
