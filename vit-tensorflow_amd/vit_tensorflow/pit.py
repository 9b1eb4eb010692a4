"""Drop-in for vit_tensorflow/pit.py: `PiT(...)` (pit.py:158-219), `Pool(dim)` (:140-156), `conv_output_size`, `cast_tuple`.  The overlapping
tokenizer, the class / position rows, the Transformers, Pool and the head run in HIP behind the C ABI (csrc/pit.hip, csrc/pit_ops.hip, one
ordinary ViT engine per stage); parameters are in the order of DESIGN.md section 27, with the shapes the reference's variables have.

WHAT THE REFERENCE DOES.  pit.py:194 reads `not_last = ind < (len(depth) < 1)`.  `len(depth) < 1` is False, `ind < False` is never true: the
reference's PiT never inserts its Pool and never doubles `dim`.  `PiT.transformer_layers` holds Transformer objects only; the model is a ViT
with overlapping patches and per-stage heads, and `Pool` is a public class nothing in the file calls.  That is what `PiT(...)` is here by
default (`pool_stages=False`).  `pool_stages=True` is the file's evident intent, NOT reference behaviour: the loop body of :196-200 with
`not_last` true -- `Pool(dim)` behind every stage but the last, `dim` doubled there, `mlp_dim` and `dim_head` kept.  It is built from the
reference's own Pool and pinned to it (tools/gen_pit_fixtures.py).

The handle follows the call's H x W (the reference unfolds whatever image it gets and slices pos_embedding, :213): an image that makes more
tokens than pos_embedding has rows is a ValueError, and so is, under pool_stages, a stage whose token map is not square (Pool's rearrange,
:150).  pos_embedding rows an image does not use get zero gradients.

Only the deterministic path exists: `dropout > 0` or `emb_dropout > 0` with a truthy `training` raises NotImplementedError."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from ._composite import ImageSizedComposite, NativeComposite, ParamBlob, as_host, like


def cast_tuple(val, num):
    """pit.py:13-14."""
    return val if isinstance(val, tuple) else (val,) * num


def conv_output_size(image_size, kernel_size, stride, padding=0):
    """pit.py:16-17."""
    return int(((image_size - kernel_size + (2 * padding)) / stride) + 1)


def _normal(rng, n):
    return rng.standard_normal(n)   # tf.random.normal (pit.py:187-188)


class PiT(ImageSizedComposite):
    _PREFIX, _NAME = "vitx_pit", "PiT"

    def __init__(self, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, dim_head=64, dropout=0.0, emb_dropout=0.0, **kwargs):
        """The reference's arguments (pit.py:159-170) and both of its assertions.  `heads` an int or a tuple; zip(depth, heads) stops at the
        shorter.  Refused with ValueError: patch_size // 2 == 0; more than 8 stages; compute='bf16' with a stage width that is no multiple
        of 64; long_attn without compute='bf16' and dim_head=64.

        Engine-only keyword extras: compute='fp32'|'bf16'|'bf16x3', max_batch=int, device=int, seed=int (the initialisers' generator),
        long_attn=None|True|False (the streamed-key attention kernels past 288 tokens, as `ViT(long_attn=)`: bf16, dim_head 64; DESIGN.md
        section 24.  None: the measured default -- on wherever they apply, i.e. compute='bf16' with dim_head=64: at the usage's 962 tokens the
        step is 7.9x faster; True where they do not apply is a ValueError.  The streamed kernels have bounds of their
        own: past 288 tokens a forward with batch * heads > 65535, or n * 3 * heads * 64 >= 2^30, is refused with a VitxError that names
        long_attn, where the materialised path would run -- so the default can refuse; long_attn=False is the way out),
        pool_stages=False (see the module text: True inserts Pool(dim) behind every stage but the last and doubles dim there)."""
        compute, max_batch, device, seed, long_attn, pool_stages = self._pop_extras(kwargs, long_attn=None, pool_stages=False)
        if long_attn is None:
            long_attn = compute == "bf16" and int(dim_head) == 64
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        assert isinstance(depth, tuple), 'depth must be a tuple of integers, specifying the number of blocks before each downsizing'
        heads = cast_tuple(heads, len(depth))
        stages = [(int(d), int(h)) for d, h in zip(depth, heads)]
        if patch_size // 2 == 0:
            raise ValueError(f"patch_size // 2 is the stride of the patch windows (pit.py:180): patch_size={patch_size} makes it 0")
        if not 1 <= len(stages) <= N.PIT_MAX_STAGES:
            raise ValueError(f"zip(depth, heads) must name between 1 and {N.PIT_MAX_STAGES} stages, got {len(stages)}")
        widths = [int(dim) * (2 ** i if pool_stages else 1) for i in range(len(stages))]
        if compute == "bf16" and any(w % 64 for w, (d, _) in zip(widths, stages) if d):
            raise ValueError(f"compute='bf16' needs every stage's width to be a multiple of 64 (use 'fp32' or 'bf16x3' otherwise); got {tuple(widths)}")
        if long_attn and (compute != "bf16" or int(dim_head) != 64):
            raise ValueError("long_attn needs compute='bf16' and dim_head=64 (the streamed-key attention kernels)")
        cfg = N.PiTConfig()
        cfg.image_size, cfg.patch_size, cfg.num_classes, cfg.dim = int(image_size), int(patch_size), int(num_classes), int(dim)
        cfg.n_stages = len(stages)
        for i, (d, h) in enumerate(stages):
            cfg.depth[i], cfg.heads[i] = d, h
        cfg.mlp_dim, cfg.dim_head = int(mlp_dim), int(dim_head)
        cfg.pool_stages, cfg.long_attn = int(bool(pool_stages)), int(bool(long_attn))
        cfg.ln_eps = 1e-3   # Keras LayerNormalization's default
        self.image_size, self.patch_size, self.stride = int(image_size), int(patch_size), int(patch_size) // 2
        self.num_classes, self.dim, self.stages, self.widths = int(num_classes), int(dim), stages, widths
        self.mlp_dim, self.dim_head = int(mlp_dim), int(dim_head)
        self.dropout, self.emb_dropout = float(dropout), float(emb_dropout)
        self.pool_stages, self.long_attn = bool(pool_stages), bool(long_attn)
        self.output_size = conv_output_size(image_size, patch_size, patch_size // 2)
        self._start(cfg, self._refused_as_value_error(N.pit_param_table, cfg), compute, max_batch, device, seed)

    # ---- initialisers: Keras Dense / Conv2D glorot_uniform with the kernel's own fans, zeros; LayerNormalization ones / zeros; pos_embedding
    # and cls_token tf.random.normal
    def _init_weights(self, rng: np.random.Generator) -> None:
        self._fill_blob(rng, ones=("gamma",), draws={"pos_embedding": _normal, "cls_token": _normal})

    # ---- geometry
    def maps_of(self, H: int, W: int):
        """[(h_s, w_s, width_s)] of the stages' token maps for an H x W image; ValueError for an image the model cannot take."""
        cfg = N.PiTConfig.from_buffer_copy(self._cfg)
        cfg.image_h, cfg.image_w = int(H), int(W)
        self._refused_as_value_error(N.pit_param_table, cfg)
        h, w = (H - self.patch_size) // self.stride + 1, (W - self.patch_size) // self.stride + 1
        out = []
        for s, width in enumerate(self.widths):
            out.append((h, w, width))
            if self.pool_stages:
                h, w = -(-h // 2), -(-w // 2)
        return out

    _check_image = maps_of

    # ---- forward
    def __call__(self, img, training=True, **kwargs):
        """PiT.call(img, training=True) (pit.py:207-219).  img: NHWC numpy or torch."""
        if training and (self.dropout > 0 or self.emb_dropout > 0):
            raise NotImplementedError(f"PiT(dropout={self.dropout}, emb_dropout={self.emb_dropout}) with training=True needs the Dropout masks of "
                                      "pit.py:46,48,70,189; they are not built.  Call with training=False, or construct with both rates 0.0 "
                                      "(then training=True is the deterministic path).")
        x, proto = self._nhwc(img)
        return self._forward(self._ensure_handle(*x.shape[:3]), x, proto)

    call = __call__
    predict = lambda self, img, **kw: self(img, training=False, **kw)

    def set_long_attn(self, on: bool) -> None:
        """Switches the streamed-key attention of every stage (between steps).  ValueError where the kernels do not apply."""
        if on and (self.compute != "bf16" or self.dim_head != 64):
            raise ValueError("long_attn needs compute='bf16' and dim_head=64 (the streamed-key attention kernels)")
        self._cfg.long_attn, self.long_attn = int(bool(on)), bool(on)
        if self._handle is not None:
            N.check(self._native("set_long_attn")(self._handle, int(bool(on))))

    def read(self, which: str) -> np.ndarray:
        """Tensors of the last forward for bisecting: 'tokens' [b, n_0, dim] (behind the position rows), 'stage.<s>' [b, n_s, width_s] (the
        stage's output), 'pooled.<s>' [b, n_{s+1}, 2 width_s] (the Pool behind stage s; pool_stages only)."""
        b, H, W, _ = self._read_shape()
        maps = self.maps_of(H, W)
        out = self._read_raw(which, b * max((1 + h * w) * d for h, w, d in maps))
        return out.reshape(b, -1, maps[0 if which == "tokens" else int(which.split(".")[1]) + (which.startswith("pooled."))][2])

    apply_gradients = NativeComposite.optimizer_step


class Pool(ParamBlob):
    """Pool(dim) (pit.py:140-156) alone: callable on tokens [b, 1 + h * h, dim] -> [b, 1 + ceil(h / 2)^2, 2 dim]; `backward(dy)` is the VJP of the
    last call.  Weights, in the reference's attribute order: downsample.dw.{kernel [3, 3, 1, 2 dim], bias}, downsample.pw.{kernel
    [1, 1, 2 dim, 2 dim], bias}, cls_ff.{kernel [dim, 2 dim], bias}.  It runs the Pool kernels of a native PiT handle made of pools alone
    (vitx_pit_pool_forward / _backward), created at the first call and again when a larger map or batch arrives (weights kept).

    Keyword extras: compute='fp32'|'bf16x3'|'bf16' (the two Dense products' mode; storage is fp32 in every mode), max_batch, device, seed."""
    _PREFIX, _NAME = "vitx_pit", "Pool"

    def __init__(self, dim, compute="fp32", max_batch=None, device=0, seed=None):
        assert compute in ("fp32", "bf16", "bf16x3"), "compute must be 'fp32' (parity), 'bf16' (throughput) or 'bf16x3'"
        self.dim, self.compute = int(dim), compute
        self._device, self._max_batch, self._hw_cap = int(device), int(max_batch or 0), 0
        self._handle, self._device_newer = None, False
        mine, off0 = self._pool_entries(self._config(1))[:2]
        self._table = [(n[len("pool.0."):], s, o - off0) for n, s, o in mine]
        self._n = sum(int(np.prod(s)) for _, s, _ in self._table)
        self._blob = np.zeros(self._n, dtype=np.float32)
        rng = np.random.default_rng(seed)
        for name, shape, off in self._table:   # Keras Conv2D / Dense: glorot_uniform with the kernel's own fans, zeros
            if name.endswith("kernel"):
                recv = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
                lim = math.sqrt(6.0 / (recv * shape[-2] + recv * shape[-1]))
                k = int(np.prod(shape))
                self._blob[off:off + k] = rng.uniform(-lim, lim, k).astype(np.float32)

    def _config(self, hw: int):
        """A PiT of two stages without layers around one Pool whose token map is hw x hw: patches of 2 every pixel on an (hw + 1)^2 image."""
        cfg = N.PiTConfig()
        cfg.image_h = cfg.image_w = hw + 1
        cfg.image_size = hw + 1 + (hw + 1) % 2
        cfg.patch_size, cfg.num_classes, cfg.dim, cfg.n_stages = 2, 1, self.dim, 2
        cfg.heads[0] = cfg.heads[1] = 1
        cfg.mlp_dim, cfg.dim_head, cfg.pool_stages, cfg.ln_eps = 1, 1, 1, 1e-3
        cfg.compute = {"fp32": N.COMPUTE_FP32, "bf16": N.COMPUTE_BF16, "bf16x3": N.COMPUTE_BF16X3}[self.compute]
        cfg.max_batch, cfg.device_id = max(1, self._max_batch), self._device
        return cfg

    @staticmethod
    def _pool_entries(cfg):
        """(the Pool's entries of the handle's table, the offset of the first, the table's element count): pos_embedding in front of them
        grows with the map."""
        full, n_full = N.pit_param_table(cfg)
        mine = [(n, s, o) for n, s, o in full if n.startswith("pool.0.")]
        return mine, mine[0][2], n_full

    def _push_params(self):
        if self._handle is not None:
            full = np.zeros(self._n_full, dtype=np.float32)
            full[self._off0:self._off0 + self._n] = self._blob
            N.check(N.lib().vitx_pit_set_params(self._handle, full.ctypes.data_as(C.c_void_p), self._n_full))
        self._device_newer = False

    def _pull_params(self):
        pass   # (nothing on the device changes the weights)

    def _ensure_handle(self, b: int, hw: int):
        if self._handle is not None and b <= self._max_batch and hw <= self._hw_cap:
            return self._handle
        if self._handle is not None:
            N.check(N.lib().vitx_pit_destroy(self._handle))
            self._handle = None
        self._max_batch, self._hw_cap = max(b, self._max_batch), max(hw, self._hw_cap)
        cfg = self._config(self._hw_cap)
        _, self._off0, self._n_full = self._pool_entries(cfg)
        h = C.c_void_p()
        N.check(N.lib().vitx_pit_create(C.byref(cfg), C.byref(h)))
        self._handle = h
        self._push_params()
        return h

    def __call__(self, x, training=True):
        t, proto = as_host(x)
        if t.ndim != 3 or t.shape[2] != self.dim:
            raise ValueError(f"expected tokens [b, 1 + h * h, {self.dim}]")
        b, n, _ = t.shape
        hw = math.isqrt(max(n - 1, 0))
        if n < 2 or hw * hw != n - 1:
            raise ValueError(f"Pool takes a class token and a square map (pit.py:150): {n - 1} tokens are not one")
        no = 1 + (-(-hw // 2)) ** 2
        out = np.empty((b, no, 2 * self.dim), dtype=np.float32)
        N.check(N.lib().vitx_pit_pool_forward(self._ensure_handle(b, hw), 0, t.ctypes.data_as(C.c_void_p), b, n, out.ctypes.data_as(C.c_void_p)))
        self._last = (b, n, no)
        return like(out, proto)

    call = __call__

    def backward(self, dy, want_dx: bool = True):
        """VJP of the last call.  Returns ({name: grad}, dx | None)."""
        if self._handle is None or getattr(self, "_last", None) is None:
            raise N.VitxError(N.ERR_STATE, "backward requires a preceding call")
        d, _ = as_host(dy)
        b, n, no = self._last
        if d.shape != (b, no, 2 * self.dim):
            raise ValueError(f"expected the cotangent of the last call's output, [{b}, {no}, {2 * self.dim}]; got {list(d.shape)}")
        dx = np.empty((b, n, self.dim), dtype=np.float32) if want_dx else None
        N.check(N.lib().vitx_pit_pool_backward(self._handle, 0, d.ctypes.data_as(C.c_void_p), dx.ctypes.data_as(C.c_void_p) if want_dx else None))
        g = np.empty(self._n_full, dtype=np.float32)
        N.check(N.lib().vitx_pit_get_grads(self._handle, g.ctypes.data_as(C.c_void_p), self._n_full))
        g = g[self._off0:self._off0 + self._n]
        return {n_: g[o:o + int(np.prod(s))].reshape(s) for n_, s, o in self._table}, dx
