"""What every model object over a native handle shares: the Keras-like weights surface over one host blob in the C library's table order
(`ParamBlob`: every model, MIM and distill among them), and the Python front of a composite model created from a config -- a C-ABI handle
that owns its parameter / gradient arenas and drives ViT engines (`NativeComposite`: CrossViT, CCT, NesT; `ImageSizedComposite`: TwinsSVT,
CvT, CrossFormer).  NativeComposite holds the keyword extras, the seeded Keras initialisers, handle management, the forward / backward / read calls, the
profiler and the refusals.  A new composite starts from here and from csrc/composite.h.  No arithmetic here."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Sequence

import numpy as np

from . import _native as N


def as_host(x):
    """(contiguous fp32 numpy array, the torch tensor it came from | None): numpy, torch (CPU or ROCm) in -- TensorFlow is what the
    reference used (vit.py:193)."""
    if type(x).__module__.startswith("torch"):
        return np.ascontiguousarray(x.detach().to("cpu").float().numpy()), x
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)), None


def like(out: np.ndarray, proto):
    if proto is None:
        return out
    import torch
    return torch.from_numpy(out).to(proto.device)


class _Weight:
    """Minimal stand-in for a tf.Variable: `.name`, `.shape`, `.numpy()`, `.assign()`."""

    def __init__(self, owner: "ParamBlob", name: str, shape, offset: int):
        self._owner, self.name, self.shape, self._offset = owner, name, tuple(shape), offset

    def numpy(self) -> np.ndarray:
        self._owner._pull_params()
        n = int(np.prod(self.shape))
        return self._owner._blob[self._offset:self._offset + n].reshape(self.shape).copy()

    def assign(self, value) -> None:
        v = np.asarray(value, dtype=np.float32)
        assert v.shape == self.shape, f"shape mismatch for {self.name}: {v.shape} vs {self.shape}"
        self._owner._pull_params()
        self._owner._blob[self._offset:self._offset + v.size] = v.reshape(-1)
        self._owner._push_params()

    def __array__(self, dtype=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None else a

    def __getitem__(self, idx):
        """`encoder.pos_embedding[:, 1:(num_patches + 1)]` (mae.py:54, simmim.py:95, distill.py:24)."""
        return self.numpy()[idx]


class ParamBlob:
    """Weights surface over `self._table` [(name, shape, offset)], `self._n`, `self._blob` (host copy) and `self._device_newer`.  The native
    handle sits in the attribute named `_HANDLE`; `<_PREFIX>_set_params / _get_params / _destroy` are its C functions."""
    _HANDLE, _PREFIX = "_handle", "vitx"

    def _native(self, op: str):
        return getattr(N.lib(), f"{self._PREFIX}_{op}")

    def _push_params(self):
        h = getattr(self, self._HANDLE)
        if h is not None:
            N.check(self._native("set_params")(h, self._blob.ctypes.data_as(C.c_void_p), self._n))
        self._device_newer = False

    def _pull_params(self):
        h = getattr(self, self._HANDLE)
        if h is not None and self._device_newer:
            N.check(self._native("get_params")(h, self._blob.ctypes.data_as(C.c_void_p), self._n))
            self._device_newer = False

    def _owns_handle(self) -> bool:
        return True

    def __del__(self):
        try:
            h = getattr(self, self._HANDLE, None)
            if h is not None and self._owns_handle():
                self._native("destroy")(h)
                setattr(self, self._HANDLE, None)
        except Exception:
            pass

    @property
    def weights(self) -> List[_Weight]:
        return [_Weight(self, n, s, o) for n, s, o in self._table]

    trainable_variables = weights
    trainable_weights = weights

    def get_weights(self) -> List[np.ndarray]:
        self._pull_params()
        return [self._blob[o:o + int(np.prod(s))].reshape(s).copy() for _, s, o in self._table]

    @staticmethod
    def _shape_ok(got, want) -> bool:
        return tuple(got) == tuple(want)

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        assert len(weights) == len(self._table), f"expected {len(self._table)} arrays, got {len(weights)}"
        for w, (n, s, o) in zip(weights, self._table):
            a = np.asarray(w, dtype=np.float32)
            assert self._shape_ok(a.shape, s), f"{n}: expected shape {tuple(s)}, got {a.shape}"
            self._blob[o:o + a.size] = a.reshape(-1)
        self._push_params()

    def state_dict(self) -> Dict[str, np.ndarray]:
        return {n: w for (n, _, _), w in zip(self._table, self.get_weights())}

    def load_state_dict(self, sd: Dict[str, np.ndarray]) -> None:
        self.set_weights([sd[n] for n, _, _ in self._table])

    def count_params(self) -> int:
        return int(self._n)

    @staticmethod
    def _npz_path(path: str) -> str:
        path = str(path)
        return path if path.endswith(".npz") else path + ".npz"    # np.savez appends the suffix: both directions agree on the name

    def save_weights(self, path: str) -> None:
        """Weights by table name in one .npz."""
        np.savez(self._npz_path(path), **self.state_dict())

    def load_weights(self, path: str) -> None:
        with np.load(self._npz_path(path)) as z:
            self.load_state_dict({k: z[k] for k in z.files})


class NativeComposite(ParamBlob):
    """Front of `<_PREFIX>_create / _destroy / _forward / _backward / _read / _profile_* ...` over a config in `self._cfg`; `_NAME` is the
    class name in its refusals.  A subclass keeps its own __init__ (built from `_pop_extras` and `_start`), the leaves its `_init_weights`
    hands to `_fill_blob`, its __call__ (over `_nhwc` and `_forward`) and its read (over `_read_raw`)."""
    _NAME = ""

    # ---- construction
    @classmethod
    def _pop_extras(cls, kwargs: dict, strict: bool = True, **own):
        """[compute, max_batch, device, seed, *own] popped from a constructor's **kwargs (`own`: the model's extras with their defaults).
        strict: anything left over is an unexpected keyword."""
        vals = [kwargs.pop(k, v) for k, v in dict(compute="fp32", max_batch=None, device=0, seed=None, **own).items()]
        if strict and kwargs:
            raise TypeError(f"{cls._NAME}() got an unexpected keyword argument '{next(iter(kwargs))}'")
        assert vals[0] in ("fp32", "bf16", "bf16x3"), "compute must be 'fp32' (parity), 'bf16' (throughput) or 'bf16x3'"
        return vals

    @staticmethod
    def _refused_as_value_error(table_fn, cfg):
        """table_fn(cfg), a refused configuration raised as ValueError."""
        try:
            return table_fn(cfg)
        except N.VitxError as e:
            raise ValueError(e.message) from None

    def _start(self, cfg, table, compute, max_batch, device, seed):
        """The end of every constructor: the engine fields of cfg, no handle yet, the host blob over `table` filled by the seeded initialisers."""
        cfg.compute = {"fp32": N.COMPUTE_FP32, "bf16": N.COMPUTE_BF16, "bf16x3": N.COMPUTE_BF16X3}[compute]
        cfg.max_batch = int(max_batch or 0)
        cfg.device_id = int(device)
        self._cfg, self.compute, self._handle = cfg, compute, None
        self._table, self._n = table
        self._blob = np.zeros(self._n, dtype=np.float32)
        self._device_newer = False
        self._init_weights(np.random.default_rng(seed))

    def _fill_blob(self, rng: np.random.Generator, ones=(), draws={}) -> None:
        """Keras initialisers in table order: a leaf named `kernel` glorot-uniform with the kernel's own fans (Conv2D / Dense), a leaf in `ones`
        ones, a leaf in `draws` ({leaf: fn(rng, n)}) what fn draws, everything else zeros."""
        for name, shape, off in self._table:
            n = int(np.prod(shape))
            leaf = name.split(".")[-1]
            if leaf in draws:
                v = draws[leaf](rng, n)
            elif leaf == "kernel":
                recv = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
                lim = math.sqrt(6.0 / (recv * shape[-2] + recv * shape[-1]))
                v = rng.uniform(-lim, lim, n)
            elif leaf in ones:
                v = np.ones(n)
            else:
                v = np.zeros(n)
            self._blob[off:off + n] = v.astype(np.float32)

    # ---- handle management (rebuilt, weights kept, when a larger batch arrives)
    def _ensure_handle(self, batch: int):
        if self._handle is not None and batch <= self._cfg.max_batch:
            return self._handle
        self._drop_handle()
        self._cfg.max_batch = max(int(batch), int(self._cfg.max_batch))
        h = C.c_void_p()
        N.check(self._native("create")(C.byref(self._cfg), C.byref(h)))
        self._handle = h
        self._push_params()
        return h

    def _drop_handle(self):
        if self._handle is not None:
            self._pull_params()
            N.check(self._native("destroy")(self._handle))
            self._handle = None

    # ---- forward / read / profile
    @staticmethod
    def _nhwc(img, channels: int = 3):
        """(host images [b, H, W, channels], the torch tensor they came from | None)"""
        x, proto = as_host(img)
        if x.ndim != 4 or x.shape[3] != channels:
            raise ValueError(f"expected NHWC images [b, H, W, {channels}]")
        return x, proto

    def _forward(self, h, x: np.ndarray, proto, *extra):
        """<_PREFIX>_forward(h, x, b, *extra, logits) on host images x: the logits [b, num_classes], as what the images came as."""
        self._img_shape = tuple(int(s) for s in x.shape)
        out = np.empty((x.shape[0], self.num_classes), dtype=np.float32)
        N.check(self._native("forward")(h, x.ctypes.data_as(C.c_void_p), x.shape[0], *extra, out.ctypes.data_as(C.c_void_p)))
        return like(out, proto)

    def _read_shape(self):
        """(b, H, W, c) of the last forward's images: where every read starts."""
        if self._handle is None:
            raise N.VitxError(N.ERR_STATE, "read requires a preceding forward")
        return self._img_shape

    def _read_raw(self, which: str, cap: int) -> np.ndarray:
        """<_PREFIX>_read of the last forward's tensor `which` through a buffer of `cap` floats: its elements, flat."""
        buf, n = np.empty(cap, dtype=np.float32), C.c_int64()
        N.check(self._native("read")(self._handle, which.encode(), buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return buf[:n.value]

    def profile(self, fn):
        """Runs fn() between <_PREFIX>_profile_begin / _end: {class: (launches, total_ms)}."""
        try:
            begin, end = self._native("profile_begin"), self._native("profile_end")
        except AttributeError:
            raise NotImplementedError(f"{self._NAME}: the profiler is not supported (the library has no {self._PREFIX}_profile_begin / _end)") from None
        h = self._ensure_handle(1)
        N.check(begin(h))
        try:
            fn()
        finally:
            stats, n = (N.KernelStat * 256)(), C.c_int32()
            N.check(end(h, stats, 256, C.byref(n)))
        return {stats[i].name.decode(): (int(stats[i].launches), float(stats[i].total_ms)) for i in range(min(n.value, 256))}

    def params_changed(self):
        """The device parameter arena (params_dev) was written by an optimizer outside the library."""
        if self._handle is not None:
            N.check(self._native("params_changed")(self._handle))
            self._device_newer = True

    def _arena(self, which: str):
        p, n = C.c_void_p(), C.c_int64()
        N.check(self._native(which)(self._ensure_handle(1), C.byref(p), C.byref(n)))
        return p.value, n.value

    def params_dev(self):
        """(device pointer, elements) of the fp32 parameter arena (table order, every tensor 16-B aligned)."""
        return self._arena("params_dev")

    def grads_dev(self):
        return self._arena("grads_dev")

    def backward(self, dlogits, want_dimg: bool = False):
        """VJP of the last forward.  Returns ({name: grad}, dimg | None)."""
        if self._handle is None:
            raise N.VitxError(N.ERR_STATE, "backward requires a preceding forward")
        d, _ = as_host(dlogits)
        dimg = np.empty(self._img_shape, dtype=np.float32) if want_dimg else None
        N.check(self._native("backward")(self._handle, d.ctypes.data_as(C.c_void_p), dimg.ctypes.data_as(C.c_void_p) if want_dimg else None))
        g = np.empty(self._n, dtype=np.float32)
        N.check(self._native("get_grads")(self._handle, g.ctypes.data_as(C.c_void_p), self._n))
        return {n: g[o:o + int(np.prod(s))].reshape(s) for n, s, o in self._table}, dimg

    # ---- not provided for a composite: refuse instead of misbehaving
    def comm_init(self, *a, **k):
        raise NotImplementedError(f"{self._NAME}: data parallel is not supported (all-reduce grads_dev() outside the library)")

    def optimizer_step(self, *a, **k):
        raise NotImplementedError(f"{self._NAME}: no in-library optimizer step (update params_dev() outside the library, then params_changed())")

    def capture_graph(self, *a, **k):
        raise NotImplementedError(f"{self._NAME}: HIP graph capture is not supported")


class ImageSizedComposite(NativeComposite):
    """A composite whose reference constructor takes no image size and none of whose parameters depends on one (TwinsSVT, CvT, CrossFormer): the handle is
    created at the first call from the image's H x W (cfg.image_h / image_w), and again, weights kept, when H x W changes or a larger batch
    arrives.  `_check_image(H, W)` raises ValueError for a size the model cannot take."""

    def _check_image(self, H: int, W: int) -> None:
        raise NotImplementedError

    def _eager_handle(self, image_size, max_batch) -> None:
        """The constructor's `image_size=int|(H, W)` extra: create the handle now."""
        if image_size is not None:
            H, W = (image_size, image_size) if isinstance(image_size, int) else image_size
            self._ensure_handle(max(1, int(max_batch or 1)), int(H), int(W))

    def _ensure_handle(self, batch: int, H: int | None = None, W: int | None = None):
        if H is None:
            H, W = int(self._cfg.image_h), int(self._cfg.image_w)
            if H == 0:
                raise N.VitxError(N.ERR_STATE, f"{self._NAME} has no native handle before its first call (pass image_size= to create it eagerly)")
        if self._handle is None or (H, W) != (self._cfg.image_h, self._cfg.image_w):
            self._check_image(H, W)
            self._drop_handle()
            self._cfg.image_h, self._cfg.image_w = int(H), int(W)
        return super()._ensure_handle(batch)
