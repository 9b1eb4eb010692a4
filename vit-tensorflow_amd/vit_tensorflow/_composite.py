"""What every model object over a native handle shares: the Keras-like weights surface over one host blob in the C library's table order
(`ParamBlob`), and the Python front of a composite model -- a C-ABI handle that owns its parameter / gradient arenas and drives ViT engines
(`NativeComposite`: CrossViT, CCT).  A new composite starts from here and from csrc/composite.h.  No arithmetic here."""
from __future__ import annotations

import ctypes as C
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
    """Front of `<_PREFIX>_create / _destroy / _backward / ...` over a config in `self._cfg`; `_NAME` is the class name in its refusals.
    A subclass keeps its own __init__, _init_weights, __call__ (which sets `self._img_shape`) and read."""
    _NAME = ""

    # ---- handle management (rebuilt, weights kept, when a larger batch arrives)
    def _ensure_handle(self, batch: int):
        if self._handle is not None and batch <= self._cfg.max_batch:
            return self._handle
        if self._handle is not None:
            self._pull_params()
            N.check(self._native("destroy")(self._handle))
            self._handle = None
        self._cfg.max_batch = max(int(batch), int(self._cfg.max_batch))
        h = C.c_void_p()
        N.check(self._native("create")(C.byref(self._cfg), C.byref(h)))
        self._handle = h
        self._push_params()
        return h

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
