"""The weights surface every model object shares (vit_tensorflow/_composite.py: ParamBlob), checked once for every class that can be
constructed without a device: ViT (the engine's table), CrossViT and CCT (composites).  Host-only: no handle is ever created."""
import numpy as np
import pytest

from vit_tensorflow import ViT
from vit_tensorflow import _native as N
from vit_tensorflow._composite import NativeComposite, ParamBlob
from vit_tensorflow._model import _Weight
from vit_tensorflow.cct import CCT
from vit_tensorflow.cross_vit import CrossViT

MAKE = {
    "ViT": lambda seed: ViT(image_size=32, patch_size=8, num_classes=5, dim=16, depth=2, heads=2, mlp_dim=24, dim_head=8, seed=seed),
    "CrossViT": lambda seed: CrossViT(image_size=32, num_classes=5, sm_dim=16, lg_dim=24, sm_patch_size=8, sm_enc_depth=1, sm_enc_heads=2,
                                      sm_enc_mlp_dim=24, sm_enc_dim_head=8, lg_patch_size=16, lg_enc_depth=1, lg_enc_heads=2, lg_enc_mlp_dim=24,
                                      lg_enc_dim_head=8, cross_attn_depth=1, cross_attn_heads=2, cross_attn_dim_head=8, depth=1, seed=seed),
    "CCT": lambda seed: CCT(img_size=16, embedding_dim=16, n_conv_layers=1, kernel_size=3, stride=1, pooling_kernel_size=3, pooling_stride=2,
                            num_layers=1, num_heads=2, mlp_ratio=1.0, num_classes=5, positional_embedding='learnable', seed=seed),
}
CLASSES = list(MAKE)


@pytest.fixture(scope="module")
def models():
    return {k: (MAKE[k](1), MAKE[k](2)) for k in CLASSES}


@pytest.mark.parametrize("cls", CLASSES)
def test_every_class_shares_the_one_surface(cls, models):
    m = models[cls][0]
    assert isinstance(m, ParamBlob) and isinstance(m, NativeComposite) == (cls != "ViT")
    for name in ("get_weights", "set_weights", "state_dict", "load_state_dict", "count_params", "_push_params", "_pull_params"):
        assert getattr(type(m), name) is getattr(ParamBlob, name), name
    assert m._handle is None


@pytest.mark.parametrize("cls", CLASSES)
def test_count_params_is_the_table_sum(cls, models):
    m = models[cls][0]
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in m._table) == m._blob.size
    assert [o for _, _, o in m._table] == list(np.cumsum([0] + [int(np.prod(s)) for _, s, _ in m._table[:-1]]))


@pytest.mark.parametrize("cls", CLASSES)
def test_get_set_state_dict_round_trip(cls, models):
    a, b = MAKE[cls](1), models[cls][1]
    ws = a.get_weights()
    assert [w.shape for w in ws] == [tuple(s) for _, s, _ in a._table] and all(w.dtype == np.float32 for w in ws)
    assert any(not np.array_equal(x, y) for x, y in zip(ws, b.get_weights()))     # the two seeds differ
    sd = b.state_dict()
    assert list(sd) == [n for n, _, _ in b._table] == [w.name for w in b.weights]
    assert len(a.trainable_variables) == len(a.trainable_weights) == len(a.weights) == len(ws)
    a.load_state_dict(sd)
    for x, y in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(x, y)
    a.set_weights(ws)
    for x, y in zip(a.get_weights(), ws):
        assert np.array_equal(x, y)
    ws[0][...] = 7.0                                                               # get_weights hands out copies
    assert not np.any(a.get_weights()[0] == 7.0)


@pytest.mark.parametrize("cls", CLASSES)
def test_save_load_weights_round_trip(cls, models, tmp_path):
    src, dst = models[cls][1], MAKE[cls](3)
    src.save_weights(str(tmp_path / "w"))                 # the suffix is appended on both sides
    assert (tmp_path / "w.npz").exists()
    with np.load(str(tmp_path / "w.npz")) as z:
        assert sorted(z.files) == sorted(n for n, _, _ in src._table)
    dst.load_weights(str(tmp_path / "w"))
    for x, y in zip(src.get_weights(), dst.get_weights()):
        assert np.array_equal(x, y)
    dst2 = MAKE[cls](4)
    dst2.load_weights(str(tmp_path / "w.npz"))
    assert all(np.array_equal(x, y) for x, y in zip(src.get_weights(), dst2.get_weights()))


def test_vit_keeps_the_keras_list_form(tmp_path):
    src, dst = MAKE["ViT"](5), MAKE["ViT"](6)
    src.save_weights(str(tmp_path / "k"), format="keras_list")
    with np.load(str(tmp_path / "k.npz")) as z:
        assert sorted(z.files) == sorted(f"arr_{i}" for i in range(len(src._table)))
    dst.load_weights(str(tmp_path / "k"))
    assert all(np.array_equal(x, y) for x, y in zip(src.get_weights(), dst.get_weights()))
    with pytest.raises(ValueError, match="format must be 'named' or 'keras_list'"):
        src.save_weights(str(tmp_path / "x"), format="h5")


@pytest.mark.parametrize("cls", CLASSES)
def test_weight_assign_and_read(cls):
    m = MAKE[cls](1)
    w = m.weights[-1]
    assert isinstance(w, _Weight) and w.name == m._table[-1][0] and w.shape == tuple(m._table[-1][1])
    v = np.arange(int(np.prod(w.shape)), dtype=np.float32).reshape(w.shape) + 1.0
    w.assign(v)
    assert np.array_equal(w.numpy(), v) and np.array_equal(np.asarray(w), v) and np.array_equal(w[...], v)
    assert np.array_equal(m.state_dict()[w.name], v) and np.array_equal(m._blob[w._offset:], v.reshape(-1))
    before = m.get_weights()
    with pytest.raises(AssertionError, match=f"shape mismatch for {w.name}"):
        w.assign(np.zeros(w.shape + (1,), np.float32))
    assert all(np.array_equal(x, y) for x, y in zip(before, m.get_weights()))


@pytest.mark.parametrize("cls", CLASSES)
def test_wrong_count_and_wrong_shape_are_rejected(cls):
    m = MAKE[cls](1)
    ws = m.get_weights()
    with pytest.raises(AssertionError, match=f"expected {len(ws)} arrays, got {len(ws) - 1}"):
        m.set_weights(ws[:-1])
    name, shape, _ = m._table[0]
    bad = list(ws)
    bad[0] = np.zeros(tuple(shape) + (1,), np.float32)     # a singleton axis more: only the MIM wrappers' hook lets that pass
    with pytest.raises(AssertionError) as e:
        m.set_weights(bad)
    assert str(e.value) == f"{name}: expected shape {tuple(shape)}, got {bad[0].shape}"
    sd = m.state_dict()
    del sd[m._table[-1][0]]
    with pytest.raises(KeyError):
        m.load_state_dict(sd)


@pytest.mark.parametrize("cls,prefix", [("CrossViT", "vitx_crossvit"), ("CCT", "vitx_cct")])
def test_composite_refusals_and_native_names(cls, prefix):
    m = MAKE[cls](1)
    assert (m._PREFIX, m._NAME) == (prefix, cls)
    for op in ("create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev", "params_changed", "backward"):
        assert m._native(op) is getattr(N.lib(), f"{prefix}_{op}")
    with pytest.raises(NotImplementedError) as e:
        m.comm_init()
    assert str(e.value) == f"{cls}: data parallel is not supported (all-reduce grads_dev() outside the library)"
    with pytest.raises(NotImplementedError) as e:
        m.optimizer_step()
    assert str(e.value) == f"{cls}: no in-library optimizer step (update params_dev() outside the library, then params_changed())"
    with pytest.raises(NotImplementedError) as e:
        m.capture_graph()
    assert str(e.value) == f"{cls}: HIP graph capture is not supported"
    assert hasattr(m, "apply_gradients") == (cls == "CCT")
    with pytest.raises(N.VitxError, match="backward requires a preceding forward"):
        m.backward(np.zeros((1, 5), np.float32))
    m.params_changed()                                     # no handle yet: nothing to tell
    assert m._handle is None and not m._device_newer


def test_table_of_is_the_one_loop():
    cfg = MAKE["CCT"](0)._cfg
    assert N.cct_param_table(cfg) == N.table_of("vitx_cct", N.C.byref(cfg))
    table, n = N.param_table(MAKE["ViT"](0)._cfg)
    assert table[0] == ("pos_embedding", (1, 17, 16), 0) and n == sum(int(np.prod(s)) for _, s, _ in table)
