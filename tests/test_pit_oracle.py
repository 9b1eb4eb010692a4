"""PiT, CPU tier: the float64 restatement (tests/pit_ref.py) reproduces every fixture the reference's own pit.py wrote
(tools/gen_pit_fixtures.py) to 1e-12, its table is the C library's, and the generator's grouped-convolution stand-in is torch's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_pit_fixtures as gen  # noqa: E402
import pit_ref  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow.pit import PiT, cast_tuple, conv_output_size  # noqa: E402

MODEL_CASES = list(gen.CASES)
TOL = 1e-12


def _rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / max(float(np.abs(want).max()), 1e-300))


@pytest.mark.parametrize("case", MODEL_CASES)
def test_restatement_reproduces_the_reference(case):
    z = gen.load(case)
    kw = gen.kwargs_of(case)
    logits, grads, dimg = pit_ref.run(kw, gen.params_of(z), z["img"], z["dlogits"])
    assert _rel(logits, z["logits"]) < TOL
    assert _rel(dimg, z["dimg"]) < TOL
    assert [str(n) for n in z["names"]] == [n for n, _, _ in pit_ref.table_of(kw)]
    for n in z["names"]:
        want = z["grad/" + str(n)]
        assert np.abs(want).max() > 0 or str(n) == "pos_embedding", n
        assert _rel(grads[str(n)], want) < TOL, n


def test_restatement_reproduces_the_reference_pool():
    z = gen.load("pit_pool_layer")
    P = gen.params_of(z)
    assert int(z["dim"]) == gen.POOL_DIM and tuple(z["maps"]) == gen.POOL_MAPS
    for hw in gen.POOL_MAPS:
        out, grads, dtok = pit_ref.run_pool(P, z[f"tokens_{hw}"], z[f"dout_{hw}"])
        no = 1 + (-(-hw // 2)) ** 2
        assert out.shape == (2, no, 2 * gen.POOL_DIM)
        assert _rel(out, z[f"out_{hw}"]) < TOL, hw
        assert _rel(dtok, z[f"dtokens_{hw}"]) < TOL, hw
        for n in z["names"]:
            assert _rel(grads[str(n)], z[f"grad_{hw}/{n}"]) < TOL, (hw, n)


def test_reference_never_pools():
    """pit.py:194: `not_last = ind < (len(depth) < 1)` is never true -- the reference's PiT(depth=(1, 2, 1)) holds three Transformers, no Pool."""
    z = gen.load("pit_small")
    assert [str(c) for c in z["layer_classes"]] == ["Transformer", "Transformer", "Transformer"]
    assert not any(str(n).startswith("pool.") for n in z["names"])
    assert (0 < (1 < 1)) is False   # the expression itself, for ind = 0 and a depth of one entry


def test_standin_is_torchs_grouped_convolution():
    assert gen.check_standin() < 1e-13


def test_same_pads_cover_both_cases():
    assert pit_ref.same_pads(31, 3, 2) == (1, 1) and pit_ref.same_pads(16, 3, 2) == (0, 1)
    assert pit_ref.same_pads(2, 3, 2) == (0, 1) and pit_ref.same_pads(1, 3, 2) == (1, 1)


def _front(kw, **extra):
    return PiT(**kw, **extra)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_table_is_the_librarys(case):
    kw = gen.kwargs_of(case)
    m = _front(kw)
    assert [(n, tuple(s), o) for n, s, o in m._table] == pit_ref.table_of(kw)
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in pit_ref.table_of(kw))


def test_default_table_has_no_pool_entry():
    kw = dict(gen.kwargs_of("pit_pooled"))
    kw.pop("pool_stages")
    names = [n for n, _, _ in _front(kw)._table]
    assert not any(n.startswith("pool.") for n in names)
    assert all(s[0] == kw["dim"] for n, s, _ in _front(kw)._table if n.endswith("attn.norm.gamma"))   # dim never doubles
    pooled = [n for n, _, _ in _front(dict(kw, pool_stages=True))._table]
    assert [n for n in pooled if n.startswith("pool.")][:2] == ["pool.0.downsample.dw.kernel", "pool.0.downsample.dw.bias"]
    assert not any(n.startswith("pool.2.") for n in pooled)   # none behind the last stage


def test_usage_table_and_token_count():
    m = PiT(image_size=224, patch_size=14, dim=256, num_classes=1000, depth=(3, 3, 3), heads=16, mlp_dim=2048, dropout=0.1, emb_dropout=0.1)
    t = {n: s for n, s, _ in m._table}
    assert t["pos_embedding"] == (1, 31 * 31 + 1, 256) and t["patch_embedding.kernel"] == (14 * 14 * 3, 256)
    assert m.maps_of(224, 224) == [(31, 31, 256)] * 3
    p = PiT(image_size=224, patch_size=14, dim=256, num_classes=1000, depth=(3, 3, 3), heads=16, mlp_dim=2048, pool_stages=True)
    assert [1 + h * w for h, w, _ in p.maps_of(224, 224)] == [962, 257, 65]
    assert [d for _, _, d in p.maps_of(224, 224)] == [256, 512, 1024]


def test_constructor_mirrors_the_reference():
    kw = dict(num_classes=3, dim=8, mlp_dim=8, dim_head=8)
    with pytest.raises(AssertionError, match="Image dimensions must be divisible by the patch size."):
        PiT(image_size=30, patch_size=8, depth=(1,), heads=1, **kw)
    with pytest.raises(AssertionError, match="depth must be a tuple of integers"):
        PiT(image_size=32, patch_size=8, depth=[1], heads=1, **kw)
    with pytest.raises(ValueError, match="stride"):
        PiT(image_size=4, patch_size=1, depth=(1,), heads=1, **kw)
    # zip(depth, heads) stops at the shorter (pit.py:193)
    m = PiT(image_size=32, patch_size=8, depth=(1, 1, 1), heads=(1, 2), **kw)
    assert len(m.stages) == 2 and not any(n.startswith("stage.2.") for n, _, _ in m._table)
    # project_out per stage (pit.py:59): heads == 1 and dim_head == dim has no to_out
    names = [n for n, _, _ in m._table]
    assert "stage.0.0.attn.to_out.kernel" not in names and "stage.1.0.attn.to_out.kernel" in names
    assert cast_tuple(3, 2) == (3, 3) and cast_tuple((1, 2), 5) == (1, 2)
    assert conv_output_size(224, 14, 7) == 31 and conv_output_size(28, 7, 3) == 8
    with pytest.raises(ValueError, match="long_attn"):
        PiT(image_size=32, patch_size=8, depth=(1,), heads=1, long_attn=True, **kw)
    # long_attn=None is the measured default: on exactly where the streamed kernels apply (bf16, heads of 64)
    big = dict(num_classes=3, dim=64, mlp_dim=8, image_size=32, patch_size=8, depth=(1,), heads=1)
    assert PiT(**big, dim_head=64, compute="bf16").long_attn is True and PiT(**big, dim_head=64).long_attn is False
    assert PiT(**big, dim_head=32, compute="bf16").long_attn is False and PiT(**big, dim_head=64, compute="bf16", long_attn=False).long_attn is False
    with pytest.raises(ValueError, match="multiple of 64"):
        PiT(image_size=32, patch_size=8, depth=(1,), heads=1, compute="bf16", **kw)
    with pytest.raises(TypeError):
        PiT(image_size=32, patch_size=8, depth=(1,), heads=1, nonsense=1, **kw)


def test_image_refusals_need_no_device():
    m = PiT(image_size=40, patch_size=8, num_classes=3, dim=8, depth=(1, 1), heads=1, mlp_dim=8, dim_head=8, pool_stages=True)
    with pytest.raises(ValueError, match="pos_embedding has 82 rows"):
        m.maps_of(48, 48)
    with pytest.raises(ValueError, match="7 x 9"):
        m.maps_of(32, 40)
    assert PiT(image_size=40, patch_size=8, num_classes=3, dim=8, depth=(1, 1), heads=1, mlp_dim=8, dim_head=8).maps_of(32, 40)[1] == (7, 9, 8)


def test_initialisers_are_keras():
    m = PiT(image_size=32, patch_size=8, num_classes=3, dim=8, depth=(1, 1), heads=2, mlp_dim=8, dim_head=8, pool_stages=True, seed=3)
    sd = m.state_dict()
    assert np.all(sd["stage.0.0.attn.norm.gamma"] == 1) and np.all(sd["pool.0.downsample.dw.bias"] == 0) and np.all(sd["mlp_head.bias"] == 0)
    k = sd["pool.0.downsample.dw.kernel"]
    lim = np.sqrt(6.0 / (9 * 1 + 9 * 16))
    assert k.shape == (3, 3, 1, 16) and np.abs(k).max() <= lim and np.abs(k).max() > 0.5 * lim
    assert 0.5 < sd["pos_embedding"].std() < 1.5 and sd["cls_token"].shape == (1, 1, 8)
