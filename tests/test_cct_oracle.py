"""cct, CPU tier: tests/cct_ref.py (float64 torch restatement) against tests/golden/ref_cct_*.npz, which tools/gen_cct_fixtures.py produced by
executing the reference's own cct.py; the generator's Conv2D / MaxPool2D shim extras against an independent formulation; the 'SAME' geometry
rule for the sequence length; the library's host-only parameter table, the cct_block flag and what is refused without a device; the factories."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cct_ref  # noqa: E402
import gen_cct_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import cct  # noqa: E402

F64_TOL = 1e-12


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z, case)
    logits, grads, dimg = cct_ref.forward_backward(G.kwargs_of(case), P, z["img"], z["dlogits"])
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z if k.startswith("grad/"))
    for n in P:
        ref = z["grad/" + n]
        if n == "classifier.attention_pool.bias" or (case == "cct_1tok" and n == "classifier.attention_pool.kernel"):
            assert np.abs(ref).max() <= 1e-15, n     # softmax is shift-invariant; over one token it is 1 whatever the logit
        else:
            assert np.abs(ref).max() > 0, n          # every other variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


def test_fixture_files_stay_small():
    import glob
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_cct_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 560 * 1024     # the size range of the other models' fixtures


@pytest.mark.parametrize("H,W,k,s", [(5, 8, 3, 1), (6, 7, 3, 2), (7, 6, 7, 2), (1, 2, 3, 1), (4, 4, 7, 2), (9, 12, 2, 2)])
def test_conv_extra_is_a_same_convolution(H, W, k, s):
    """The generator's Conv2D (extract_patches + matmul) against torch's conv2d on an explicitly 'SAME'-padded tensor."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 3, dtype=torch.float64, generator=g)
    layer = G.Conv2D(filters=5, kernel_size=k, strides=s, padding="SAME", use_bias=False)
    got = layer(x)
    want = cct_ref.conv_same(x, layer.kernel, s)
    assert got.shape == want.shape == (2, -(-H // s), -(-W // s), 5)
    assert float((got - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("H,W,k,s", [(1, 1, 3, 2), (2, 3, 3, 2), (5, 6, 3, 2), (6, 5, 3, 1), (7, 8, 2, 2), (4, 9, 5, 3)])
def test_pool_extra_is_a_same_max_pool(H, W, k, s):
    """The generator's MaxPool2D (extract_patches + max) against torch's max_pool2d on a tensor explicitly padded with -inf."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.relu(torch.randn(2, H, W, 4, dtype=torch.float64, generator=g))
    got = G.MaxPool2D(pool_size=k, strides=s, padding="SAME")(x)
    want = cct_ref.maxpool_same(x, k, s)
    assert got.shape == want.shape == (2, -(-H // s), -(-W // s), 4)
    assert torch.equal(torch.as_tensor(got), want)
    with pytest.raises(AssertionError):
        G.MaxPool2D(pool_size=k, strides=s, padding="SAME")(x - 1.0)


def test_same_padding_is_asymmetric():
    assert cct_ref.same_pads(6, 3, 2) == (3, 0, 1) and cct_ref.same_pads(5, 3, 2) == (3, 1, 1) and cct_ref.same_pads(224, 7, 2) == (112, 2, 3)


def test_sequence_lengths():
    """The geometry rule gives what Tokenizer.sequence_length found by running the tokenizer on zeros (recorded in the fixtures), and the
    counts of the reference's usage configurations."""
    for case in G.CASES:
        z = G.load(case)
        kw = G.kwargs_of(case)
        assert cct.CCT(**kw).sequence_length == int(z["sequence_length"]) == cct_ref.sequence_length(kw)
    k7 = dict(kernel_size=7, stride=2, pooling_kernel_size=3, pooling_stride=2, num_layers=1, num_heads=2, embedding_dim=8, num_classes=2,
              positional_embedding="none")
    assert cct.CCT(img_size=224, n_conv_layers=1, **k7).sequence_length == 3136
    assert cct.CCT(img_size=224, n_conv_layers=2, **k7).sequence_length == 196
    assert cct.CCT(img_size=(224, 448), n_conv_layers=2, **k7).sequence_length == 392
    assert cct.sequence_length((224, 448), n_conv_layers=2) == 392 and cct.sequence_length(224) == 3136


def test_abi_symbols_exist():
    l = N.lib()
    for s in ("param_table_size", "param_table_entry", "sequence_length", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev",
              "grads_dev", "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end"):
        assert hasattr(l, "vitx_cct_" + s), s


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_generators(case):
    z = G.load(case)
    table = cct_ref.table_of(G.kwargs_of(case))
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]
    off = 0
    for _, s, o in table:
        assert o == off
        off += int(np.prod(s))


def test_sine_is_not_a_parameter():
    kw = {**G.kwargs_of("cct_small"), "positional_embedding": "sine"}
    names = [t[0] for t in cct_ref.table_of(kw)]
    assert "classifier.positional_emb" not in names
    assert names == [t[0] for t in cct_ref.table_of({**kw, "positional_embedding": "none"})]
    kw.pop("positional_embedding")                       # 'sine' is TransformerClassifier's default (cct.py:228)
    assert cct.CCT(**kw).positional_embedding == "sine"
    t = cct_ref.sine_table(3, 4)[0]
    assert np.allclose(t[:, 0], np.sin(np.arange(3))) and np.allclose(t[:, 1], np.cos(np.arange(3)))
    assert np.allclose(t[:, 2], np.sin(np.arange(3) / 100.0)) and np.allclose(t[:, 3], np.cos(np.arange(3) / 100.0))


def _vit_cfg(cct_block=0, small_dataset=0, heads=2, dim_head=16, dropout=0.0):
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h = c.image_w = 16
    c.patch_h = c.patch_w = 4
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 3, 5, 32, 2, heads, dim_head, 48
    c.pool, c.ln_eps, c.max_batch, c.dropout = N.POOL_CLS, 1e-3, 1, dropout
    c.cct_block, c.small_dataset = cct_block, small_dataset
    return c


def test_zeroed_flag_leaves_the_plain_vit_table():
    """The flag came out of `reserved`: same struct size, and a cleared flag gives the plain ViT's table (oracle/spec.py states it)."""
    from oracle import spec
    assert C.sizeof(N.Config) == 29 * 4
    assert N.Config.small_dataset.offset == 24 * 4 and N.Config.cct_block.offset == 25 * 4 and N.Config.cct_block.size == 4
    table, _ = N.param_table(_vit_cfg())
    cfg = spec.make_config(variant="vit", image_size=16, patch_size=4, num_classes=5, dim=32, depth=2, heads=2, mlp_dim=48, dim_head=16)
    assert [(t[0], tuple(t[1])) for t in table] == [(nm, tuple(sh)) for nm, sh, _ in spec.param_spec(cfg)]
    # the flag keeps the table, except that heads == 1 with dim_head == dim keeps to_out (cct.py:117-122 always projects)
    assert [t[0] for t in N.param_table(_vit_cfg(cct_block=1))[0]] == [t[0] for t in table]
    plain1 = [t[0] for t in N.param_table(_vit_cfg(heads=1, dim_head=32))[0]]
    flag1 = [t[0] for t in N.param_table(_vit_cfg(cct_block=1, heads=1, dim_head=32))[0]]
    assert "transformer.0.attn.to_out.kernel" not in plain1 and "transformer.0.attn.to_out.kernel" in flag1


def test_host_side_refusals():
    with pytest.raises(N.VitxError, match="small_dataset"):
        N.param_table(_vit_cfg(cct_block=1, small_dataset=1))
    with pytest.raises(N.VitxError, match="dropout"):
        N.param_table(_vit_cfg(cct_block=1, dropout=0.1))
    m = cct.CCT(**G.kwargs_of("cct_1tok"))
    with pytest.raises(NotImplementedError, match="dropout on the attention probabilities.*stochastic depth"):
        m(np.zeros((1, 4, 4, 3), np.float32), training=True)
    with pytest.raises(ValueError, match="img_size"):
        m(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(TypeError):
        cct.CCT(attention_dropout=0.0)                   # hard-wired by CCT (cct.py:337): a duplicate keyword in the reference
    with pytest.raises(TypeError):
        cct.CCT(stochastic_depth_rate=0.0)
    # refused by vitx_cct_create before a device is looked for
    bad = cct.CCT(**{**G.kwargs_of("cct_small"), "embedding_dim": 96, "num_heads": 2}, compute="bf16")
    with pytest.raises(N.VitxError, match="multiples of 64"):
        bad._ensure_handle(1)
    with pytest.raises(N.VitxError, match="divisible by num_heads"):
        cct.CCT(**{**G.kwargs_of("cct_small"), "embedding_dim": 30, "num_heads": 4})
    from vit_tensorflow.mae import MAE
    with pytest.raises(AssertionError):
        MAE(image_size=4, encoder=m, masking_ratio=0.75, decoder_dim=16)   # the wrappers take the library's ViT / DeepViT only


FACTORIES = {"cct_2": (2, 2, 1, 128), "cct_4": (4, 2, 1, 128), "cct_6": (6, 4, 2, 256), "cct_7": (7, 4, 2, 256), "cct_8": (8, 4, 2, 256),
             "cct_14": (14, 6, 3, 384), "cct_16": (16, 6, 3, 384)}   # cct.py:16-48


def test_factories():
    assert cct.__all__ == list(FACTORIES)
    for name, (layers, heads, ratio, dim) in FACTORIES.items():
        m = getattr(cct, name)(img_size=32, num_classes=10, positional_embedding="learnable")
        c = m._cfg
        assert (c.num_layers, c.num_heads, c.dim_feedforward, c.embedding_dim) == (layers, heads, ratio * dim, dim), name
        assert (c.kernel_size, c.stride) == (3, 1)                                    # _cct: max(1, 3 // 2 - 1)
    for k, s in ((3, 1), (5, 1), (7, 2), (9, 3)):
        assert cct.cct_2(img_size=32, kernel_size=k, num_classes=3)._cfg.stride == s  # cct.py:54
    assert cct.cct_2(img_size=32, kernel_size=7, stride=1, num_classes=3)._cfg.stride == 1
    # the usage example (cct.py:348-363): unknown keywords are swallowed, so the misspelt mlp_radio leaves mlp_ratio at 4.0
    m = cct.CCT(img_size=(224, 448), embedding_dim=384, n_conv_layers=2, kernel_size=7, stride=2, padding=3, pooling_kernel_size=3,
                pooling_stride=2, pooling_padding=1, num_layers=14, num_heads=6, mlp_radio=3., num_classes=1000, positional_embedding='learnable')
    assert m.sequence_length == 392 and m._cfg.dim_feedforward == 1536
    shapes = {n: s for n, s, _ in m._table}
    assert shapes["tokenizer.conv_layers.0.kernel"] == (7, 7, 3, 64) and shapes["tokenizer.conv_layers.1.kernel"] == (7, 7, 64, 384)
    assert shapes["classifier.positional_emb"] == (1, 392, 384) and shapes["classifier.attention_pool.kernel"] == (384, 1)
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())


def test_weights_api_round_trip(tmp_path):
    m = cct.CCT(**G.kwargs_of("cct_small"), seed=1)
    sd = m.state_dict()
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd)
    assert np.abs(sd["classifier.positional_emb"]).max() <= 0.4 + 1e-6       # truncated normal, stddev 0.2
    assert np.all(sd["classifier.norm.gamma"] == 1) and np.all(sd["classifier.fc.bias"] == 0)
    m.save_weights(str(tmp_path / "w"))
    m2 = cct.CCT(**G.kwargs_of("cct_small"), seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
