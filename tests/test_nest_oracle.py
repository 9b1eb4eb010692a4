"""nest, CPU tier: tests/nest_ref.py (float64 torch restatement) against tests/golden/ref_nest_*.npz, which tools/gen_nest_fixtures.py produced
by executing the reference's own nest.py; the generator's Conv2D / MaxPool2D shim extras against an independent formulation; the library's
host-only parameter table against the restatement's own; the nest_block flag; what is refused without a device; and the zero gradient of the
last level's pos_emb (one scalar per position ahead of channel LayerNorms only: the reference gives 1e-16 .. 1e-17 there)."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import nest_ref  # noqa: E402
import gen_nest_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import nest  # noqa: E402

F64_TOL = 1e-12


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    logits, grads, dimg = nest_ref.forward_backward(kw, P, z["img"], z["dlogits"])
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z if k.startswith("grad/"))
    for n in P:
        ref = z["grad/" + n]
        assert ref.shape == P[n].shape, n
        if n != nest_ref.last_pos_emb(kw):
            assert np.abs(ref).max() > 0, n          # every other variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


@pytest.mark.parametrize("case", list(G.CASES))
def test_last_level_pos_emb_has_a_zero_gradient(case):
    """pos_emb is one scalar per position, broadcast over channels, and every LayerNorm normalises over channels: behind the LAST level's
    pos_emb there is no aggregation convolution to mix channels, so its true gradient is exactly zero.  The finer levels' are of order 1."""
    z, kw = G.load(case), G.kwargs_of(case)
    last = nest_ref.last_pos_emb(kw)
    assert np.abs(z["grad/" + last]).max() <= 1e-12
    for i in range(kw["num_hierarchies"] - 1):
        assert np.abs(z[f"grad/nest_layers.{i}.transformer.pos_emb"]).max() > 1e-3, i


def test_fixture_files_stay_small():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_nest_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 480 * 1024


@pytest.mark.parametrize("H,W,k,s,bias", [(5, 8, 3, 1, True), (6, 6, 3, 1, True), (1, 2, 3, 1, True), (4, 7, 1, 1, True), (4, 7, 1, 1, False),
                                          (7, 6, 3, 2, False)])
def test_conv_extra_is_a_same_convolution(H, W, k, s, bias):
    """The generator's biased Conv2D (extract_patches + matmul + bias) against torch's conv2d on an explicitly 'SAME'-padded tensor."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 3, dtype=torch.float64, generator=g)
    layer = G.Conv2D(filters=5, kernel_size=k, strides=s, padding="SAME" if k > 1 else "valid", use_bias=bias)
    layer(x)
    if bias:
        G.tf_shim.assign(layer.bias, torch.randn(5, dtype=torch.float64, generator=g))
    got = layer(x)
    want = nest_ref.conv_same(x, layer.kernel, layer.bias if bias else None, s)
    assert got.shape == want.shape == (2, -(-H // s), -(-W // s), 5)
    assert float((got - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("H,W,k,s", [(1, 1, 3, 2), (2, 3, 3, 2), (5, 6, 3, 2), (6, 6, 3, 2), (7, 8, 2, 2), (4, 9, 5, 3)])
def test_pool_extra_is_a_same_max_pool_on_signed_input(H, W, k, s):
    """The generator's MaxPool2D (shift non-negative, extract_patches + max, shift back) against torch's max_pool2d on a tensor padded with -inf."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 4, dtype=torch.float64, generator=g) - 0.5
    assert float(x.min()) < 0
    got = G.MaxPool2D(pool_size=k, strides=s, padding="SAME")(x)
    want = nest_ref.maxpool_same(x, k, s)
    assert got.shape == want.shape == (2, -(-H // s), -(-W // s), 4)
    assert float((torch.as_tensor(got) - want).abs().max()) <= 4.5e-16 * max(1.0, float(x.abs().max()))   # two roundings of at most half an ulp at magnitude <= 2 max|x|


def test_abi_symbols_exist():
    l = N.lib()
    for s in ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
              "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end"):
        assert hasattr(l, "vitx_nest_" + s), s


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_restatements_and_the_generators(case):
    z, kw = G.load(case), G.kwargs_of(case)
    table = list(nest.NesT(**kw)._table)
    assert [(n, tuple(s), o) for n, s, o in table] == nest_ref.table_of(kw)
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]


def test_usage_configuration_table():
    """nest.py:218-231: dim_head 32 at every level, 196 tokens per block."""
    m = nest.NesT(image_size=224, patch_size=4, dim=96, heads=3, num_hierarchies=3, block_repeats=(2, 2, 8), num_classes=1000)
    shapes = {n: s for n, s, _ in m._table}
    assert m.seq_len == 196 and shapes["nest_layers.0.transformer.pos_emb"] == (196,)
    assert shapes["patch_embedding.kernel"] == (1, 1, 48, 96) and shapes["nest_layers.1.aggregate.conv.kernel"] == (3, 3, 192, 384)
    assert shapes["nest_layers.2.transformer.7.attn.to_qkv.kernel"] == (1, 1, 384, 1152) and shapes["mlp_head.kernel"] == (384, 1000)
    assert "nest_layers.2.aggregate.conv.kernel" not in shapes
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())


def _vit_cfg(nest_block=0, cct_block=0, small_dataset=0, heads=2, dim_head=16, variant=None):
    c = N.Config()
    c.variant = N.VARIANT_VIT if variant is None else variant
    c.image_h = c.image_w = 16
    c.patch_h = c.patch_w = 4
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 3, 5, 32, 2, heads, dim_head, 48
    c.cls_depth = 1
    c.pool, c.ln_eps, c.max_batch = N.POOL_CLS, 1e-5, 1
    c.nest_block, c.cct_block, c.small_dataset = nest_block, cct_block, small_dataset
    return c


def test_flag_keeps_the_struct_and_a_cleared_flag_the_plain_table():
    from oracle import spec
    assert C.sizeof(N.Config) == 29 * 4
    assert N.Config.small_dataset.offset == 24 * 4 and N.Config.cct_block.offset == 25 * 4 and N.Config.reserved.offset == 25 * 4
    assert N.Config.nest_block.offset == 26 * 4 and N.Config.nest_block.size == 4 and N.Config.reserved.size == 16
    c = _vit_cfg(nest_block=1)
    assert list(c.reserved) == [0, 1, 0, 0]
    table, _ = N.param_table(_vit_cfg())
    cfg = spec.make_config(variant="vit", image_size=16, patch_size=4, num_classes=5, dim=32, depth=2, heads=2, mlp_dim=48, dim_head=16)
    assert [(t[0], tuple(t[1])) for t in table] == [(nm, tuple(sh)) for nm, sh, _ in spec.param_spec(cfg)]
    # the flag keeps the table, except that heads == 1 with dim_head == dim keeps to_out (nest.py:88-91 always projects)
    assert [t[0] for t in N.param_table(_vit_cfg(nest_block=1))[0]] == [t[0] for t in table]
    plain1 = [t[0] for t in N.param_table(_vit_cfg(heads=1, dim_head=32))[0]]
    flag1 = [t[0] for t in N.param_table(_vit_cfg(nest_block=1, heads=1, dim_head=32))[0]]
    assert "transformer.0.attn.to_out.kernel" not in plain1 and "transformer.0.attn.to_out.kernel" in flag1


def test_flag_refusals():
    with pytest.raises(N.VitxError, match="cct_block"):
        N.param_table(_vit_cfg(nest_block=1, cct_block=1))
    with pytest.raises(N.VitxError, match="small_dataset"):
        N.param_table(_vit_cfg(nest_block=1, small_dataset=1))
    for variant in (N.VARIANT_DEEPVIT, N.VARIANT_CAIT, N.VARIANT_PATCH_MERGER):
        with pytest.raises(N.VitxError, match="nest_block needs the ViT variant"):
            N.param_table(_vit_cfg(nest_block=1, variant=variant))
    c = _vit_cfg(nest_block=1)
    c.num_parallel_branches = 2
    with pytest.raises(N.VitxError, match="num_parallel_branches"):
        N.param_table(c)


def test_constructor_and_call_refusals():
    kw = G.kwargs_of("nest_1level")
    with pytest.raises(ValueError, match="Image dimensions must be divisible by the patch size."):      # nest.py:163
        nest.NesT(**{**kw, "image_size": 10})
    with pytest.raises(ValueError, match="divisible by 2\\^\\(num_hierarchies - 1\\)"):
        nest.NesT(**{**G.kwargs_of("nest_small"), "image_size": 12})                                     # 6 x 6 map, 4 blocks per side
    with pytest.raises(ValueError, match="block_repeats has 2 entries for num_hierarchies = 3"):
        nest.NesT(**{**G.kwargs_of("nest_small"), "block_repeats": (1, 1)})
    m = nest.NesT(**kw)
    with pytest.raises(ValueError, match="image_size"):
        m(np.zeros((1, 16, 16, 3), np.float32))
    with pytest.raises(ValueError, match="image_size"):
        m(np.zeros((1, 8, 4, 3), np.float32))
    d = nest.NesT(**kw, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        d(np.zeros((1, 8, 8, 3), np.float32))                                                            # training=True is the reference's default
    with pytest.raises(NotImplementedError, match="dropout"):
        d(np.zeros((1, 8, 8, 3), np.float32), training=True)
    # the C table refuses the same geometry
    c = N.NesTConfig()
    c.image_size, c.patch_size, c.num_classes, c.dim, c.heads, c.num_hierarchies, c.mlp_mult = 12, 2, 5, 8, 1, 3, 2
    with pytest.raises(N.VitxError, match="divisible by 2\\^\\(num_hierarchies - 1\\)"):
        N.nest_param_table(c)
    # refused by vitx_nest_create before a device is looked for: the usage's dim 96 in the bf16 mode
    bad = nest.NesT(image_size=32, patch_size=4, dim=96, heads=3, num_hierarchies=2, block_repeats=1, num_classes=10, compute="bf16")
    with pytest.raises(N.VitxError, match="multiples of 64"):
        bad._ensure_handle(1)
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()


def test_small_attn_choice_reaches_the_config():
    """vitx_nest_config.small_attn came out of its reserved words: 0 = the measured per-mode default, 1 = wherever they apply, -1 = nowhere."""
    kw = G.kwargs_of("nest_1level")
    assert C.sizeof(N.NesTConfig) == 28 * 4 and N.NesTConfig.small_attn.offset == 20 * 4 and N.NesTConfig.reserved.size == 7 * 4
    assert [nest.NesT(**kw, small_attn=v)._cfg.small_attn for v in (None, True, False)] == [0, 1, -1]
    assert nest.NesT(**kw)._cfg.small_attn == 0


def test_weights_api_round_trip(tmp_path):
    kw = G.kwargs_of("nest_small")
    m = nest.NesT(**kw, seed=1)
    sd = m.state_dict()
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd) == len(m.trainable_variables)
    assert np.all(sd["mlp_head.norm.g"] == 1) and np.all(sd["mlp_head.bias"] == 0) and np.abs(sd["nest_layers.0.transformer.pos_emb"]).max() > 0
    k = sd["nest_layers.0.aggregate.conv.kernel"]
    assert k.shape == (3, 3, 8, 16) and np.abs(k).max() <= np.sqrt(6.0 / (9 * 8 + 9 * 16)) + 1e-6
    m.save_weights(str(tmp_path / "w"))
    m2 = nest.NesT(**kw, seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in nest_ref.table_of(kw))
