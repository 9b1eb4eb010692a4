"""twins_svt, CPU tier: tests/twins_ref.py (float64 torch restatement) against tests/golden/ref_twins_*.npz, which tools/gen_twins_fixtures.py
produced by executing the reference's own twins_svt.py; the generator's grouped / 'valid' Conv2D and GlobalAvgPool2D shim extras against an
independent formulation; the library's host-only parameter table against the restatement's own; the global_k flag of vitx_config; what is
refused without a device."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import twins_ref  # noqa: E402
import gen_twins_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import twins_svt  # noqa: E402

F64_TOL = 1e-12


def zero_gradient_names(kw, image):
    """Variables whose true gradient is zero: a global attention with ONE key has softmax == 1 whatever q and k are, so to_q and the k half of
    to_kv receive nothing; so does a local attention on one-token windows."""
    out = set()
    H, W = image
    for s, (d, p, lp, gk, depth, has_local) in enumerate(twins_ref.stages_of(kw)):
        H, W = H // p, W // p
        for t, n in ((0, 1), (1, depth)):
            for l in range(n):
                q = f"svt_layers.{s}.transformer.{t}.{l}"
                if (H // gk) * (W // gk) == 1:
                    out.add(q + ".global_attn.to_q.kernel")
                if has_local and lp == 1:
                    out.add(q + ".local_attn.to_q.kernel")
    return out


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    logits, grads, dimg = twins_ref.forward_backward(kw, P, z["img"], z["dlogits"])
    assert z["img"].shape[1:3] == G.image_of(case)
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z if k.startswith("grad/"))
    zero = zero_gradient_names(kw, G.image_of(case))
    for n in P:
        ref = z["grad/" + n]
        assert ref.shape == P[n].shape, n
        if n in zero:
            assert np.abs(ref).max() <= 1e-12, n
        else:
            assert np.abs(ref).max() > 0, n          # every other variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


def test_fixture_files_stay_small():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_twins_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 480 * 1024
    assert sum(os.path.getsize(f) for f in files) <= 4 * 1024 * 1024


@pytest.mark.parametrize("H,W,k,s,padding,groups,bias", [
    (4, 6, 1, 1, "valid", 1, True), (4, 6, 1, 1, "valid", 1, False),          # the 1x1 Denses
    (4, 6, 2, 2, "valid", 1, False), (7, 7, 7, 7, "valid", 1, False), (5, 7, 2, 2, "valid", 1, False),   # to_kv; 5 x 7: 'valid' floors
    (4, 6, 3, 1, "SAME", 5, True), (2, 2, 5, 1, "SAME", 5, True), (1, 3, 3, 1, "SAME", 5, True)])       # the depthwise PEG convolution
def test_conv_extra_is_the_convolution(H, W, k, s, padding, groups, bias):
    """The generator's Conv2D (extract_patches + a product with the kernel + bias) against torch's conv2d on an explicitly padded tensor."""
    g = torch.Generator().manual_seed(H * 100 + W)
    cin = 5
    x = torch.randn(2, H, W, cin, dtype=torch.float64, generator=g)
    filters = cin if groups > 1 else 6
    layer = G.Conv2D(filters=filters, kernel_size=k, strides=s, padding=padding, use_bias=bias, groups=groups)
    layer(x)
    assert tuple(layer.kernel.shape) == (k, k, cin // groups, filters)
    if bias:
        G.tf_shim.assign(layer.bias, torch.randn(filters, dtype=torch.float64, generator=g))
    got = layer(x)
    xp = x.permute(0, 3, 1, 2)
    if padding == "SAME":
        pt, pb = twins_ref.same_pads(H, k, s)
        pl, pr = twins_ref.same_pads(W, k, s)
        xp = F.pad(xp, (pl, pr, pt, pb))
    want = F.conv2d(xp, torch.as_tensor(layer.kernel).permute(3, 2, 0, 1), torch.as_tensor(layer.bias) if bias else None, stride=s,
                    groups=groups).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(want.shape)
    assert want.shape[1:3] == ((-(-H // s), -(-W // s)) if padding == "SAME" else ((H - k) // s + 1, (W - k) // s + 1))
    assert float((torch.as_tensor(got) - want).abs().max()) <= 1e-13


def test_pool_extra_is_the_mean_over_the_map():
    x = torch.randn(3, 4, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    got = G.GlobalAvgPool2D()(x)
    assert tuple(got.shape) == (3, 6)
    assert float((torch.as_tensor(got) - x.mean(dim=(1, 2))).abs().max()) <= 1e-15


def test_abi_symbols_exist():
    l = N.lib()
    for s in ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
              "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end"):
        assert hasattr(l, "vitx_twins_" + s), s


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_restatements_and_the_generators(case):
    z, kw = G.load(case), G.kwargs_of(case)
    table = list(twins_svt.TwinsSVT(**kw)._table)
    assert [(n, tuple(s), o) for n, s, o in table] == twins_ref.table_of(kw)
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]


def test_usage_configuration_table():
    """twins_svt.py:271-298: 8 heads of 64 at every width, 7 x 7 to_kv kernels, no local pair at stage 4."""
    m = twins_svt.TwinsSVT(num_classes=1000)
    table = [(n, tuple(s), o) for n, s, o in m._table]
    assert table == twins_ref.table_of(dict(num_classes=1000))
    shapes = {n: s for n, s, _ in table}
    assert shapes["svt_layers.0.patch_embedding.proj.kernel"] == (1, 1, 48, 64)
    assert shapes["svt_layers.1.patch_embedding.proj.kernel"] == (1, 1, 256, 128)
    assert shapes["svt_layers.0.transformer.0.0.local_attn.to_kv.kernel"] == (1, 1, 64, 1024)
    assert shapes["svt_layers.2.transformer.1.4.global_attn.to_kv.kernel"] == (7, 7, 256, 1024)
    assert shapes["svt_layers.3.transformer.1.3.global_attn.to_q.kernel"] == (1, 1, 512, 512)
    assert shapes["svt_layers.2.peg.kernel"] == (3, 3, 1, 256) and shapes["head.kernel"] == (512, 1000)
    assert not any(".local_attn." in n or ".ff1." in n for n in shapes if n.startswith("svt_layers.3."))
    assert "svt_layers.0.transformer.1.1.ff2.fc1.kernel" not in shapes and "svt_layers.2.transformer.1.5.ff2.fc1.kernel" not in shapes
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())
    assert m.maps_of(224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]


def _vit_cfg(global_k=0, nest_block=1, H=4, W=6):
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h, c.image_w = H, W
    c.patch_h = c.patch_w = 1
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 1, 1, 8, 2, 2, 16, 32
    c.pool, c.ln_eps, c.max_batch = N.POOL_CLS, 1e-5, 1
    c.nest_block, c.global_k = nest_block, global_k
    return c


def test_flag_keeps_the_struct_and_a_cleared_flag_the_table():
    assert C.sizeof(N.Config) == 29 * 4
    assert N.Config.nest_block.offset == 26 * 4 and N.Config.global_k.offset == 27 * 4 and N.Config.global_k.size == 4
    assert N.Config.reserved.offset == 25 * 4 and N.Config.reserved.size == 16
    assert list(_vit_cfg(global_k=2).reserved) == [0, 1, 2, 0]
    plain = N.param_table(_vit_cfg())[0]
    flagged = N.param_table(_vit_cfg(global_k=2))[0]
    assert "transformer.0.attn.to_qkv.kernel" in [t[0] for t in plain] and "transformer.0.attn.to_q.kernel" not in [t[0] for t in plain]
    names = [t[0] for t in flagged]
    assert "transformer.0.attn.to_qkv.kernel" not in names
    shapes = {t[0]: t[1] for t in flagged}
    assert shapes["transformer.1.attn.to_q.kernel"] == (8, 32) and shapes["transformer.1.attn.to_kv.kernel"] == (2 * 2 * 8, 64)
    assert [n for n in names if "to_q" not in n and "to_kv" not in n] == [t[0] for t in plain if "to_qkv" not in t[0]]


def test_flag_refusals():
    with pytest.raises(N.VitxError, match="global_k needs nest_block"):
        N.param_table(_vit_cfg(global_k=2, nest_block=0))
    with pytest.raises(N.VitxError, match="global_k must divide"):
        N.param_table(_vit_cfg(global_k=4))
    c = _vit_cfg(global_k=2)
    c.patch_h = c.patch_w = 2
    with pytest.raises(N.VitxError, match="patch_h == patch_w == 1"):
        N.param_table(c)


def test_constructor_and_call_refusals():
    kw = G.kwargs_of("twins_tiny")
    m = twins_svt.TwinsSVT(**kw)
    with pytest.raises(ValueError, match="s1_patch_size"):
        m(np.zeros((1, 9, 8, 3), np.float32))                       # 9 rows, patch 2
    with pytest.raises(ValueError, match="s3_local_patch_size"):
        m(np.zeros((1, 12, 8, 3), np.float32))                      # 6 x 4 maps at stages 1 and 2, 3 x 2 at stage 3 with 2 x 2 windows
    with pytest.raises(ValueError, match="s1_local_patch_size"):
        twins_svt.TwinsSVT(**{**kw, "s1_local_patch_size": 3})(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="s3_patch_size"):
        twins_svt.TwinsSVT(**{**kw, "s1_local_patch_size": 1, "s2_local_patch_size": 1, "s1_global_k": 1, "s2_global_k": 1})(
            np.zeros((1, 6, 8, 3), np.float32))                     # 3 x 4 maps at stages 1 and 2, then patch 2
    with pytest.raises(ValueError, match="s1_global_k"):
        twins_svt.TwinsSVT(**{**kw, "s1_global_k": 3})(np.zeros((1, 8, 8, 3), np.float32))   # 4 x 4 map: the reference would floor to 1 x 1
    with pytest.raises(ValueError, match="s2_local_patch_size"):
        twins_svt.TwinsSVT(**{**kw, "s2_local_patch_size": 3})(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="s4_global_k"):
        twins_svt.TwinsSVT(**{**kw, "s4_global_k": 4}, image_size=8)                         # the eager form refuses at construction
    with pytest.raises(ValueError, match="expected NHWC"):
        m(np.zeros((1, 8, 8, 4), np.float32))
    with pytest.raises(ValueError, match="peg_kernel_size must be odd"):
        twins_svt.TwinsSVT(**kw, peg_kernel_size=2)
    with pytest.raises(ValueError, match="multiple of 64"):                                   # before a device is looked for
        twins_svt.TwinsSVT(**kw, compute="bf16")
    with pytest.raises(TypeError, match="unexpected keyword"):
        twins_svt.TwinsSVT(**kw, heads=4)
    d = twins_svt.TwinsSVT(**kw, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        d(np.zeros((1, 8, 8, 3), np.float32))                       # training=True is the reference's default
    with pytest.raises(NotImplementedError, match="dropout"):
        d(np.zeros((1, 8, 8, 3), np.float32), training=True)
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()
    # the C table refuses the same geometry, and vitx_twins_create a configuration without an image
    c = N.TwinsConfig.from_buffer_copy(m._cfg)
    c.image_h, c.image_w = 8, 16
    N.twins_param_table(c)
    c.image_h = 9
    with pytest.raises(N.VitxError, match="s1_patch_size"):
        N.twins_param_table(c)
    c.image_h = 0
    with pytest.raises(N.VitxError, match="invalid image size"):
        N.twins_param_table(c)


def test_weights_api_round_trip(tmp_path):
    kw = G.kwargs_of("twins_tiny")
    m = twins_svt.TwinsSVT(**kw, seed=1)
    sd = m.state_dict()
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd) == len(m.trainable_variables)
    assert np.all(sd["svt_layers.0.transformer.0.0.global_attn.norm.g"] == 1) and np.all(sd["head.bias"] == 0)
    k = sd["svt_layers.2.peg.kernel"]
    assert k.shape == (3, 3, 1, 8) and 0 < np.abs(k).max() <= np.sqrt(6.0 / (9 * 1 + 9 * 8)) + 1e-6
    k = sd["svt_layers.0.transformer.0.0.global_attn.to_kv.kernel"]
    assert k.shape == (2, 2, 4, 1024) and 0 < np.abs(k).max() <= np.sqrt(6.0 / (4 * 4 + 4 * 1024)) + 1e-6
    m.save_weights(str(tmp_path / "w"))
    m2 = twins_svt.TwinsSVT(**kw, seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in twins_ref.table_of(kw))
