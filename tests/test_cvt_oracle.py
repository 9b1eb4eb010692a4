"""cvt, CPU tier: tests/cvt_ref.py (float64 torch restatement) against tests/golden/ref_cvt_*.npz, which tools/gen_cvt_fixtures.py produced by
executing the reference's own cvt.py; the generator's BatchNormalization stand-in and its strided / depthwise 'SAME' Conv2D against independent
formulations; the library's host-only parameter table against the restatement's own; the conv_proj flag of vitx_config; what is refused
without a device; the weights surface with the moving statistics."""
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

import cvt_ref  # noqa: E402
import gen_cvt_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import cvt  # noqa: E402

F64_TOL = 1e-12
TRAIN_CASES = [c for c in G.CASES if G.CASES[c][2]]


def zero_gradient_names(kw, image):
    """Variables whose true gradient is zero: an attention with ONE key has softmax == 1 whatever q and k are, so the whole q branch (depthwise
    kernel, BatchNorm scale / offset, pointwise kernel) receives nothing.  The offset of the LayerNorm in front of it gets nothing either: it
    moves the one kv position of every image by the same amount per channel, which BatchNormalization over the batch removes (the reference
    gives float64 round-off there, at most 1.3e-16, not always an exact zero)."""
    out = set()
    for s, ((full, kv), st) in enumerate(zip(cvt_ref.maps_of(kw, *image), cvt_ref.stages_of(kw))):
        if kv[0] * kv[1] != 1:
            continue
        for l in range(st[6]):
            q = f"cvt_layers.{s}.transformer.{l}.attn.to_q."
            out |= {q + "dw.kernel", q + "bn.gamma", q + "bn.beta", q + "pw.kernel", f"cvt_layers.{s}.transformer.{l}.attn.norm.b"}
    return out


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    logits, grads, dimg = cvt_ref.forward_backward(kw, P, z["img"], z["dlogits"])
    assert z["img"].shape[1:3] == G.image_of(case) and z["img"].shape[0] == 2
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    trainable = [n for n in P if not cvt_ref.is_moving(n)]
    assert sorted("grad/" + n for n in trainable) == sorted(k for k in z if k.startswith("grad/"))
    zero = zero_gradient_names(kw, G.image_of(case))
    for n in trainable:
        ref = z["grad/" + n]
        assert ref.shape == P[n].shape, n
        if n in zero:
            assert np.abs(ref).max() <= 1e-12, n
        else:
            assert np.abs(ref).max() > 0, n          # every other trainable variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    for n in P:
        if cvt_ref.is_moving(n):
            assert np.abs(grads[n]).max() == 0, n    # a training forward does not read them
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


def test_restatement_reproduces_the_inference_fixture():
    z = G.load("cvt_eval")
    assert int(z["training"]) == 0 and not any(k.startswith("grad/") for k in z)
    kw, P = G.kwargs_of("cvt_eval"), G.params_of(z)
    Pt = {n: torch.tensor(v) for n, v in P.items()}
    logits = cvt_ref.forward(kw, Pt, torch.tensor(z["img"]), training=False).numpy()
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    # the moving statistics matter: the training path on the same weights gives other logits
    train = cvt_ref.forward(kw, Pt, torch.tensor(z["img"]), training=True).numpy()
    assert np.abs(train - z["logits"]).max() > 1e-3
    assert np.abs(train - G.load("cvt_odd")["logits"]).max() <= F64_TOL


def test_fixture_files_stay_small():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_cvt_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 480 * 1024
    assert sum(os.path.getsize(f) for f in files) <= 2 * 1024 * 1024


def test_fixture_geometry_is_what_the_cases_claim():
    maps = lambda case: cvt_ref.maps_of(G.kwargs_of(case), *G.image_of(case))
    assert maps("cvt_tiny") == [((4, 4), (2, 2)), ((2, 2), (1, 1)), ((1, 1), (1, 1))]
    assert maps("cvt_odd") == [((5, 7), (3, 4)), ((5, 7), (3, 4)), ((3, 4), (2, 2))]
    assert maps("cvt_k5s3") == [((7, 10), (3, 4)), ((3, 4), (3, 4)), ((2, 2), (1, 1))]
    assert cvt_ref.same_pads(16, 7, 4) == (1, 2) and cvt_ref.same_pads(4, 3, 2) == (0, 1) and cvt_ref.same_pads(3, 5, 1) == (2, 2)
    assert cvt_ref.same_pads(4, 2, 2) == (0, 0) and cvt_ref.same_pads(3, 2, 2) == (0, 1) and cvt_ref.same_pads(7, 5, 3) == (2, 2)


@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 1, 1, 3), (2, 1, 1, 4)])
def test_batchnorm_extra_is_batch_norm(shape):
    """The generator's BatchNormalization against torch.nn.functional.batch_norm, in training and with given statistics."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, dtype=torch.float64, generator=g)
    c = shape[-1]
    layer = G.BatchNormalization(momentum=0.9, epsilon=1e-5)
    layer(x, training=True)
    gamma, beta = torch.randn(c, dtype=torch.float64, generator=g), torch.randn(c, dtype=torch.float64, generator=g)
    mean, var = torch.randn(c, dtype=torch.float64, generator=g), torch.rand(c, dtype=torch.float64, generator=g) + 0.5
    for v, t in ((layer.gamma, gamma), (layer.beta, beta), (layer.moving_mean, mean), (layer.moving_variance, var)):
        G.tf_shim.assign(v, t)
    xc = x.permute(0, 3, 1, 2)
    if x.numel() > c:
        want = F.batch_norm(xc, None, None, gamma, beta, training=True, eps=1e-5).permute(0, 2, 3, 1)
    else:     # one value per channel (torch refuses it): the deviation from the mean is zero, the output is beta
        want = beta.expand(shape)
    assert float((torch.as_tensor(layer(x, training=True)) - want).abs().max()) <= 1e-12
    want = F.batch_norm(xc, mean, var, gamma, beta, training=False, eps=1e-5).permute(0, 2, 3, 1)
    assert float((torch.as_tensor(layer(x, training=False)) - want).abs().max()) <= 1e-12
    assert float((torch.as_tensor(layer(x)) - want).abs().max()) <= 1e-12                 # Keras: no `training` means inference
    # the moving statistics are not updated by a training call
    assert torch.equal(torch.as_tensor(layer.moving_mean), mean) and torch.equal(torch.as_tensor(layer.moving_variance), var)


@pytest.mark.parametrize("H,W,k,s,groups", [
    (4, 6, 3, 2, 5), (4, 4, 3, 2, 1), (6, 8, 5, 3, 5), (8, 6, 7, 4, 1), (4, 6, 2, 2, 5), (7, 10, 5, 3, 5), (3, 4, 5, 1, 5), (2, 2, 1, 2, 5), (4, 6, 2, 3, 1)])
def test_conv_extra_is_the_strided_same_convolution(H, W, k, s, groups):
    """The generator's Conv2D against torch's conv2d on an explicitly, unevenly padded tensor: strides 2, 3 and 4, depthwise, even maps."""
    g = torch.Generator().manual_seed(H * 100 + W + k)
    cin = 5
    x = torch.randn(2, H, W, cin, dtype=torch.float64, generator=g)
    filters = cin if groups > 1 else 6
    layer = G.Conv2D(filters=filters, kernel_size=k, strides=s, padding="SAME", use_bias=False, groups=groups)
    got = layer(x)
    assert tuple(layer.kernel.shape) == (k, k, cin // groups, filters)
    pt, pb = cvt_ref.same_pads(H, k, s)
    pl, pr = cvt_ref.same_pads(W, k, s)
    assert pb - pt in (0, 1) and pr - pl in (0, 1)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    want = F.conv2d(xp, torch.as_tensor(layer.kernel).permute(3, 2, 0, 1), None, stride=s, groups=groups).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(want.shape) == (2, -(-H // s), -(-W // s), filters)
    assert float((torch.as_tensor(got) - want).abs().max()) <= 1e-13
    assert float((cvt_ref.conv_same(x, torch.as_tensor(layer.kernel), s, groups=groups) - want).abs().max()) <= 1e-13


def test_abi_symbols_exist():
    l = N.lib()
    for s in ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
              "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end"):
        assert hasattr(l, "vitx_cvt_" + s), s


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_restatements_and_the_generators(case):
    z, kw = G.load(case), G.kwargs_of(case)
    table = list(cvt.CvT(**kw)._table)
    assert [(n, tuple(s), o) for n, s, o in table] == cvt_ref.table_of(kw)
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]


def test_usage_configuration_table():
    """cvt.py:150-177,204-232: 1 + 2 + 10 blocks, heads of 64: inner 64 / 192 / 384 with the constructor's defaults (s3_heads = 6, every other
    value the usage block's); the usage block itself passes s3_heads = 4: inner 256 at stage 3."""
    m = cvt.CvT(num_classes=1000)
    table = [(n, tuple(s), o) for n, s, o in m._table]
    assert table == cvt_ref.table_of(dict(num_classes=1000))
    shapes = {n: s for n, s, _ in table}
    assert len([n for n in shapes if n.endswith(".attn.to_out.kernel")]) == 13
    assert shapes["cvt_layers.0.embed.kernel"] == (7, 7, 3, 64) and shapes["cvt_layers.1.embed.kernel"] == (3, 3, 64, 192)
    assert shapes["cvt_layers.0.transformer.0.attn.to_q.pw.kernel"] == (1, 1, 64, 64)
    assert shapes["cvt_layers.0.transformer.0.attn.to_out.kernel"] == (1, 1, 64, 64)        # to_out exists at heads 1, dim 64
    assert shapes["cvt_layers.1.transformer.1.attn.to_kv.pw.kernel"] == (1, 1, 192, 384)
    assert shapes["cvt_layers.2.transformer.9.attn.to_q.pw.kernel"] == (1, 1, 384, 384)
    assert shapes["cvt_layers.2.transformer.9.attn.to_kv.pw.kernel"] == (1, 1, 384, 768)
    assert shapes["cvt_layers.2.transformer.9.attn.to_kv.dw.kernel"] == (3, 3, 1, 384)
    assert shapes["cvt_layers.2.transformer.0.attn.to_kv.bn.moving_variance"] == (384,)
    assert shapes["cvt_layers.2.transformer.9.ff.fc1.kernel"] == (1, 1, 384, 1536) and shapes["head.kernel"] == (384, 1000)
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())
    assert m.maps_of(224, 224) == [((56, 56), (28, 28)), ((28, 28), (14, 14)), ((14, 14), (7, 7))]
    u = cvt.CvT(**cvt_ref.USAGE)
    assert [(n, tuple(s), o) for n, s, o in u._table] == cvt_ref.table_of(cvt_ref.USAGE)
    assert {n: s for n, s, _ in u._table}["cvt_layers.2.transformer.0.attn.to_q.pw.kernel"] == (1, 1, 384, 256)


def _vit_cfg(k=0, s=0, nest_block=1, global_k=0, H=4, W=6):
    c = N.Config()
    c.variant = N.VARIANT_VIT
    c.image_h, c.image_w = H, W
    c.patch_h = c.patch_w = 1
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 1, 1, 8, 2, 2, 16, 32
    c.pool, c.ln_eps, c.max_batch = N.POOL_CLS, 1e-5, 1
    c.nest_block, c.global_k, c.conv_proj_kernel, c.conv_proj_stride = nest_block, global_k, k, s
    return c


def test_flag_keeps_the_struct_and_a_cleared_flag_the_table():
    assert C.sizeof(N.Config) == 29 * 4
    assert N.Config.reserved.offset == 25 * 4 and N.Config.reserved.size == 16
    assert N.Config.conv_proj_kernel.offset == 28 * 4 and N.Config.conv_proj_stride.offset == 28 * 4 + 2
    assert N.Config.conv_proj_kernel.size == N.Config.conv_proj_stride.size == 2
    assert list(_vit_cfg(k=3, s=2).reserved) == [0, 1, 0, 3 | (2 << 16)]
    assert list(_vit_cfg(global_k=2).reserved) == [0, 1, 2, 0]
    plain = N.param_table(_vit_cfg())[0]
    flagged = N.param_table(_vit_cfg(k=3, s=2))[0]
    assert "transformer.0.attn.to_qkv.kernel" in [t[0] for t in plain]
    assert not any("to_q." in t[0] or "to_kv." in t[0] for t in plain)
    names = [t[0] for t in flagged]
    assert "transformer.0.attn.to_qkv.kernel" not in names
    at = names.index("transformer.1.attn.norm.beta")
    assert names[at + 1:at + 13] == [f"transformer.1.attn.{p}.{t}" for p in ("to_q", "to_kv")
                                     for t in ("dw.kernel", "bn.gamma", "bn.beta", "bn.moving_mean", "bn.moving_variance", "pw.kernel")]
    shapes = {t[0]: t[1] for t in flagged}
    assert shapes["transformer.1.attn.to_q.dw.kernel"] == (3, 3, 1, 8) and shapes["transformer.1.attn.to_kv.bn.moving_mean"] == (8,)
    assert shapes["transformer.1.attn.to_q.pw.kernel"] == (8, 32) and shapes["transformer.1.attn.to_kv.pw.kernel"] == (8, 64)
    assert [n for n in names if ".to_q." not in n and ".to_kv." not in n] == [t[0] for t in plain if "to_qkv" not in t[0]]


def test_flag_refusals():
    with pytest.raises(N.VitxError, match="conv_proj_kernel needs nest_block"):
        N.param_table(_vit_cfg(k=3, s=2, nest_block=0))
    with pytest.raises(N.VitxError, match="does not combine with global_k"):
        N.param_table(_vit_cfg(k=3, s=2, global_k=2))
    with pytest.raises(N.VitxError, match="both be positive or both be 0"):
        N.param_table(_vit_cfg(k=3, s=0))
    with pytest.raises(N.VitxError, match="both be positive or both be 0"):
        N.param_table(_vit_cfg(k=0, s=2))
    with pytest.raises(N.VitxError, match="both be positive or both be 0"):
        N.param_table(_vit_cfg(k=-1, s=-1))
    c = _vit_cfg(k=3, s=2)
    c.patch_h = c.patch_w = 2
    with pytest.raises(N.VitxError, match="patch_h == patch_w == 1"):
        N.param_table(c)
    N.param_table(_vit_cfg(k=3, s=4, H=5, W=7))     # unlike global_k, nothing has to divide


def test_constructor_and_call_refusals():
    kw = G.kwargs_of("cvt_tiny")
    m = cvt.CvT(**kw)
    with pytest.raises(ValueError, match="expected NHWC"):
        m(np.zeros((1, 8, 8, 4), np.float32))
    with pytest.raises(ValueError, match="multiple of 64"):                                   # before a device is looked for
        cvt.CvT(**kw, compute="bf16")
    with pytest.raises(TypeError, match="unexpected keyword"):
        cvt.CvT(**kw, dim_head=32)
    with pytest.raises(ValueError, match="s2: emb_dim"):
        cvt.CvT(**{**kw, "s2_kv_proj_stride": 0})
    with pytest.raises(ValueError, match="s3_depth"):
        cvt.CvT(**{**kw, "s3_depth": -1})
    cvt.CvT(**{**kw, "s1_depth": 0})                                                          # the reference runs a stage without blocks
    d = cvt.CvT(**kw, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        d(np.zeros((1, 8, 8, 3), np.float32))                       # training=True is the reference's default
    with pytest.raises(NotImplementedError, match="dropout"):
        d(np.zeros((1, 8, 8, 3), np.float32), training=True)
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()
    with pytest.raises(N.VitxError, match="no native handle"):
        m.params_dev()
    # the C table takes any image (nothing has to divide), refuses half an image size, and vitx_cvt_create a configuration without an image
    c = N.CvTConfig.from_buffer_copy(m._cfg)
    c.image_h, c.image_w = 9, 13
    N.cvt_param_table(c)
    c.image_h = 0
    with pytest.raises(N.VitxError, match="invalid image size"):
        N.cvt_param_table(c)
    c.image_w = 0
    h = C.c_void_p()
    assert N.lib().vitx_cvt_create(C.byref(c), C.byref(h)) == N.ERR_INVALID
    assert b"needs the image size" in N.lib().vitx_last_error()


def test_weights_api_round_trip(tmp_path):
    kw = G.kwargs_of("cvt_tiny")
    m = cvt.CvT(**kw, seed=1)
    sd = m.state_dict()
    moving = [n for n in sd if cvt_ref.is_moving(n)]
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd)
    assert len(moving) == 2 * 2 * 4                                    # four blocks, two projections each, two statistics
    # trainable_variables / trainable_weights leave the moving statistics out; weights, state_dict and save_weights keep them
    assert [w.name for w in m.trainable_variables] == [n for n in sd if n not in moving] == [w.name for w in m.trainable_weights]
    assert all(np.all(sd[n] == (1 if n.endswith("variance") else 0)) for n in moving)
    assert np.all(sd["cvt_layers.0.transformer.0.attn.norm.g"] == 1) and np.all(sd["head.bias"] == 0)
    assert np.all(sd["cvt_layers.1.transformer.0.attn.to_kv.bn.gamma"] == 1) and np.all(sd["cvt_layers.1.transformer.0.attn.to_kv.bn.beta"] == 0)
    k = sd["cvt_layers.2.transformer.1.attn.to_q.dw.kernel"]
    assert k.shape == (3, 3, 1, 8) and 0 < np.abs(k).max() <= np.sqrt(6.0 / (9 * 1 + 9 * 8)) + 1e-6
    k = sd["cvt_layers.0.embed.kernel"]
    assert k.shape == (7, 7, 3, 4) and 0 < np.abs(k).max() <= np.sqrt(6.0 / (49 * 3 + 49 * 4)) + 1e-6
    k = sd["cvt_layers.1.transformer.0.attn.to_kv.pw.kernel"]
    assert k.shape == (1, 1, 8, 256) and 0 < np.abs(k).max() <= np.sqrt(6.0 / (8 + 256)) + 1e-6
    # non-trivial moving statistics travel through set_weights / save_weights / load_weights / assign
    P = cvt_ref.init_params(cvt_ref.table_of(kw), seed=3)
    m.load_state_dict({n: v.astype(np.float32) for n, v in P.items()})
    m.save_weights(str(tmp_path / "w"))
    m2 = cvt.CvT(**kw, seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for (n, _, _), a, b in zip(m._table, m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b) and np.array_equal(a, P[n].astype(np.float32)), n
    name = "cvt_layers.2.transformer.0.attn.to_q.bn.moving_variance"
    w = [w for w in m2.weights if w.name == name][0]
    w.assign(np.full(w.shape, 2.5, np.float32))
    assert np.all(m2.state_dict()[name] == 2.5)
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in cvt_ref.table_of(kw))
