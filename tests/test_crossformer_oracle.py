"""crossformer, CPU tier: tests/crossformer_ref.py (float64 torch restatement) against tests/golden/ref_cf_*.npz, which
tools/gen_crossformer_fixtures.py produced by executing the reference's own crossformer.py; the generator's tf.stack / tf.meshgrid stand-ins
against numpy; the bias index arithmetic; the library's host-only parameter table against the restatement's own; the exported symbols; what
is refused without a device."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import crossformer_ref as R  # noqa: E402
import gen_crossformer_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import crossformer  # noqa: E402

F64_TOL = 1e-12
ABI = ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
       "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end")


def zero_gradient_names(kw):
    """Variables whose true gradient is zero: every dpb variable (crossformer.py:163 cuts the bias from the tape), and to_qkv's q and k thirds
    of a one-token window (softmax == 1 whatever q and k are) -- the kernel as a whole still gets the v third's gradient."""
    return {n for n, _, _ in R.table_of(kw) if R.is_dpb(n)}


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    logits, grads, dimg = R.forward_backward(kw, P, z["img"], z["dlogits"])
    assert z["img"].shape[1:3] == G.image_of(case) and z["img"].shape[0] == 2
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z if k.startswith("grad/"))
    zero = zero_gradient_names(kw)
    assert zero
    for n in P:
        ref = z["grad/" + n]
        assert ref.shape == P[n].shape, n
        if n in zero:
            assert np.all(ref == 0), n               # exact zeros: the reference's autograd returns None for them
            assert np.all(grads[n] == 0), n
        else:
            assert np.abs(ref).max() > 0, n          # every other variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


@pytest.mark.parametrize("case", list(G.CASES))
def test_fixture_pins_the_bias(case):
    """The generator's assertion, checked again on the committed file and through the restatement: without the position biases the logits
    move by at least 1e-2 of their spread."""
    z = G.load(case)
    assert float(z["bias_effect"]) >= 1e-2
    P = G.params_of(z)
    for n in P:
        if ".dpb.dense.3." in n:
            P[n] = np.zeros_like(P[n])
    Pt = {n: torch.tensor(v) for n, v in P.items()}
    logits = R.forward(G.kwargs_of(case), Pt, torch.tensor(z["img"])).numpy()
    spread = z["logits"].max() - z["logits"].min()
    assert np.abs(logits - z["logits"]).max() >= 1e-2 * spread


def test_one_token_window_qk_gradient_is_zero():
    """cf_rect, stage 3: local windows of one token -- the q and k thirds of to_qkv get nothing, the v third does."""
    z = G.load("cf_rect")
    g = z["grad/crossformer_layers.2.transformer.0.short_attn.to_qkv.kernel"]
    inner = g.shape[-1] // 3
    assert np.abs(g[..., :2 * inner]).max() <= 1e-14 and np.abs(g[..., 2 * inner:]).max() > 0


def test_fixture_files_stay_small():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_cf_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 512 * 1024


def test_stack_and_meshgrid_extras_agree_with_numpy():
    a, b = np.arange(-3, 4), np.arange(5)
    for indexing in ("ij", "xy"):
        got = G.meshgrid(torch.tensor(a), torch.tensor(b), indexing=indexing)
        want = np.meshgrid(a, b, indexing=indexing)
        assert isinstance(got, list) and len(got) == 2
        for g, w in zip(got, want):
            assert tuple(g.shape) == w.shape and np.array_equal(np.asarray(g), w)
    ij = G.meshgrid(torch.tensor(a), torch.tensor(a), indexing="ij")
    for axis in (0, 1, -1):
        got = G.stack(ij, axis=axis)
        want = np.stack(np.meshgrid(a, a, indexing="ij"), axis=axis)
        assert tuple(got.shape) == want.shape and np.array_equal(np.asarray(got), want)
    x = torch.randn(3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert np.array_equal(np.asarray(G.stack([x, 2 * x])), np.stack([x.numpy(), 2 * x.numpy()]))


@pytest.mark.parametrize("wsz", [1, 2, 3, 7, 8])
def test_bias_indices_are_the_references_asymmetric_ones(wsz):
    """Row stride 2 wsz - 1 (crossformer.py:131) into a table of (2 wsz + 1)^2 rows (:159-161): in range, and -- from wsz 2 on -- NOT the
    index of the relative position in that table."""
    idx = R.rel_pos_indices(wsz)
    n = wsz * wsz
    assert idx.shape == (n, n) and idx.min() >= 0 and idx.max() == (2 * wsz - 2) * 2 * wsz < (2 * wsz + 1) ** 2
    i, j = np.divmod(np.arange(n), wsz)
    dy, dx = i[:, None] - i[None, :], j[:, None] - j[None, :]
    assert np.array_equal(idx, (dy + wsz - 1) * (2 * wsz - 1) + dx + wsz - 1)
    symmetric = (dy + wsz) * (2 * wsz + 1) + dx + wsz          # where (dy, dx) sits in the table of positions -wsz .. wsz
    assert not np.array_equal(idx, symmetric)
    assert len(np.unique(idx)) == (2 * wsz - 1) ** 2           # still one table row per relative position


def test_window_partitions_are_the_einops_patterns():
    from einops import rearrange
    x = torch.arange(2 * 6 * 9 * 5, dtype=torch.float64).reshape(2, 6, 9, 5)
    s = R.to_short(x, 3)
    assert torch.equal(s, rearrange(x, "b (h s1) (w s2) d -> (b h w) s1 s2 d", s1=3, s2=3))
    assert torch.equal(R.from_short(s, 2, 6, 9), x)
    l = R.to_long(x, 3)
    assert torch.equal(l, rearrange(x, "b (l1 h) (l2 w) d -> (b h w) l1 l2 d", l1=3, l2=3))
    assert torch.equal(R.from_long(l, 2, 6, 9), x)
    assert not torch.equal(s, l)


def test_abi_symbols_exist_and_are_declared():
    l = N.lib()
    header = open(os.path.join(ROOT, "include", "vitx.h")).read()
    for s in ABI:
        assert hasattr(l, "vitx_crossformer_" + s), s
        assert re.search(r"int32_t vitx_crossformer_%s\(" % s, header), s
    assert "typedef struct vitx_crossformer_config" in header
    # the engine's configuration did not grow: the bias travels through engine fields
    assert C.sizeof(N.Config) == 29 * 4
    assert C.sizeof(N.CrossFormerConfig) == (3 + 4 * 4 + 4 + 4 * 8 + 4 + 4 + 8) * 4


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_restatements_and_the_generators(case):
    z, kw = G.load(case), G.kwargs_of(case)
    table = list(crossformer.CrossFormer(**kw)._table)
    assert [(n, tuple(s), o) for n, s, o in table] == R.table_of(kw)
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]


def test_usage_configuration_table():
    """crossformer.py:258-269: widths 64 .. 512, heads of 32, four scales at stage 1, dpb width dim // 4."""
    m = crossformer.CrossFormer(num_classes=1000)
    table = [(n, tuple(s), o) for n, s, o in m._table]
    assert table == R.table_of(dict(num_classes=1000))
    shapes = {n: s for n, s, _ in table}
    assert [shapes[f"crossformer_layers.0.cel.convs.{i}.kernel"] for i in range(4)] == [(4, 4, 3, 32), (8, 8, 3, 16), (16, 16, 3, 8), (32, 32, 3, 8)]
    assert shapes["crossformer_layers.1.cel.convs.1.kernel"] == (4, 4, 64, 64)
    assert shapes["crossformer_layers.2.transformer.7.long_attn.to_qkv.kernel"] == (1, 1, 256, 768)
    assert shapes["crossformer_layers.3.transformer.1.short_attn.dpb.dense.0.kernel"] == (2, 128)
    assert shapes["crossformer_layers.3.transformer.1.short_attn.dpb.dense.3.kernel"] == (128, 1)
    assert shapes["to_logits.kernel"] == (512, 1000)
    assert "crossformer_layers.2.transformer.8.short_attn.norm.g" not in shapes
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())
    assert m.maps_of(224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    sd = m.state_dict()
    assert np.all(sd["crossformer_layers.0.transformer.0.short_attn.dpb.norm.1.gamma"] == 1) and np.all(sd["to_logits.bias"] == 0)
    k = sd["crossformer_layers.0.transformer.0.long_attn.dpb.dense.0.kernel"]
    assert 0 < np.abs(k).max() <= np.sqrt(6.0 / (2 + 16)) + 1e-6


def test_kernel_sizes_are_sorted_and_widths_follow_the_reference():
    kw = dict(dim=48, depth=0, cross_embed_kernel_sizes=((8, 3, 4), (4, 2), (3,), (4, 2)), cross_embed_strides=1, num_classes=2)
    shapes = {n: s for n, s, _ in crossformer.CrossFormer(**kw)._table}
    assert [shapes[f"crossformer_layers.0.cel.convs.{i}.kernel"] for i in range(3)] == [(3, 3, 3, 24), (4, 4, 3, 12), (8, 8, 3, 12)]
    assert shapes["crossformer_layers.2.cel.convs.0.kernel"] == (3, 3, 48, 48)
    assert [(n, tuple(s), o) for n, s, o in crossformer.CrossFormer(**kw)._table] == R.table_of(kw)


def test_constructor_and_call_refusals():
    """Every refusal raises with its text before a device is looked for."""
    kw = G.kwargs_of("cf_rect")
    for k in ("dim", "depth", "global_window_size", "local_window_size", "cross_embed_kernel_sizes", "cross_embed_strides"):
        with pytest.raises(ValueError, match=k + " must be a scalar or a tuple of 4"):
            crossformer.CrossFormer(**{**kw, k: kw[k][:3]})
    m = crossformer.CrossFormer(**kw)
    with pytest.raises(ValueError, match=r"stage 1: the map \(6 x 11\) must be divisible by local_window_size = 3"):
        m(np.zeros((1, 24, 44, 3), np.float32))
    with pytest.raises(ValueError, match=r"stage 3: the map \(4 x 6\) must be divisible by global_window_size = 3"):
        crossformer.CrossFormer(**{**kw, "local_window_size": (1, 2, 1, 1)})(np.zeros((1, 32, 48, 3), np.float32))
    with pytest.raises(ValueError, match="global_window_size = 3"):
        crossformer.CrossFormer(**{**kw, "local_window_size": (1, 2, 1, 1)}, image_size=(32, 48))     # the eager form refuses at construction
    with pytest.raises(ValueError, match=r"dim must be >= 32 \(heads = dim // 32 would be 0"):
        crossformer.CrossFormer(**{**kw, "dim": (48, 64, 31, 32)})
    with pytest.raises(ValueError, match="a window of more than 288 tokens"):
        crossformer.CrossFormer(**{**kw, "local_window_size": 17})
    with pytest.raises(ValueError, match="a window of more than 288 tokens"):
        crossformer.CrossFormer(**{**kw, "global_window_size": (2, 1, 3, 18)})
    with pytest.raises(ValueError, match="multiple of 64"):
        crossformer.CrossFormer(**kw, compute="bf16")
    with pytest.raises(ValueError, match="expected NHWC"):
        m(np.zeros((1, 24, 48, 4), np.float32))
    with pytest.raises(TypeError, match="unexpected keyword"):
        crossformer.CrossFormer(**kw, dim_head=64)
    crossformer.CrossFormer(**kw, attn_dropout=0.3)                     # accepted and unused, as in the reference
    d = crossformer.CrossFormer(**kw, ff_dropout=0.1)
    with pytest.raises(NotImplementedError, match="ff_dropout=0.1"):
        d(np.zeros((1, 24, 48, 3), np.float32))                         # training=True is the reference's default
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()
    # the C table refuses the same geometry, and vitx_crossformer_create a configuration without an image
    c = N.CrossFormerConfig.from_buffer_copy(m._cfg)
    c.image_h, c.image_w = 24, 48
    N.crossformer_param_table(c)
    c.image_w = 44
    with pytest.raises(N.VitxError, match="local_window_size = 3"):
        N.crossformer_param_table(c)
    c.image_h = 0
    with pytest.raises(N.VitxError, match="invalid image size"):
        N.crossformer_param_table(c)
    c.image_w = 0
    h = C.c_void_p()
    assert N.lib().vitx_crossformer_create(C.byref(c), C.byref(h)) != N.OK
    assert "needs the image size" in N.lib().vitx_last_error().decode()


def test_weights_api_round_trip(tmp_path):
    kw = G.kwargs_of("cf_usage_windows")
    m = crossformer.CrossFormer(**kw, seed=1)
    sd = m.state_dict()
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd)
    m.save_weights(str(tmp_path / "w"))
    m2 = crossformer.CrossFormer(**kw, seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
