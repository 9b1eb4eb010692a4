"""regionvit, CPU tier: tests/regionvit_ref.py (float64 torch restatement) against tests/golden/ref_rv_*.npz, which
tools/gen_regionvit_fixtures.py produced by executing the reference's own regionvit.py; the generator's tf.pad / tf.convert_to_tensor
stand-ins against numpy; the bias index table against a direct numpy statement; the library's host-only parameter table against the
restatement's own; what is refused without a device."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import regionvit_ref as R  # noqa: E402
import gen_regionvit_fixtures as G  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402
from vit_tensorflow import regionvit  # noqa: E402

F64_TOL = 1e-12


def zero_embeddings(kw):
    """Embeddings whose true gradient is exactly zero: those of the stages without layers (off the tape: the reference returns None), and that
    of the last stage with layers when its depth is 1 (its only layer's local tokens reach nothing)."""
    depths = R.config_of(kw)["depth"]
    last = max(s for s in range(4) if depths[s] > 0)
    return {f"region_layers.{s}.transformer.local_rel_pos_bias" for s in range(4) if depths[s] == 0 or (s == last and depths[s] == 1)}


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = G.load(case)
    P = G.params_of(z)
    kw = G.kwargs_of(case)
    logits, grads, dimg = R.forward_backward(kw, P, z["img"], z["dlogits"])
    assert z["img"].shape[1:3] == G.image_of(case) and z["img"].shape[0] == 2
    assert np.abs(logits - z["logits"]).max() <= F64_TOL * max(1.0, np.abs(z["logits"]).max())
    assert sorted("grad/" + n for n in P) == sorted(k for k in z if k.startswith("grad/"))
    zero = zero_embeddings(kw)
    assert zero or case == "rv_bf16"          # (rv_bf16: every embedding receives a gradient)
    for n in P:
        ref = z["grad/" + n]
        assert ref.shape == P[n].shape, n
        if n in zero:
            assert np.all(ref == 0) and np.all(grads[n] == 0), n    # exact zeros
        else:
            assert np.abs(ref).max() > 0, n                          # every other variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(z["dimg"]).max() > 0
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


def test_fixtures_pin_what_they_were_made_for():
    z = G.load("rv_bf16")     # last stage two layers deep: its embedding gradient is non-zero
    assert np.abs(z["grad/region_layers.3.transformer.local_rel_pos_bias"]).max() > 0
    z = G.load("rv_w14")      # 197- and 50-token stages, then two stages without layers
    assert [np.any(z[f"grad/region_layers.{s}.transformer.local_rel_pos_bias"]) for s in range(4)] == [True, False, False, False]
    assert [w[0] * w[1] + 1 for *_, w in R.maps_of(G.kwargs_of("rv_w14"), 56, 56)][:2] == [197, 50]
    assert [w for *_, w in R.maps_of(G.kwargs_of("rv_rect"), 28, 56)] == [(7, 7), (4, 7), (2, 4), (1, 2)]
    assert [r[0] * r[1] for _, r, _ in R.maps_of(G.kwargs_of("rv_small"), 64, 64)] == [64, 16, 4, 1]
    assert R.maps_of(G.kwargs_of("rv_lps2"), 32, 32)[0][2] == (2, 2)
    # rows of the embedding tables rv_rect touches: (2 wh - 1)(2 ww - 1)
    for s, rows in enumerate((169, 91, 21)):
        g = z = G.load("rv_rect")[f"grad/region_layers.{s}.transformer.local_rel_pos_bias"]
        assert int(np.any(g != 0, axis=1).sum()) == rows, s


@pytest.mark.parametrize("case", list(G.CASES))
def test_fixture_pins_the_embeddings(case):
    """The generator's assertion, checked again on the committed file and through the restatement: without the embeddings the logits move by
    at least 1e-2 of their spread."""
    z = G.load(case)
    assert float(z["bias_effect"]) >= 1e-2
    P = G.params_of(z)
    for n in P:
        if R.is_embedding(n):
            P[n] = np.zeros_like(P[n])
    Pt = {n: torch.tensor(v) for n, v in P.items()}
    logits = R.forward(G.kwargs_of(case), Pt, torch.tensor(z["img"])).numpy()
    spread = z["logits"].max() - z["logits"].min()
    moved = np.abs(logits - z["logits"]).max()
    assert moved >= 1e-2 * spread and abs(moved / spread - float(z["bias_effect"])) <= 1e-9


def test_fixture_files_stay_small():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "ref_rv_*.npz"))
    assert len(files) >= len(G.CASES)
    assert max(os.path.getsize(f) for f in files) <= 512 * 1024


def test_pad_and_convert_to_tensor_extras_agree_with_numpy():
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float64).reshape(2, 3, 4, 5)
    for paddings in ([[0, 0], [0, 0], [1, 0], [1, 0]], [[1, 2], [0, 0], [0, 3], [2, 1]], [[0, 0]] * 4):
        got = G.pad(torch.tensor(x), paddings=paddings)
        want = np.pad(x, paddings)
        assert tuple(got.shape) == want.shape and np.array_equal(np.asarray(got), want)
    got = G.pad(torch.tensor(x[0, 0]), [[1, 0], [0, 2]], constant_values=7)
    assert np.array_equal(np.asarray(got), np.pad(x[0, 0], [[1, 0], [0, 2]], constant_values=7))
    t = G.convert_to_tensor([1, 13])
    assert tuple(t.shape) == (2,) and np.array_equal(np.asarray(t), np.array([1, 13])) and not t.dtype.is_floating_point
    assert np.array_equal(np.asarray(t[:, None, None] * torch.ones(2, 3, 3, dtype=torch.long)), np.array([1, 13])[:, None, None] * np.ones((2, 3, 3), np.int64))
    assert np.array_equal(np.asarray(G.convert_to_tensor(np.float64(2.5))), np.float64(2.5))


@pytest.mark.parametrize("geom", [(7, 7, 7), (2, 2, 2), (4, 7, 7), (2, 4, 7), (1, 2, 7), (2, 2, 4), (14, 14, 14), (1, 1, 3)])
def test_bias_indices_against_a_direct_numpy_statement(geom):
    """(dh + ws - 1) + (dw + ws - 1)(2 ws - 1) with ws = window_size, for square and rectangular windows and windows smaller than
    window_size: the reference's grid arithmetic (regionvit.py:144-152) stated with numpy's meshgrid."""
    wh, ww, ws = geom
    gy, gx = np.meshgrid(np.arange(wh), np.arange(ww), indexing="ij")
    grid = np.stack([gy, gx]).reshape(2, -1)
    rel = grid[:, :, None] - grid[:, None, :] + ws - 1
    want = (rel * np.array([1, 2 * ws - 1])[:, None, None]).sum(0)
    idx = R.bias_indices(wh, ww, ws)
    assert idx.shape == (wh * ww, wh * ww) and np.array_equal(idx, want)
    assert idx.min() >= 0 and idx.max() < (2 * ws - 1) ** 2
    assert len(np.unique(idx)) == (2 * wh - 1) * (2 * ww - 1)
    emb = torch.arange((2 * ws - 1) ** 2 * 4, dtype=torch.float64).reshape(-1, 4) + 1
    b = R.position_bias(emb, wh, ww, ws).numpy()
    assert b.shape == (4, 1 + wh * ww, 1 + wh * ww) and np.all(b[:, 0] == 0) and np.all(b[:, :, 0] == 0)
    assert np.array_equal(b[:, 1:, 1:], np.moveaxis(emb.numpy()[want], -1, 0))


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_restatements_and_the_generators(case):
    z, kw = G.load(case), G.kwargs_of(case)
    table = list(regionvit.RegionViT(**kw)._table)
    assert [(n, tuple(s), o) for n, s, o in table] == R.table_of(kw)
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]


def test_usage_configuration_table():
    """regionvit.py:265-277: widths 64 .. 512, 4 heads of 32 at every width, one embedding of 169 rows per stage."""
    m = regionvit.RegionViT(num_classes=1000)
    table = [(n, tuple(s), o) for n, s, o in m._table]
    assert table == R.table_of(dict(num_classes=1000))
    shapes = {n: s for n, s, _ in table}
    assert shapes["local_encoder.kernel"] == (8, 8, 3, 64) and shapes["region_encoder.1.kernel"] == (1, 1, 3 * 28 * 28, 64)
    assert shapes["region_layers.1.down.conv.kernel"] == (3, 3, 64, 128) and "region_layers.0.down.conv.kernel" not in shapes
    assert shapes["region_layers.2.transformer.local_rel_pos_bias"] == (169, 4)
    assert shapes["region_layers.2.transformer.7.attn.to_qkv.kernel"] == (256, 384) and shapes["region_layers.3.transformer.1.attn.to_out.kernel"] == (128, 512)
    assert shapes["region_layers.3.transformer.1.ff.fc1.kernel"] == (512, 2048) and "region_layers.2.transformer.8.attn.norm.gamma" not in shapes
    assert shapes["to_logits.kernel"] == (512, 1000) and "region_layers.1.peg.proj.kernel" not in shapes
    assert m.count_params() == sum(int(np.prod(s)) for s in shapes.values())
    assert m.maps_of(224, 224) == [((56, 56), (8, 8), (7, 7)), ((28, 28), (4, 4), (7, 7)), ((14, 14), (2, 2), (7, 7)), ((7, 7), (1, 1), (7, 7))]
    assert m.maps_of(224, 224) == R.maps_of(dict(num_classes=1000), 224, 224)
    sd = m.state_dict()
    assert np.all(sd["region_layers.0.transformer.0.attn.norm.gamma"] == 1) and np.all(sd["to_logits.bias"] == 0)
    e = sd["region_layers.0.transformer.local_rel_pos_bias"]
    assert 0 < np.abs(e).max() <= 0.05
    peg = regionvit.RegionViT(num_classes=10, use_peg=True, tokenize_local_3_conv=True)
    assert [(n, tuple(s), o) for n, s, o in peg._table] == R.table_of(dict(num_classes=10, use_peg=True, tokenize_local_3_conv=True))


def test_constructor_and_call_refusals():
    """Every refusal raises with its text before a device is looked for."""
    kw = G.kwargs_of("rv_small")
    for k in ("dim", "depth"):
        with pytest.raises(ValueError, match=k + " needs to be a single value or a tuple of length 4"):
            regionvit.RegionViT(**{**kw, k: kw[k][:3]})
    m = regionvit.RegionViT(**G.kwargs_of("rv_rect"))
    with pytest.raises(ValueError, match="height and width must be divisible by region patch size"):
        m(np.zeros((1, 28, 60, 3), np.float32))
    with pytest.raises(ValueError, match="height and width must be divisible by region patch size"):
        regionvit.RegionViT(**G.kwargs_of("rv_rect"), image_size=(30, 56))         # the eager form refuses at construction
    # 84 x 84 at window_size 7: local 21 -> 11, region 3 -> 2: 11 % 2
    with pytest.raises(ValueError, match=r"stage 2: the region map \(2 x 2\) and the local map \(11 x 11\) do not cut into windows"):
        m(np.zeros((1, 84, 84, 3), np.float32))
    # local_patch_size 2 at window_size 2 (region patch 4): the stride-4 local map is as large as the region map, then larger windows never
    # appear; local_patch_size 8 gives 2 x 2 ... windows of 4 x 4 > window_size 2
    with pytest.raises(ValueError, match=r"stage 1: a 4 x 4 window leaves the position table of window_size = 2"):
        regionvit.RegionViT(dim=32, depth=1, window_size=2, local_patch_size=8, num_classes=2)(np.zeros((1, 32, 32, 3), np.float32))
    with pytest.raises(ValueError, match="a window plus its region token of more than 288 tokens"):
        regionvit.RegionViT(dim=32, depth=1, window_size=17, num_classes=2)(np.zeros((1, 68, 68, 3), np.float32))
    with pytest.raises(ValueError, match=r"a region sequence of more than 288 tokens is not built \(324\)"):
        regionvit.RegionViT(dim=32, depth=1, window_size=2, num_classes=2)(np.zeros((1, 144, 144, 3), np.float32))
    with pytest.raises(ValueError, match="multiple of 64"):
        regionvit.RegionViT(**kw, compute="bf16")
    with pytest.raises(ValueError, match="expected NHWC"):
        m(np.zeros((1, 28, 56, 4), np.float32))
    with pytest.raises(TypeError, match="unexpected keyword"):
        regionvit.RegionViT(**kw, dim_head=64)
    regionvit.RegionViT(**kw, attn_dropout=0.3)                     # accepted and unused, as in the reference
    d = regionvit.RegionViT(**kw, ff_dropout=0.1)
    with pytest.raises(NotImplementedError, match="ff_dropout=0.1"):
        d(np.zeros((1, 64, 64, 3), np.float32))                     # training=True is the reference's default
    for refused in (m.comm_init, m.optimizer_step, m.capture_graph):
        with pytest.raises(NotImplementedError):
            refused()
    # the C table refuses the same geometry, and vitx_regionvit_create a configuration without an image
    c = N.RegionViTConfig.from_buffer_copy(m._cfg)
    c.image_h, c.image_w = 28, 56
    N.regionvit_param_table(c)
    c.image_w = 60
    with pytest.raises(N.VitxError, match="divisible by region patch size"):
        N.regionvit_param_table(c)
    c.image_h = 0
    with pytest.raises(N.VitxError, match="invalid image size"):
        N.regionvit_param_table(c)
    c.image_w = 0
    h = C.c_void_p()
    assert N.lib().vitx_regionvit_create(C.byref(c), C.byref(h)) != N.OK
    assert "needs the image size" in N.lib().vitx_last_error().decode()


def test_weights_api_round_trip(tmp_path):
    kw = G.kwargs_of("rv_small")
    m = regionvit.RegionViT(**kw, seed=1)
    sd = m.state_dict()
    assert list(sd) == [t[0] for t in m._table] and len(m.weights) == len(sd)
    m.save_weights(str(tmp_path / "w"))
    m2 = regionvit.RegionViT(**kw, seed=2)
    m2.load_weights(str(tmp_path / "w"))
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
