"""vit_for_small_dataset, CPU tier: tests/small_dataset_ref.py (float64 torch restatement) against tests/golden/ref_sd_*.npz, which
tools/gen_small_dataset_fixtures.py produced by executing the reference's own vit_for_small_dataset.py; the library's host-only parameter
table with the flag set and clear; the usage configuration's size; what vitx_create refuses."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import small_dataset_ref  # noqa: E402
import gen_small_dataset_fixtures as G  # noqa: E402
from oracle import gen_ref_fixtures  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402

F64_TOL = 1e-12
USAGE_KW = dict(image_size=256, patch_size=16, num_classes=1000, dim=1024, depth=6, heads=16, mlp_dim=2048, dropout=0.1,
                emb_dropout=0.1)   # vit_for_small_dataset.py:218-228


def _load(case):
    return np.load(os.path.join(ROOT, "tests", "golden", f"ref_{case}.npz"))


def _cfg(small_dataset=1, variant=N.VARIANT_VIT, image=(16, 16), patch=(4, 4), dim=32, depth=2, heads=2, dim_head=16, mlp_dim=48, num_classes=5,
         branches=0, pool=N.POOL_CLS):
    c = N.Config()
    c.variant = variant
    c.image_h, c.image_w = image
    c.patch_h, c.patch_w = patch
    c.channels, c.num_classes, c.dim, c.depth, c.heads, c.dim_head, c.mlp_dim = 3, num_classes, dim, depth, heads, dim_head, mlp_dim
    c.pool, c.ln_eps, c.max_batch, c.num_parallel_branches, c.patch_merge_num_tokens = pool, 1e-3, 1, branches, 8
    c.small_dataset = small_dataset
    return c


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = _load(case)
    P = G.params_of(z, case)
    logits, grads, dimg = small_dataset_ref.forward_backward(G.kwargs_of(case), P, z["img"], z["dlogits"])
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z.files if k.startswith("grad/"))
    for n in P:
        ref = z["grad/" + n]
        if case == "sd_2tok" and n.endswith("temperature"):
            assert np.abs(ref).max() == 0    # one live key per row: P = 1 whatever the scale, so the temperature gets exactly no gradient
        else:
            assert np.abs(ref).max() > 0, n  # every other variable of the reference received a gradient (each temperature included)
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


def test_fixture_weights_are_off_their_defaults():
    z = _load("sd_small")
    P = G.params_of(z, "sd_small")
    assert np.abs(P["patch_embedding.norm.gamma"] - 1).min() > 0 and np.abs(P["patch_embedding.norm.beta"]).min() > 0
    t = [float(P[f"transformer.{l}.attn.temperature"][0]) for l in range(2)]
    assert t[0] != t[1] and all(abs(v - np.log(16 ** -0.5)) > 1e-3 for v in t)


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_generators(case):
    z = _load(case)
    table = small_dataset_ref.table_of(G.kwargs_of(case))
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]
    off = 0
    for _, s, o in table:
        assert o == off
        off += int(np.prod(s))


def test_table_order_with_the_flag_set():
    table, n = N.param_table(_cfg())
    names = [t[0] for t in table]
    shapes = {t[0]: tuple(t[1]) for t in table}
    feat = 5 * 4 * 4 * 3
    assert names[:6] == ["pos_embedding", "cls_token", "patch_embedding.norm.gamma", "patch_embedding.norm.beta", "patch_embedding.kernel",
                         "patch_embedding.bias"]
    assert shapes["patch_embedding.norm.gamma"] == shapes["patch_embedding.norm.beta"] == (feat,)
    assert shapes["patch_embedding.kernel"] == (feat, 32)
    for l in range(2):
        i = names.index(f"transformer.{l}.attn.norm.beta")
        assert names[i + 1] == f"transformer.{l}.attn.temperature" and names[i + 2] == f"transformer.{l}.attn.to_qkv.kernel"
        assert shapes[f"transformer.{l}.attn.temperature"] == (1,)


def test_table_with_the_flag_clear_is_the_plain_vit():
    """The flag came out of `reserved`: same struct size, and a cleared flag gives the plain ViT's table (oracle/spec.py is the statement of
    that table the other CPU tests already pin)."""
    from oracle import spec
    assert C.sizeof(N.Config) == 29 * 4
    assert N.Config.small_dataset.offset == 24 * 4 and N.Config.reserved.offset == 25 * 4 and N.Config.reserved.size == 16
    table, n = N.param_table(_cfg(small_dataset=0))
    names = [t[0] for t in table]
    assert not [x for x in names if "temperature" in x or "patch_embedding.norm" in x]
    assert names[:4] == ["pos_embedding", "cls_token", "patch_embedding.kernel", "patch_embedding.bias"]
    cfg = spec.make_config(variant="vit", image_size=16, patch_size=4, num_classes=5, dim=32, depth=2, heads=2, mlp_dim=48, dim_head=16)
    assert [(t[0], tuple(t[1])) for t in table] == [(nm, tuple(sh)) for nm, sh, _ in spec.param_spec(cfg)]


def test_usage_configuration_size():
    """Parameter count from the reference's layer shapes (vit_for_small_dataset.py:182-195, 94-102, 77-82, 146-150)."""
    from vit_tensorflow.vit_for_small_dataset import ViT
    v = ViT(**USAGE_KW)
    d, m, inner, nc, feat, np_ = 1024, 2048, 16 * 64, 1000, 5 * 16 * 16 * 3, 256
    layer = 2 * d + 1 + d * 3 * inner + inner * d + d + 2 * d + d * m + m + m * d + d
    want = (np_ + 1) * d + d + 2 * feat + feat * d + d + 6 * layer + 2 * d + d * nc + nc
    assert v.count_params() == want
    t = [w for w in v.weights if w.name.endswith("temperature")]
    assert len(t) == 6 and all(abs(float(w.numpy()[0]) - np.log(64 ** -0.5)) < 1e-6 for w in t)
    assert np.all(v.state_dict()["patch_embedding.norm.gamma"] == 1) and np.all(v.state_dict()["patch_embedding.norm.beta"] == 0)


def test_assertion_texts_and_square_patch():
    from vit_tensorflow.vit_for_small_dataset import ViT
    kw = dict(num_classes=3, dim=16, depth=1, heads=1, mlp_dim=16, dim_head=16)
    with pytest.raises(AssertionError, match='Image dimensions must be divisible by the patch size.'):
        ViT(image_size=30, patch_size=4, **kw)
    with pytest.raises(AssertionError, match='pool type must be either cls \\(cls token\\) or mean \\(mean pooling\\)'):
        ViT(image_size=16, patch_size=4, pool='max', **kw)
    with pytest.raises(AssertionError, match='square'):
        ViT(image_size=16, patch_size=(4, 8), **kw)


def _create_fails(c):
    h = C.c_void_p()
    rc = N.lib().vitx_create(C.byref(c), C.byref(h))
    assert rc != N.OK
    return rc, N.lib().vitx_last_error().decode()


def test_create_refusals():
    rc, msg = _create_fails(_cfg(patch=(4, 8), image=(16, 16)))
    assert rc == N.ERR_INVALID and "square" in msg
    for variant in (N.VARIANT_CAIT, N.VARIANT_DEEPVIT):
        rc, msg = _create_fails(_cfg(variant=variant))
        assert rc == N.ERR_INVALID and "ViT variant" in msg
    rc, msg = _create_fails(_cfg(branches=2))
    assert rc == N.ERR_INVALID and "num_parallel_branches" in msg
    rc, msg = _create_fails(_cfg(dim_head=24))
    assert rc == N.ERR_UNSUPPORTED and "dim_head" in msg and "288" in msg
    rc, msg = _create_fails(_cfg(image=(72, 72), patch=(4, 4)))      # 325 tokens
    assert rc == N.ERR_UNSUPPORTED and "288" in msg and "325" in msg
    # the tokenizer alone (SPT, depth 0) has no attention and no LSA limit: whatever else happens (no device here, a handle where there is one),
    # the config is not refused as unsupported or invalid
    h = C.c_void_p()
    rc = N.lib().vitx_create(C.byref(_cfg(image=(72, 72), patch=(4, 4), depth=0)), C.byref(h))
    assert rc not in (N.ERR_UNSUPPORTED, N.ERR_INVALID)
    if rc == N.OK:
        N.lib().vitx_destroy(h)


def test_untested_paths_refuse():
    from vit_tensorflow.vit_for_small_dataset import ViT
    v = ViT(image_size=8, patch_size=4, num_classes=3, dim=16, depth=1, heads=1, mlp_dim=16, dim_head=16)
    for fn in (v.comm_init, v.apply_gradients, v.forward_patches):
        with pytest.raises(NotImplementedError):
            fn()
    # the wrappers refuse such an encoder when they are constructed (before any device is needed)
    from vit_tensorflow.mae import MAE
    from vit_tensorflow.simmim import SimMIM
    from vit_tensorflow.mpp import MPP
    from vit_tensorflow.distill import DistillWrapper
    with pytest.raises(NotImplementedError, match="vit_for_small_dataset"):
        MAE(image_size=8, encoder=v, decoder_dim=16, masking_ratio=0.5)
    with pytest.raises(NotImplementedError, match="vit_for_small_dataset"):
        SimMIM(image_size=8, encoder=v, masking_ratio=0.5)
    with pytest.raises(NotImplementedError, match="vit_for_small_dataset"):
        MPP(image_size=8, transformer=v, patch_size=4)
    with pytest.raises(AssertionError, match="student must be a vision transformer"):
        DistillWrapper(teacher=None, student=v)
    # ... and so do the attributes an efficient.ViT shell or hand-written wrapper code would borrow
    with pytest.raises(NotImplementedError):
        v.patch_embedding.layers
    with pytest.raises(NotImplementedError):
        v.transformer(np.zeros((1, 5, 16), np.float32))
    with pytest.raises(NotImplementedError):
        v.mlp_head(np.zeros((1, 16), np.float32))


@pytest.mark.skipif(not os.path.isdir(gen_ref_fixtures.REF), reason="the reference's sources are not staged under oracle/_ref (build() stages them where a reference checkout exists)")
@pytest.mark.parametrize("case", list(G.CASES))
def test_committed_fixture_is_what_the_reference_source_produces(case):
    """Re-run the reference's vit_for_small_dataset.py under the shim in a fresh interpreter and compare with the committed file bit for bit."""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "import gen_small_dataset_fixtures as G\n"
        "d = G.make(%r); z = np.load(%r)\n"
        "assert sorted(d) == sorted(z.files), sorted(set(d) ^ set(z.files))\n"
        "bad = [k for k in d if not np.array_equal(np.asarray(d[k]), z[k])]\n"
        "assert not bad, bad\n"
    ) % (os.path.join(ROOT, "tools"), case, os.path.join(ROOT, "tests", "golden", f"ref_{case}.npz"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
