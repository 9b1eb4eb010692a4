"""CrossViT, CPU tier: tests/crossvit_ref.py (float64 torch restatement) against tests/golden/ref_crossvit_*.npz, which
tools/gen_crossvit_fixtures.py produced by executing the reference's own cross_vit.py; the library's host-only parameter table against
the generator's; the README configuration's size; the reference's assertion text."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import crossvit_ref  # noqa: E402
import gen_crossvit_fixtures as G  # noqa: E402
from oracle import gen_ref_fixtures  # noqa: E402
from vit_tensorflow import _native as N  # noqa: E402

F64_TOL = 1e-12
README_KW = dict(image_size=256, num_classes=1000, depth=4, sm_dim=192, sm_patch_size=16, sm_enc_depth=2, sm_enc_heads=8, sm_enc_mlp_dim=2048,
                 lg_dim=384, lg_patch_size=64, lg_enc_depth=3, lg_enc_heads=8, lg_enc_mlp_dim=2048, cross_attn_depth=2, cross_attn_heads=8,
                 dropout=0.1, emb_dropout=0.1)   # README.md:325-342


def _load(case):
    return np.load(os.path.join(ROOT, "tests", "golden", f"ref_{case}.npz"))


def _cfg_struct(kw):
    kw = {**crossvit_ref.DEFAULTS, **kw}
    c = N.CrossViTConfig()
    for k in ("image_size", "num_classes", "sm_dim", "lg_dim", "sm_patch_size", "sm_enc_depth", "sm_enc_heads", "sm_enc_mlp_dim", "sm_enc_dim_head",
              "lg_patch_size", "lg_enc_depth", "lg_enc_heads", "lg_enc_mlp_dim", "lg_enc_dim_head", "cross_attn_depth", "cross_attn_heads",
              "cross_attn_dim_head", "depth"):
        setattr(c, k, int(kw[k]))
    return c


@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_reproduces_reference_fixture(case):
    z = _load(case)
    P = G.params_of(z)
    logits, grads, dimg = crossvit_ref.forward_backward(G.kwargs_of(case), P, z["img"], z["dlogits"])
    assert np.abs(logits - z["logits"]).max() <= F64_TOL
    assert sorted("grad/" + n for n in P) == sorted(k for k in z.files if k.startswith("grad/"))
    for n in P:
        ref = z["grad/" + n]
        assert np.abs(ref).max() > 0, n          # every variable of the reference received a gradient
        assert np.abs(grads[n] - ref).max() <= F64_TOL * max(1.0, np.abs(ref).max()), n
    assert np.abs(dimg - z["dimg"]).max() <= F64_TOL * max(1.0, np.abs(z["dimg"]).max())


@pytest.mark.parametrize("case", list(G.CASES))
def test_library_table_is_the_generators(case):
    z = _load(case)
    table, n = N.crossvit_param_table(_cfg_struct(G.kwargs_of(case)))
    assert [t[0] for t in table] == [str(s) for s in z["names"]]
    assert [",".join(str(s) for s in t[1]) for t in table] == [str(s) for s in z["shapes"]]
    off = 0
    for _, s, o in table:
        assert o == off
        off += int(np.prod(s))
    assert off == n


def test_readme_configuration_size():
    from vit_tensorflow.cross_vit import CrossViT
    v = CrossViT(**README_KW)
    assert v.count_params() == 55152912
    assert len(v.weights) == 432
    names = [w.name for w in v.weights]
    assert names[:4] == ["sm_image_embedder.pos_embedding", "sm_image_embedder.cls_token", "sm_image_embedder.patch_embedding.kernel",
                         "sm_image_embedder.patch_embedding.bias"]
    assert names[-1] == "lg_mlp_head.bias"


def test_bad_patch_size_carries_the_reference_message():
    from vit_tensorflow.cross_vit import CrossViT
    with pytest.raises(AssertionError, match='Image dimensions must be divisible by the patch size.'):
        CrossViT(image_size=250, num_classes=10, sm_dim=32, lg_dim=64, sm_patch_size=10, lg_patch_size=16)
    c = _cfg_struct(dict(image_size=250, num_classes=10, sm_dim=32, lg_dim=64, sm_patch_size=10, lg_patch_size=16))
    import ctypes as C
    nt, ne = C.c_int64(), C.c_int64()
    assert N.lib().vitx_crossvit_param_table_size(C.byref(c), C.byref(nt), C.byref(ne)) == N.ERR_INVALID
    assert N.lib().vitx_last_error().decode() == 'Image dimensions must be divisible by the patch size.'


def test_out_of_scope_paths_refuse():
    from vit_tensorflow.cross_vit import CrossViT
    v = CrossViT(image_size=32, num_classes=3, sm_dim=16, lg_dim=32, sm_patch_size=8, lg_patch_size=16)
    for fn in (v.comm_init, v.optimizer_step, v.capture_graph):
        with pytest.raises(NotImplementedError):
            fn()


@pytest.mark.skipif(not os.path.isdir(gen_ref_fixtures.REF), reason="the reference's sources are not staged under oracle/_ref (build() stages them where a reference checkout exists)")
@pytest.mark.parametrize("case", list(G.CASES))
def test_committed_fixture_is_what_the_reference_source_produces(case):
    """Re-run the reference's cross_vit.py under the shim in a fresh interpreter and compare with the committed file bit for bit."""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "import gen_crossvit_fixtures as G\n"
        "d = G.make(%r); z = np.load(%r)\n"
        "assert sorted(d) == sorted(z.files), sorted(set(d) ^ set(z.files))\n"
        "bad = [k for k in d if not np.array_equal(np.asarray(d[k]), z[k])]\n"
        "assert not bad, bad\n"
    ) % (os.path.join(ROOT, "tools"), case, os.path.join(ROOT, "tests", "golden", f"ref_{case}.npz"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
