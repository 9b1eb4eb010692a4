"""Class-row form of the last block (csrc/engine.hip, block_forward_cls_rows / block_backward_cls_rows): under pool='cls' the head reads row 0 of
every image only, so everything of the last block behind its attention runs on the b class rows, and the attention kernels compute query row 0.
VITX_LAST_BLOCK_FULL=1 (read per forward) is the full form, with the bits of the library before this form existed.

What must hold: the logits, d(img) and every parameter gradient have the bits of the full form, except eight tensors of the last block (the
out-projection, fc1 and fc2 kernels and biases, LayerNorm 2's gamma and beta), which sum the same b nonzero fp32 terms in another order."""
import numpy as np
import pytest

from oracle import spec

pytestmark = pytest.mark.gpu

WIDTH = dict(num_classes=10, dim=128, heads=2, dim_head=64, mlp_dim=256)
TOKENS = {17: dict(image_size=32, patch_size=8),      # one query block
          65: dict(image_size=64, patch_size=8),      # dead query blocks, a dead tile pair in the dK / dV pass
          197: dict(image_size=224, patch_size=16)}   # the flagship's token count (14-tile kernels)

# Gate of the eight reassociated tensors, relative to the tensor's largest magnitude: 8 x the largest difference observed over CASES on MI355X
# (OBSERVED_REASSOC, first passing GPU run of this file).  As a condition, not a measurement, it must stay below 1e-4: a dropped or doubled row at these batches
# is 1e-2 or more, plain reassociation of at most 65 fp32 terms is around 1e-6.
OBSERVED_REASSOC = 1.667e-7   # 17 tokens, depth 2, batch 65: fc2 bias
REASSOC_GATE = 8 * OBSERVED_REASSOC
assert REASSOC_GATE < 1e-4


def eight(depth):
    p = f"transformer.{depth - 1}."
    return {p + "attn.to_out.kernel", p + "attn.to_out.bias", p + "mlp.norm.gamma", p + "mlp.norm.beta", p + "mlp.fc1.kernel", p + "mlp.fc1.bias",
            p + "mlp.fc2.kernel", p + "mlp.fc2.bias"}


def make(ntok, depth, max_batch, cls=None, **over):
    from vit_tensorflow import ViT
    kw = dict(WIDTH, **TOKENS[ntok], depth=depth)
    kw.update(over)
    okw = {k: v for k, v in kw.items() if k not in ("dropout", "emb_dropout")}
    P = spec.init_params(spec.make_config("vit", **okw), 1, randomize_all=True)
    m = (cls or ViT)(**kw, compute="bf16", max_batch=max_batch, seed=0)
    m.load_state_dict({k: v.astype(np.float32) for k, v in P.items()})
    return m, kw


def inputs(kw, b, seed=0, hw=None):
    rng = np.random.default_rng(seed)
    s = hw or kw["image_size"]
    img = rng.standard_normal((b, s, s, 3)).astype(np.float32)
    dl = (rng.standard_normal((b, kw["num_classes"])) / 2).astype(np.float32)
    return img, dl


def form(m):
    return int(m.debug_read("last_block_form", 0)[0])


def step(m, monkeypatch, full, img, dl, want_form=None):
    if full:
        monkeypatch.setenv("VITX_LAST_BLOCK_FULL", "1")
    else:
        monkeypatch.delenv("VITX_LAST_BLOCK_FULL", raising=False)
    logits = np.array(m(img, training=False))
    if want_form is not None:
        assert form(m) == want_form
    g, dimg = m.backward(dl, want_dimg=True)
    return logits, {k: np.array(v) for k, v in g.items()}, np.array(dimg)


def compare(got, ref, depth, what=""):
    """got: class-row form, ref: full form.  Returns the largest relative difference seen in the eight reassociated tensors."""
    assert np.array_equal(got[0], ref[0]), f"{what} logits"
    assert np.array_equal(got[2], ref[2]), f"{what} dimg"
    worst = 0.0
    for k in ref[1]:
        if k in eight(depth):
            den = float(np.abs(ref[1][k]).max())
            assert den > 0, k
            err = float(np.abs(got[1][k] - ref[1][k]).max()) / den
            worst = max(worst, err)
            print(f"[reassoc] {what} {k}: {err:.3e}")
            assert err <= REASSOC_GATE, (what, k, err)
        else:
            assert np.array_equal(got[1][k], ref[1][k]), f"{what} {k}"
    return worst


CASES = [(ntok, depth, b) for ntok in (17, 65, 197) for depth in (1, 2) for b in (1, 3, 65)]


@pytest.mark.parametrize("ntok,depth,b", CASES)
def test_class_row_form_equals_full_form(monkeypatch, ntok, depth, b):
    m, kw = make(ntok, depth, b)
    img, dl = inputs(kw, b)
    full = step(m, monkeypatch, True, img, dl, want_form=0)
    got = step(m, monkeypatch, False, img, dl, want_form=1)
    worst = compare(got, full, depth, f"{ntok}tok d{depth} b{b}")
    print(f"[reassoc] worst {worst:.3e} (gate {REASSOC_GATE:.1e})")
    # backward twice after one forward: the same gradients again
    g2, dimg2 = m.backward(dl, want_dimg=True)
    for k in g2:
        assert np.array_equal(g2[k], got[1][k]), k
    assert np.array_equal(dimg2, got[2])


@pytest.mark.parametrize("ntok,b", [(17, 3), (65, 3), (197, 1)])
def test_one_and_two_launch_attention_backward_agree_in_class_row_form(monkeypatch, ntok, b):
    m, kw = make(ntok, 2, b)
    img, dl = inputs(kw, b, seed=3)
    got = []
    for split in ("0", "1"):
        monkeypatch.setenv("VITX_ATTN_BWD_SPLIT", split)
        got.append(step(m, monkeypatch, False, img, dl, want_form=1))
    for k in got[0][1]:
        assert np.array_equal(got[0][1][k], got[1][1][k]), k
    assert np.array_equal(got[0][2], got[1][2])


@pytest.mark.parametrize("depth", [1, 2])
def test_debug_reads_of_the_last_block_complete_it(monkeypatch, depth):
    m, kw = make(65, depth, 3)
    img, dl = inputs(kw, 3, seed=4)
    last = depth - 1
    names = ("act", "hpre", "attn_out", "x_out", "x_mid", "y2")
    monkeypatch.setenv("VITX_LAST_BLOCK_FULL", "1")
    logits_full = np.array(m(img, training=False))
    want = {n: m.debug_read(n, last) for n in names}
    g_full, dimg_full = m.backward(dl, want_dimg=True)
    g_full = {k: np.array(v) for k, v in g_full.items()}
    monkeypatch.delenv("VITX_LAST_BLOCK_FULL")
    for first in names:   # whichever tensor is read first triggers the completion
        logits = np.array(m(img, training=False))
        assert form(m) == 1
        assert np.array_equal(logits, logits_full)
        for n in (first,) + names:
            assert np.array_equal(m.debug_read(n, last), want[n]), (first, n)
        assert form(m) == 0
        g, dimg = m.backward(dl, want_dimg=True)   # the full form: every gradient bit for bit
        for k in g_full:
            assert np.array_equal(g[k], g_full[k]), (first, k)
        assert np.array_equal(dimg, dimg_full)
    # reads that need no completion leave the form alone
    m(img, training=False)
    for n in ("x_in", "y1", "qkv"):
        m.debug_read(n, last)
    assert form(m) == 1


def test_form_is_not_taken_for_mean_pooling_dropout_or_a_distillation_token(monkeypatch):
    from vit_tensorflow.distill import DistillableViT
    # mean pooling
    m, kw = make(17, 2, 3, pool="mean")
    img, dl = inputs(kw, 3, seed=5)
    a = step(m, monkeypatch, False, img, dl, want_form=0)
    f = step(m, monkeypatch, True, img, dl, want_form=0)
    assert np.array_equal(a[0], f[0]) and np.array_equal(a[2], f[2]) and all(np.array_equal(a[1][k], f[1][k]) for k in f[1])
    # dropout > 0 in a training forward (an evaluation forward of the same handle has no dropout and takes the form)
    m, kw = make(17, 2, 3, dropout=0.1)
    outs = []
    for full in (False, True):
        if full:
            monkeypatch.setenv("VITX_LAST_BLOCK_FULL", "1")
        else:
            monkeypatch.delenv("VITX_LAST_BLOCK_FULL", raising=False)
        logits = np.array(m(img, training=True, seed=11))
        assert form(m) == 0
        g, dimg = m.backward(dl, want_dimg=True)
        outs.append((logits, {k: np.array(v) for k, v in g.items()}, np.array(dimg)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][2], outs[1][2])
    assert all(np.array_equal(outs[0][1][k], outs[1][1][k]) for k in outs[1][1])
    monkeypatch.delenv("VITX_LAST_BLOCK_FULL")
    m(img, training=False)
    assert form(m) == 1
    # a distillable forward with a distillation token
    m, kw = make(17, 2, 3, cls=DistillableViT)
    tok = np.random.default_rng(6).standard_normal((1, 1, kw["dim"])).astype(np.float32)
    dd = np.random.default_rng(7).standard_normal((3, kw["dim"])).astype(np.float32)
    outs = []
    for full in (False, True):
        if full:
            monkeypatch.setenv("VITX_LAST_BLOCK_FULL", "1")
        else:
            monkeypatch.delenv("VITX_LAST_BLOCK_FULL", raising=False)
        logits, dtok = m(img, distill_token=tok, training=False)
        assert form(m) == 0
        g, dt = m.backward_distill(dl, dd)
        outs.append((np.array(logits), np.array(dtok), {k: np.array(v) for k, v in g.items()}, np.array(dt)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][3], outs[1][3])
    assert all(np.array_equal(outs[0][2][k], outs[1][2][k]) for k in outs[1][2])
    monkeypatch.delenv("VITX_LAST_BLOCK_FULL")
    m(img, training=False)   # the same handle without a token: the form applies again
    assert form(m) == 1


def test_geometry_changes_between_steps(monkeypatch):
    """Batch 3, 1, 3, then a smaller image, on one handle in each form: the compact buffers' rows >= b are K padding of the weight gradients and
    must read as zero after every change (re-zeroed with the other activation buffers)."""
    ma, kw = make(65, 2, 3)
    mf, _ = make(65, 2, 3)
    for i, (b, hw) in enumerate([(3, None), (1, None), (3, None), (3, 32), (2, 32), (3, None)]):
        img, dl = inputs(kw, b, seed=20 + i, hw=hw)
        got = step(ma, monkeypatch, False, img, dl, want_form=1)
        ref = step(mf, monkeypatch, True, img, dl, want_form=0)
        compare(got, ref, 2, f"step {i} b{b} hw{hw}")
