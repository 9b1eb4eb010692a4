"""CPU tier: the host side of the long-sequence attention switch (vitx_set_long_attn, ViT(..., long_attn=...)).  No device is touched: the
constructor refusals come from the configuration alone."""
import os
import re
import subprocess
import sys

import pytest

from vit_tensorflow import ViT
from vit_tensorflow import _native as N
from vit_tensorflow import parallel_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(image_size=(16, 18), patch_size=1, num_classes=5, dim=64, depth=1, heads=2, mlp_dim=64, dim_head=64)


def test_setter_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vitx.h")).read()
    assert re.search(r"int32_t\s+vitx_set_long_attn\s*\(\s*vitx_handle\s+h\s*,\s*int32_t\s+on\s*\)\s*;", header)
    assert "vit.py:73-82" in header[header.index("vitx_set_long_attn") - 1500:header.index("vitx_set_long_attn")]
    fn = N.lib().vitx_set_long_attn          # bound by _native with its argument types
    assert fn.restype is not None and len(fn.argtypes) == 2


def test_null_handle_is_refused_on_the_host():
    assert N.lib().vitx_set_long_attn(None, 1) == N.ERR_INVALID


@pytest.mark.parametrize("compute", ["fp32", "bf16x3"])
def test_long_attn_needs_bf16(compute):
    with pytest.raises(ValueError, match="bf16"):
        ViT(**KW, compute=compute, long_attn=True)
    with pytest.raises(ValueError, match="bf16"):
        parallel_vit.ViT(**KW, compute=compute, long_attn=True)


def test_long_attn_needs_dim_head_64():
    with pytest.raises(ValueError, match="dim_head"):
        ViT(**dict(KW, dim_head=32), compute="bf16", long_attn=True)


def test_long_attn_is_vit_only():
    from vit_tensorflow.deepvit import DeepViT
    with pytest.raises(ValueError, match="ViT"):
        DeepViT(**KW, compute="bf16", long_attn=True)


def test_flag_off_builds_the_same_parameter_table():
    a = ViT(**KW, compute="bf16", seed=3)
    b = ViT(**KW, compute="bf16", seed=3, long_attn=False)
    c = ViT(**KW, compute="bf16", seed=3, long_attn=True)      # the flag is no parameter: the same table either way
    for m in (b, c):
        assert m._table == a._table and m._n == a._n
        assert (m._blob == a._blob).all()
    assert a._handle is None and b._handle is None and c._handle is None   # nothing was created on a device


def test_chunk_loops_of_the_streamed_kernels_keep_their_loads_in_flight():
    """tools/isa_check.py over the object the library is linked from: in every chunk loop, read in run order from the issue of the next chunk's
    LDS-DMA, no s_waitcnt vmcnt in front of the last LDS read of the iteration (such a wait drains the chunk in flight), no scratch access, no M0
    write but the DMA statements' own."""
    obj = os.path.join(ROOT, "vit-tensorflow_amd", "build", "attn_stream.o")
    if not os.path.exists(obj):   # library came pre-built without its objects: rebuild them
        sys.path.insert(0, os.path.join(ROOT, "vit-tensorflow_amd"))
        import build as _b
        _b.build(force=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), obj], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 3, r.stdout + r.stderr          # forward, d(q), d(k, v)
    assert r.returncode == 0 and all(l.startswith("ok") for l in lines), r.stdout + r.stderr
