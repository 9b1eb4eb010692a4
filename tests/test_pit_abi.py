"""pit, CPU tier: the vitx_pit_* family is exported, declared in include/vitx.h and bound, and the existing structures kept their layout
(a PiT stage is an ordinary vitx_config engine: nothing was added to vitx_config)."""
import ctypes as C
import os
import re

import numpy as np

from vit_tensorflow import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
       "params_changed", "set_long_attn", "forward", "forward_dev", "backward", "backward_dev", "pool_forward", "pool_backward", "read",
       "profile_begin", "profile_end")


def test_abi_symbols_exist_and_are_declared():
    l = N.lib()
    header = open(os.path.join(ROOT, "include", "vitx.h")).read()
    bound = {s[0] for s in N.SYMBOLS}
    for s in ABI:
        assert hasattr(l, "vitx_pit_" + s), s
        assert re.search(r"int32_t vitx_pit_%s\(" % s, header), s
        assert "vitx_pit_" + s in bound, s
    assert "typedef struct vitx_pit_config" in header
    assert sorted(n for n in bound if n.startswith("vitx_pit_")) == sorted("vitx_pit_" + s for s in ABI)


def test_existing_structures_keep_their_layout():
    assert C.sizeof(N.Config) == 29 * 4
    assert C.sizeof(N.CrossFormerConfig) == (3 + 4 * 4 + 4 + 4 * 8 + 4 + 4 + 8) * 4
    assert C.sizeof(N.RegionViTConfig) == (3 + 4 + 4 + 4 + 4 + 1 + 7) * 4
    assert C.sizeof(N.PiTConfig) == (7 + 2 * 8 + 3 + 1 + 3 + 1 + 8) * 4
    f = dict((n, getattr(N.PiTConfig, n).offset) for n, _ in N.PiTConfig._fields_)
    assert f["image_size"] == 8 and f["depth"] == 28 and f["heads"] == 60 and f["mlp_dim"] == 92 and f["ln_eps"] == 104 and f["long_attn"] == 120


def test_host_only_table_call_needs_no_device():
    cfg = N.PiTConfig()
    cfg.image_size, cfg.patch_size, cfg.num_classes, cfg.dim, cfg.n_stages = 32, 8, 3, 16, 2
    cfg.depth[0], cfg.depth[1], cfg.heads[0], cfg.heads[1] = 1, 0, 2, 2
    cfg.mlp_dim, cfg.dim_head, cfg.pool_stages = 24, 8, 1
    table, n = N.pit_param_table(cfg)
    names = [t[0] for t in table]
    assert names[:4] == ["patch_embedding.kernel", "patch_embedding.bias", "pos_embedding", "cls_token"] and names[-1] == "mlp_head.bias"
    assert "pool.0.cls_ff.bias" in names and not any(s.startswith("stage.1.") for s in names)    # a stage of depth 0 has no layers
    assert dict((t[0], t[1]) for t in table)["mlp_head.norm.gamma"] == (32,)
    assert n == sum(int(np.prod(s)) for _, s, _ in table)
