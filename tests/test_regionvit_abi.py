"""regionvit, CPU tier: the vitx_regionvit_* family is exported, declared in include/vitx.h and bound, and the existing structures kept their
layout (the per-head bias and its gradient travel through vitx_engine fields, not through vitx_config)."""
import ctypes as C
import os
import re

from vit_tensorflow import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("param_table_size", "param_table_entry", "create", "destroy", "set_params", "get_params", "get_grads", "params_dev", "grads_dev",
       "params_changed", "forward", "forward_dev", "backward", "backward_dev", "read", "profile_begin", "profile_end", "attn", "partition")


def test_abi_symbols_exist_and_are_declared():
    l = N.lib()
    header = open(os.path.join(ROOT, "include", "vitx.h")).read()
    bound = {s[0] for s in N.SYMBOLS}
    for s in ABI:
        assert hasattr(l, "vitx_regionvit_" + s), s
        assert re.search(r"int32_t vitx_regionvit_%s\(" % s, header), s
        assert "vitx_regionvit_" + s in bound, s
    assert "typedef struct vitx_regionvit_config" in header


def test_existing_structures_keep_their_layout():
    assert C.sizeof(N.Config) == 29 * 4
    assert C.sizeof(N.CrossFormerConfig) == (3 + 4 * 4 + 4 + 4 * 8 + 4 + 4 + 8) * 4
    assert C.sizeof(N.RegionViTConfig) == (3 + 4 + 4 + 4 + 4 + 1 + 7) * 4
    f = dict((n, getattr(N.RegionViTConfig, n).offset) for n, _ in N.RegionViTConfig._fields_)
    assert f["dim"] == 12 and f["depth"] == 28 and f["window_size"] == 44 and f["ln_eps"] == 60 and f["window_attn"] == 76


def test_host_only_table_call_needs_no_device():
    cfg = N.RegionViTConfig()
    cfg.num_classes = 3
    for i in range(4):
        cfg.dim[i], cfg.depth[i] = 32, 1
    cfg.window_size, cfg.local_patch_size = 7, 4
    table, n = N.regionvit_param_table(cfg)
    assert table[0][0] == "local_encoder.kernel" and table[-1][0] == "to_logits.bias"
    assert n == sum(int(__import__("numpy").prod(s)) for _, s, _ in table)
