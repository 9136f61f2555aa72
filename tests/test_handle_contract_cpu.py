"""The five encoder handles' refusals that need no GPU: what every exported entry point answers to a NULL handle or a NULL config, code and
full avexhip_last_error() text.  The host plumbing around the handles (csrc/handle_core.h) is shared; the texts are each family's own and
part of the C contract (BEATs' accessors say "overflow_count: ...", without a family prefix: they are older than the prefixes)."""
import ctypes as C

import numpy as np
import pytest

from avex_amd import _capi, kernels as K, synth

FAMILIES = ("beats", "eat", "aves", "effnet", "stack")
U32 = C.c_uint32


def _config(family):
    """A config the family accepts (the create calls below are refused before it is read)."""
    if family == "beats":
        return K.make_beats_config(synth.BEATS_BASE_CFG)
    if family == "eat":
        c = _capi.EatConfig()
        c.embed_dim, c.num_heads, c.depth, c.ffn_dim, c.patch_size, c.target_length, c.n_mels = 768, 12, 1, 3072, 16, 1024, 128
        c.norm_eps, c.norm_mean, c.norm_std = 1e-6, -4.268, 4.569
        return c
    if family == "aves":
        c = _capi.AvesConfig()
        c.embed_dim, c.num_heads, c.num_layers, c.ffn_dim, c.pos_conv_kernel, c.pos_conv_groups, c.n_conv_layers = 768, 12, 1, 3072, 128, 16, 7
        for i, (k, s) in enumerate(((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2))):
            c.conv_kernel[i], c.conv_stride[i] = k, s
        return c
    if family == "effnet":
        c = _capi.EffnetConfig()
        c.n_stages = len(synth.EFFNET_B0_STAGES)
        for i, st in enumerate(synth.EFFNET_B0_STAGES):
            for j in range(6):
                c.stage[i][j] = int(st[j])
        c.stem_channels, c.head_channels, c.bn_eps = 32, 1280, 1e-5
        return c
    c = _capi.StackConfig()
    c.embed_dim, c.num_heads, c.num_layers, c.ffn_dim, c.norm_eps, c.activation, c.residual_dtype = 128, 2, 1, 128, 1e-5, 3, 1
    return c


def _call(fn, *args):
    return fn(*args), _capi.last_error()


@pytest.mark.parametrize("family", FAMILIES)
def test_create_refuses_a_null_config_and_a_missing_device(built_lib, family):
    lib = built_lib
    create = getattr(lib, f"avexhip_{family}_create")
    arr, n, keep = K.tensor_table({"some.weight": np.zeros(4, np.float32)})
    h, msg = _call(create, None, arr, n)
    assert not h and msg == f"{family}_create: null config or empty weight table"
    cfg = _config(family)
    h, msg = _call(create, C.byref(cfg), None, 1)
    assert not h and msg == f"{family}_create: null config or empty weight table"
    h, msg = _call(create, C.byref(cfg), arr, 0)
    assert not h and msg == f"{family}_create: null config or empty weight table"
    if lib.avexhip_device_count() <= 0:      # (with a device this call would go on to read the table: tests/test_gpu_handle_contract.py)
        h, msg = _call(create, C.byref(cfg), arr, n)
        assert not h and msg == f"{family}_create: no HIP device visible (this path has no CPU fallback)"
    del keep


FORWARD_NULL = {
    "beats": (lambda lib: lib.avexhip_beats_forward(None, None, 1, 16000, 16000, None, 0, None, 0, None, None, None, 0, None),
              "beats_forward: null handle or input"),
    "eat": (lambda lib: lib.avexhip_eat_forward(None, None, 1, 16000, 16000, None, 0, None, 0, None, None, 0, None, 0, None),
            "eat_forward: give exactly one of wav / spec"),
    "aves": (lambda lib: lib.avexhip_aves_forward(None, None, 1, 16000, 16000, None, 0, None, 0, None, None, None, 0, None),
             "aves_forward: null handle or input"),
    "effnet": (lambda lib: lib.avexhip_effnet_forward(None, None, 1, 64, 64, 0, None, None, None, None, 0, None),
               "effnet_forward: null handle or input"),
    "stack": (lambda lib: lib.avexhip_stack_forward(None, None, 1, 16, None, None, None, None, 0, None),
              "stack_forward: null handle / input or empty batch"),
}


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_refuses_a_null_handle(built_lib, family):
    call, text = FORWARD_NULL[family]
    assert _call(call, built_lib) == (-1, text)


def test_beats_other_entry_points_refuse_a_null_handle(built_lib):
    lib = built_lib
    assert _call(lib.avexhip_beats_forward_fbank, None, None, 1, 96, None, 0, None, 0, None, None, None, 0, None) == \
        (-1, "beats_forward_fbank: null handle or input")
    g, msg = _call(lib.avexhip_beats_graph_capture, None, None, 1, 16000, 16000, None, 0, None, 0, None, None, None, 0, None)
    assert not g and msg == "beats_graph_capture: null handle / input or empty batch"
    assert _call(lib.avexhip_beats_overflow_reset, None, None) == (-1, "overflow_reset: null handle")
    assert _call(lib.avexhip_beats_graph_launch, None, None) == (-1, "beats_graph_launch: null graph")
    assert lib.avexhip_beats_graph_nodes(None) == 0


@pytest.mark.parametrize("family", FAMILIES)
def test_accessors_refuse_a_null_handle(built_lib, family):
    lib = built_lib
    prefix = "" if family == "beats" else family + "_"      # BEATs' accessors carry no family prefix in their texts
    n = U32(7)
    assert _call(getattr(lib, f"avexhip_{family}_overflow_count"), None, C.byref(n), None, 0) == (-1, f"{prefix}overflow_count: null argument")
    assert n.value == 7
    if family == "stack":      # the layer stack exports no profiling accessors
        assert not hasattr(lib, "avexhip_stack_set_profiling") and not hasattr(lib, "avexhip_stack_last_profile")
        return
    assert _call(getattr(lib, f"avexhip_{family}_set_profiling"), None, 1) == (-1, f"{prefix}set_profiling: null handle")
    names, ms, fl, cnt = C.POINTER(C.c_char_p)(), C.POINTER(C.c_float)(), C.POINTER(C.c_double)(), C.c_int(7)
    assert _call(getattr(lib, f"avexhip_{family}_last_profile"), None, C.byref(names), C.byref(ms), C.byref(fl), C.byref(cnt)) == \
        (-1, f"{prefix}last_profile: null argument")
    assert cnt.value == 7


def test_sizes_of_a_null_handle_are_zero(built_lib):
    lib = built_lib
    assert lib.avexhip_beats_workspace_bytes(None, 2, 16000) == 0 and lib.avexhip_beats_num_tokens(None, 16000) == 0
    assert lib.avexhip_eat_workspace_bytes(None, 2) == 0 and lib.avexhip_eat_num_tokens(None) == 0
    assert lib.avexhip_aves_workspace_bytes(None, 2, 16000) == 0 and lib.avexhip_aves_num_tokens(None, 16000) == 0
    assert lib.avexhip_effnet_workspace_bytes(None, 2, 64, 64) == 0 and lib.avexhip_effnet_num_taps(None) == 0
    assert lib.avexhip_stack_workspace_bytes(None, 2, 16) == 0
