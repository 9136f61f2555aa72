"""The contract the five encoder handles share, on the smallest handles (synthetic checkpoints, one layer, B = 2): the refusals of
*_forward and *_create that need a device (code and full avexhip_last_error() text; every one is an argument check that returns before
the first launch), the profile's stage list, the range alarm after a clean forward, close() twice.  The texts and stage lists are the
library's as it stood before the handles' host plumbing was gathered into csrc/handle_core.h; they are each family's own."""
import ctypes as C

import numpy as np
import pytest
import torch

from avex_amd import _capi, kernels as K, synth
from avex_amd.aves_encoder import AvesEncoder
from avex_amd.eat_encoder import EatEncoder
from avex_amd.effnet_encoder import EfficientNetB0Encoder
from test_handle_contract_cpu import _call, _config

pytestmark = pytest.mark.gpu
B = 2
SENTINEL = 7.0

# stage names of last_profile() for the forwards of `Case` below, in order of first appearance
STAGES = {
    "beats": ["fbank", "gemm.patch_embed", "layernorm", "gemm.post_extract_proj", "posconv", "gemm.qkv", "attention", "gemm.out_proj", "gemm.fc1",
              "gemm.fc2"],
    "eat": ["fbank", "gemm.patch_embed", "token_embed_ln", "gemm.qkv", "attention", "gemm.out_proj", "gemm.fc1", "gemm.fc2", "layernorm"],
    "aves": ["wavconv0", "gemm.conv1", "gemm.conv2", "gemm.conv3", "gemm.conv4", "gemm.conv5", "gemm.conv6", "layernorm", "gemm.feature_projection",
             "posconv", "gemm.qkv", "attention", "gemm.out_proj", "gemm.fc1", "gemm.fc2"],
    "effnet": ["stem", "dwconv", "se", "gemm.project", "mbconv.front", "gemm.expand", "gemm.head"],
}
# (noun of "bits beyond <noun> <last>", what a selected hook is called, number of hooks) of the one-layer handles
HOOKS = {"beats": ("layer", "hook", 2), "eat": ("block", "hook", 1), "aves": ("layer", "hook", 1), "effnet": ("tap", "tap", 17)}


class Case:
    """One family's smallest handle: the wrapper, its input, and the raw C forward with everything valid but what a test overrides."""

    def __init__(self, family):
        self.family = family
        dev = torch.device("cuda", torch.cuda.current_device())
        wav = torch.from_numpy(synth.noise_clips(B, 16000, seed=21)).to(dev)
        if family == "beats":
            cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=1)
            self.enc, self.x, self.out_shape = K.BeatsEncoder(cfg, synth.beats_state_dict(cfg, seed=5)), wav, (B, 48, 768)
            assert self.enc.num_tokens(16000) == 48
            self.need = int(_capi.lib().avexhip_beats_workspace_bytes(self.enc._h, B, 16000))
        elif family == "eat":
            cfg = dict(synth.EAT_BASE_CFG, depth=1)
            self.enc, self.x, self.out_shape = EatEncoder(cfg, synth.eat_state_dict(cfg)), wav, (B, 513, 768)
            self.need = int(_capi.lib().avexhip_eat_workspace_bytes(self.enc._h, B))
        elif family == "aves":
            cfg = dict(synth.AVES_BASE_CFG, encoder_num_layers=1)
            self.enc, self.x, self.out_shape = AvesEncoder(cfg, synth.aves_state_dict(cfg)), wav, (B, 49, 768)
            assert self.enc.num_tokens(16000) == 49
            self.need = int(_capi.lib().avexhip_aves_workspace_bytes(self.enc._h, B, 16000))
        elif family == "effnet":
            self.enc = EfficientNetB0Encoder(synth.effnet_b0_state_dict())
            self.x = torch.from_numpy(np.abs(synth.normal("contract_mel", (B, 64, 64), 0.5)).astype(np.float32)).to(dev)
            self.out_shape = (B,) + self.enc._shape(-1, 64, 64)
            self.need = int(_capi.lib().avexhip_effnet_workspace_bytes(self.enc._h, B, 64, 64))
        else:
            cfg = _config("stack")
            g = torch.Generator().manual_seed(4)
            E, F = cfg.embed_dim, cfg.ffn_dim
            p = "layers.0."
            table = {p + "self_attn.in_proj.weight": torch.randn(3 * E, E, generator=g) * 0.05, p + "self_attn.in_proj.bias": torch.zeros(3 * E),
                     p + "self_attn.out_proj.weight": torch.randn(E, E, generator=g) * 0.05, p + "self_attn.out_proj.bias": torch.zeros(E),
                     p + "norm1.weight": torch.ones(E), p + "norm1.bias": torch.zeros(E),
                     p + "linear1.weight": torch.randn(F, E, generator=g) * 0.05, p + "linear1.bias": torch.zeros(F),
                     p + "linear2.weight": torch.randn(E, F, generator=g) * 0.05, p + "linear2.bias": torch.zeros(E),
                     p + "norm2.weight": torch.ones(E), p + "norm2.bias": torch.zeros(E)}
            self.enc = K.EncoderHandle("stack")
            self.enc._create(cfg, table)
            self.x, self.out_shape = torch.randn(B, 16, E, generator=g).to(dev), (B, 16, E)
            self.need = int(_capi.lib().avexhip_stack_workspace_bytes(self.enc._h, B, 16))
        assert self.need > 0
        self.ws = torch.empty((self.need,), dtype=torch.uint8, device=dev)
        self.out = torch.full(self.out_shape, SENTINEL, dtype=torch.float32, device=dev)

    def raw_forward(self, mask=0, hook_out=None, ws_bytes=None):
        """(code, message) of the C forward on the wrapper's handle, features into ``self.out``."""
        lib, h, x, s = _capi.lib(), self.enc._h, K._ptr(self.x), K._stream()
        out, ws, nws = K._ptr(self.out), K._ptr(self.ws), self.need if ws_bytes is None else ws_bytes
        if self.family == "beats":
            return _call(lib.avexhip_beats_forward, h, x, B, 16000, 16000, None, mask, hook_out, 0, out, None, ws, nws, s)
        if self.family == "eat":
            return _call(lib.avexhip_eat_forward, h, x, B, 16000, 16000, None, mask, hook_out, 0, out, None, 0, ws, nws, s)
        if self.family == "aves":
            return _call(lib.avexhip_aves_forward, h, x, B, 16000, 16000, None, mask, hook_out, 0, out, None, ws, nws, s)
        if self.family == "effnet":
            return _call(lib.avexhip_effnet_forward, h, x, B, 64, 64, mask, hook_out, out, None, ws, nws, s)
        return _call(lib.avexhip_stack_forward, h, x, B, 16, None, out, None, ws, nws, s)

    def untouched(self):
        """Did the calls since the last ``reset()`` leave the output buffer alone?"""
        torch.cuda.synchronize()
        return bool((self.out == SENTINEL).all())

    def reset(self):
        self.out.fill_(SENTINEL)


@pytest.fixture(scope="module", params=("beats", "eat", "aves", "effnet", "stack"))
def case(request, built_lib):
    c = Case(request.param)
    yield c
    c.enc.close()
    c.enc.close()      # twice is harmless
    assert c.enc._h is None and c.enc._ws is None and not c.enc._handles


def test_workspace_one_byte_short_is_refused_before_any_launch(case):
    case.reset()
    rc, msg = case.raw_forward(ws_bytes=case.need - 1)
    assert (rc, msg) == (-4, f"{case.family}_forward: workspace too small ({case.need - 1} bytes given, {case.need} needed)")
    assert case.untouched()


def test_hook_arguments_are_refused_before_any_launch(case):
    if case.family == "stack":
        return      # the layer stack has no hooks
    case.reset()
    noun, item, n = HOOKS[case.family]
    who = f"{case.family}_forward"
    ptrs = (C.c_void_p * 32)()
    assert case.raw_forward(mask=1, hook_out=None) == (-1, f"{who}: hook_mask set but hook_out is NULL")
    sel = n - 1      # the last hook, its entry NULL
    assert case.raw_forward(mask=1 << sel, hook_out=ptrs) == (-1, f"{who}: {item} {sel} selected but hook_out[{sel}] is NULL")
    assert case.raw_forward(mask=1 << n, hook_out=ptrs) == (-1, f"{who}: hook_mask has bits beyond {noun} {n - 1}")
    assert case.untouched()


@pytest.mark.parametrize("family", ("beats", "eat", "aves", "effnet", "stack"))
def test_create_refusals_keep_their_texts(built_lib, family):
    lib = built_lib
    create = getattr(lib, f"avexhip_{family}_create")
    arr, n, keep = K.tensor_table({"some.weight": np.zeros(4, np.float32)})
    cfg = _config(family)
    cfg.operand_dtype = 7
    h, msg = _call(create, C.byref(cfg), arr, n)
    assert not h and msg == f"{family}_create: unknown operand dtype 7"
    if family == "effnet":
        return      # no heads
    cfg = _config(family)
    if family == "beats":
        cfg.encoder_embed_dim = 640      # 12 heads
        want = "beats_create: head_dim must be 64 (E=640, H=12)"
    elif family == "stack":
        cfg.embed_dim, cfg.num_heads = 128, 8
        want = "stack_create: head width must be 32, 64, 96 or 128 (E=128, H=8)"
    else:
        cfg.embed_dim = 640
        want = f"{family}_create: head_dim must be 64 (E=640, H=12)"
    h, msg = _call(create, C.byref(cfg), arr, n)
    assert not h and msg == want
    del keep


def test_profile_stage_list_and_a_quiet_alarm(case):
    enc = case.enc
    if case.family == "stack":      # no profiling accessors; its first stage is "cast"
        case.reset()
        assert case.raw_forward()[0] == 0
        assert enc.overflow_events() == 0 and not case.untouched()
        return
    assert enc.last_profile() == []
    enc.set_profiling(True)
    out = enc.forward(case.x)
    prof = enc.last_profile()
    enc.set_profiling(False)
    assert tuple(out["features"].shape) == case.out_shape and bool(torch.isfinite(out["features"]).all())
    assert [name for name, _ms, _fl in prof] == STAGES[case.family]
    assert all(ms >= 0.0 and fl >= 0.0 for _name, ms, fl in prof)
    assert enc.overflow_events() == 0
    if case.family in ("eat", "aves"):      # the call returned un-averaged rows: the fp32-stream handle only
        assert set(enc._handles) == {"f32"}
