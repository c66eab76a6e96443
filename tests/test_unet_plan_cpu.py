"""The pieces of the UNet's plan builder (live2diff_amd/unet_plan.py), called directly on CPU tensors in validate-only mode: the
form lookup, the LayerNorm -> Linear helper, the head segment's decline path.  (Whole plans: tests/test_plan_fingerprints.py.)"""
import pytest
import torch

from live2diff_amd import _lib, ops
from live2diff_amd.config import tiny_config
from live2diff_amd.unet_hip import HipStreamingUNet
from live2diff_amd.unet_plan import UNetPlan
from live2diff_amd.weights import random_state_dict


@pytest.fixture
def dry_run():
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def _plan(unet, W=None) -> UNetPlan:
    """a stream plan of `unet` with nothing built yet (only the builder's own first op)"""
    return UNetPlan(unet.cfg, W or unet.W, unet.h, unet.w, unet.N, unet.F, unet.device, temb_offsets=unet.temb_offsets,
                    text_offsets=unet.text_offsets, n_map_blocks=unet.n_map_blocks, text_len=unet.text_len,
                    tattn_variant=unet.tattn_variant, mode="stream", kv_cache=unet.prepare_cache(unet.N))


_tiny = {}


def _tiny_unet():
    """16 x 24 latent: 384 / 96 / 24 / 6 tokens per sample -- the spatial blocks of level 2 and the mid block hold both packed forms"""
    if not _tiny:
        cfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=96)
        sd = random_state_dict(cfg, dtype=torch.float16)
        _tiny.update(sd=sd, unet=HipStreamingUNet(sd, cfg, 16, 24, 2, device="cpu"))
    return _tiny["unet"], _tiny["sd"]


def _kinds(pl, since):
    return [op.kind for op in pl._ops[since:]]


def test_form_lookup_where_both_forms_are_packed(dry_run):
    unet, _ = _tiny_unet()
    p, W = _plan(unet), unet.W
    for blk, T in (("down_blocks.2.attentions.0", 24), ("mid_block.attentions.0", 6)):
        b = blk + ".transformer_blocks.0"
        for name, sfx in ((blk + ".proj_in", ""), (b + ".attn2.to_q", ""), (b + ".ff", "1")):
            assert (name + ".rw" + sfx) in W and (name + ".w" + sfx) in W
            assert p.form(name, sfx=sfx) == "row"                    # (a temporal layer, or whole tiles)
            assert p.form(name, 96, sfx) == "row"
            assert p.form(name, T, sfx) == "igemm"                   # this level's samples are no whole 32-token tiles
    ws = next(k[:-3] for k in W if k.endswith(".ww"))
    assert (ws + ".rw") not in W and p.form(ws) == p.form(ws, 24) == "ws"
    assert (set(W) & {"conv_in.w", "conv_in.rw", "conv_in.ww", "conv_in.cw"}) == {"conv_in.w"} and p.form("conv_in") == "igemm"
    p.W = dict(W, **{"conv_in.cw": W["conv_in.w"]})
    assert p.form("conv_in") == "cconv"


def test_layernorm_linear_helper_emits_each_form(dry_run):
    unet, sd = _tiny_unet()
    b = "down_blocks.1.attentions.0.transformer_blocks.0"            # level 1: 128 channels, 8 x 12 = 96 tokens per sample
    name, C, HW = b + ".attn2.to_q", 128, (8, 12)
    assert (name + ".rw") in unet.W and (name + ".w") not in unet.W and (name + ".ww") not in unet.W
    g = lambda k: sd[k]
    ww, wb, wcs = ops.pack_wsgemm(g(name + ".weight"), None, g(b + ".norm2.weight"), g(b + ".norm2.bias"))
    forms = {"row": unet.W,
             "ws": dict({k: v for k, v in unet.W.items() if not k.startswith(name)}, **{name + ".ww": ww, name + ".wb": wb, name + ".wcs": wcs}),
             "igemm": dict({k: v for k, v in unet.W.items() if not k.startswith(name)}, **{name + ".w": ops.pack_linear(g(name + ".weight"))})}
    want = {"row": [_lib.OP_ROWGEMM], "ws": [_lib.OP_WSGEMM], "igemm": [_lib.OP_LAYERNORM, _lib.OP_IGEMM]}
    for form, W in forms.items():
        p = _plan(unet, W)
        assert p.form(name) == form
        x, out = p.act(C, *HW), p.act(C, *HW)
        n0 = len(p.pl)
        got, n = p.ln_linear(x, b + ".norm2", name, out)
        assert _kinds(p.pl, n0) == want[form], form
        assert (n is not None) == (form == "igemm") and (got.C, got.H, got.W) == (C, *HW)
        last = p.pl[len(p.pl) - 1]
        assert last.p[0] == (n if form == "igemm" else x).buf.data_ptr()              # reads the LayerNorm's output / x itself
        if form != "igemm":
            assert got is out and last.i[{"row": 7, "ws": 20}[form]] == 1            # the LayerNorm is the launch's prologue
        p.pl.run(stream=0)                                                           # every launch passes the library's validation
    # the feed-forward's first layer through the same helper (GEGLU epilogue), spatial block without whole tiles: implicit GEMM
    p = _plan(unet)
    ff = "down_blocks.2.attentions.0.transformer_blocks.0.ff"
    x = p.act(256, 4, 6)
    for T, kinds in ((None, [_lib.OP_ROWGEMM]), (24, [_lib.OP_LAYERNORM, _lib.OP_IGEMM])):
        n0 = len(p.pl)
        hid, n = p.ln_linear(x, ff[:-3] + ".norm3", ff, p.act(1024, 4, 6), T=T, sfx="1", epi=1)
        assert _kinds(p.pl, n0) == kinds and hid.C == 1024
    p.pl.run(stream=0)


def _arena_state(p):
    return ({k: [t.data_ptr() for t in v] for k, v in p.arena.free.items() if v}, [t.data_ptr() for t in p.arena.all], len(p.pl),
            p.gn_layers)


def test_declined_head_segment_leaves_the_arena_as_it_found_it(dry_run):
    # level 0 at the chain kernel's width, 2 x 40 x 40 tokens = 100 blocks: the head segment runs here when its statistics can
    cfg = tiny_config(channels=(320, 64, 64, 64), cross_attention_dim=64)
    unet = HipStreamingUNet(random_state_dict(cfg, dtype=torch.float16), cfg, 40, 40, 2, device="cpu")
    p = _plan(unet)
    t = "down_blocks.0.motion_modules.0.temporal_transformer"
    a, b = t + ".proj_in", t + ".transformer_blocks.0.attention_blocks.0.qkv"
    assert ops.rowchain_ok(2 * 1600, 320, 1600) and all(k in unet.W for k in (a + ".rw", a + ".rb", b + ".rw"))
    x, res = p.act(320, 40, 40), p.act(320, 40, 40)
    for warm in (p.act(320, 40, 40), p.act(3 * 320, 40, 40)):          # something on the free lists a leak or a swap would show in
        p.free(warm)
    before = _arena_state(p)
    assert x.producer is None                                          # no producer: the GroupNorm's statistics cannot come from one
    assert p.block_head(x, a, b, 3, gn_of=x) == (None, None, None)
    assert _arena_state(p) == before
    small = _plan(_tiny_unet()[0])                                     # 64 channels: not the chain kernel's width
    xs = small.act(64, 16, 24)
    before_s = _arena_state(small)
    assert small.block_head(xs, a, b, 3, gn_of=xs) == (None, None, None) and small.block_head(xs, a, b, 3, res=xs, vt=True) == (None,) * 3
    assert _arena_state(small) == before_s
    # and where it runs: one launch, h and q | k | v from the arena (the two buffers that were free), nothing else touched
    h, qkv, vt = p.block_head(x, a, b, 3, res=res)
    assert vt is None and (h.C, qkv.C) == (320, 960) and _kinds(p.pl, before[2]) == [_lib.OP_ROWCHAIN]
    assert _arena_state(p) == ({}, before[1], before[2] + 1, before[3])
    p.pl.run(stream=0)
