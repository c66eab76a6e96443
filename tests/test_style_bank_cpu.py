"""Style switch / blend, the parts that need no GPU: the numpy oracle `blend_ref`, op number and ABI, every validation message of
L2D_OP_WEIGHT_BLEND's launcher and of `WeightBlender` (dry-run), `load_mix` / `set_style` argument checks on CPU instances, and
the MJPEG server's `/style` route against a stub wrapper."""
import io
import json
import os
import sys
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def make_set(seed, extra=None):
    g = torch.Generator().manual_seed(seed)
    s = {"a.w": torch.randn(33, 7, generator=g).to(torch.float16), "a.b": torch.randn(1025, generator=g),
         "big": torch.randn(40000, generator=g).to(torch.float16)}
    s.update(extra or {})
    return s


# ----------------------------------------------------------------------------- the oracle
def test_blend_ref_one_hot_is_the_source_bit_for_bit():
    from live2diff_amd.style_bank import blend_ref
    s0, s1 = make_set(0), make_set(1)
    s0["a.b"][:4] = torch.tensor([-0.0, 0.0, 1e-42, -65504.0])          # -0.0 + 0 * x would be +0.0: the zero term is dropped
    s0["a.w"].view(-1)[:3] = torch.tensor([-0.0, 6e-8, 65504.0], dtype=torch.float16)
    for srcs, w in (([s0], [1.0]), ([s0, s1], [1.0, 0.0]), ([s1, s0], [0.0, 1.0]), ([s1, s0, s1], [0, 1, 0])):
        out = blend_ref(srcs, w)
        for k in s0:
            assert out[k].dtype == s0[k].dtype and out[k].shape == s0[k].shape
            assert np.array_equal(out[k].numpy().view(np.uint8), s0[k].numpy().view(np.uint8)), (k, w)


def test_blend_ref_is_fp32_mul_then_add_in_source_order():
    from live2diff_amd.style_bank import blend_ref
    f = np.float32
    # three terms, the order written out: ((a0 x0) + (a1 x1)) + (a2 x2), every product and every sum an fp32 of its own
    a = [0.5, 0.25, 0.25]
    x = [f(2.0) + f(2.0 ** -22), f(2.0 ** -22) + f(2.0 ** -45), f(3.0 ** -7)]
    srcs = [{"t": torch.tensor([v], dtype=torch.float32)} for v in x]
    want = f(f(f(a[0]) * x[0]) + f(f(a[1]) * x[1])) + f(f(a[2]) * x[2])
    got = blend_ref(srcs, a)["t"].numpy()[0]
    assert got.dtype == np.float32 and got == want
    # the same terms in exact arithmetic (what an fma chain approaches) or in another order give another fp32
    rng = np.random.default_rng(0)
    s = [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]
    w = [0.3, 0.3, 0.4]
    got = blend_ref([{"t": torch.from_numpy(v)} for v in s], w)["t"].numpy()
    step = f(w[0]) * s[0]
    step = step + f(w[1]) * s[1]
    step = step + f(w[2]) * s[2]
    assert np.array_equal(got, step)
    fused = (np.float64(f(w[0])) * s[0] + np.float64(f(w[1])) * s[1]).astype(np.float32)         # fma(a1, s1, a0 s0) up to its one rounding
    two = (f(w[0]) * s[0] + f(w[1]) * s[1])
    assert (fused != two).any(), "the data cannot tell mul + add from a fused multiply-add"
    swapped = blend_ref([{"t": torch.from_numpy(v)} for v in (s[2], s[1], s[0])], [w[2], w[1], w[0]])["t"].numpy()
    assert (swapped != got).any()
    # fp16: fp32 accumulation, ONE rounding at the end
    h = [torch.from_numpy(v).to(torch.float16) for v in s]
    got16 = blend_ref([{"t": v} for v in h], w)["t"]
    acc = f(w[0]) * h[0].numpy().astype(np.float32)
    for k in (1, 2):
        acc = acc + f(w[k]) * h[k].numpy().astype(np.float32)
    assert got16.dtype == torch.float16 and np.array_equal(got16.numpy(), acc.astype(np.float16))
    # a negative weight (extrapolation) is an affine combination too
    out = blend_ref([{"t": torch.tensor([1.0, 2.0])}, {"t": torch.tensor([3.0, 6.0])}], [-0.5, 1.5])["t"]
    assert out.tolist() == [4.0, 8.0]


def test_op_number_and_abi():
    from live2diff_amd import _lib, ops
    assert _lib.OP_WEIGHT_BLEND == 42 and _lib.ABI_VERSION == 6 and _lib.lib.l2d_abi_version() == 6
    assert ops.WBLEND_REC.itemsize == 64 and ops.WBLEND_TILE_BYTES % 16 == 0
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert "L2D_OP_WEIGHT_BLEND = 42," in hdr and "#define L2D_ABI_VERSION 6" in hdr
    assert f"#define L2D_WBLEND_TILE_BYTES {ops.WBLEND_TILE_BYTES}" in hdr and f"#define L2D_WBLEND_MAX_SRC {ops.WBLEND_MAX_SRC}" in hdr


# ----------------------------------------------------------------------------- the launcher's validation (dry run)
def test_launcher_rejects_what_the_kernel_cannot_do(dry_run):
    from live2diff_amd import ops
    from live2diff_amd._lib import L2DError
    from live2diff_amd.style_bank import WeightBlender
    d, s = make_set(9), [make_set(j) for j in range(4)]
    wb = WeightBlender(d, "cpu")
    dev, host, _ = wb._table(s[:2])
    assert len(host) == 1 + 1 + 2 and host["n"].tolist() == [33 * 7, 1025, 32768, 40000 - 32768] and host["dtype"].tolist() == [0, 1, 0, 0]
    assert int(host["dst"][3]) == d["big"].data_ptr() + ops.WBLEND_TILE_BYTES
    assert int(host["src"][3][1]) == s[1]["big"].data_ptr() + ops.WBLEND_TILE_BYTES and (host["src"][:, 2:] == 0).all()

    def bad(match, op):
        with pytest.raises(L2DError, match=match):
            ops.run(op)

    def table(**change):
        h = host.copy()
        for k, v in change.items():
            if k == "src1":
                h["src"][1][1] = v
            else:
                h[k][1] = v
        return torch.from_numpy(h.view(np.uint8).reshape(-1).copy()), h

    ops.run(ops.weight_blend(dev, host, [0.25, 0.75]))
    ops.run(ops.weight_blend(dev, host, [-0.5, 1.5], nt=1))
    ops.run(ops.weight_blend(dev, host, [1.0]))                         # K = 1 reads src[0] only
    bad("K = 0 sources", ops.weight_blend(dev, host, []))
    bad("K = 5 sources", ops.weight_blend(dev, host, [0.2] * 5))
    bad("src 2", ops.weight_blend(dev, host, [0.5, 0.25, 0.25]))        # the table was built for two sources: src[2] is null
    bad("weight 1 is not finite", ops.weight_blend(dev, host, [0.5, float("nan")]))
    bad("weight 0 is not finite", ops.weight_blend(dev, host, [float("inf"), 0.5]))
    bad("cache policy 2", ops.weight_blend(dev, host, [0.5, 0.5], nt=2))
    bad("record 1: dst is not 16-byte aligned", ops.weight_blend(*table(dst=int(host["dst"][1]) + 4), [0.5, 0.5]))
    bad("record 1: src 1 is not 16-byte aligned", ops.weight_blend(*table(src1=int(host["src"][1][1]) + 2), [0.5, 0.5]))
    bad("record 1 has a null dst", ops.weight_blend(*table(dst=0), [0.5, 0.5]))
    bad("record 1 has a null src 1", ops.weight_blend(*table(src1=0), [0.5, 0.5]))
    bad("record 1 has 0 elements", ops.weight_blend(*table(n=0), [0.5, 0.5]))
    bad("record 1 has -3 elements", ops.weight_blend(*table(n=-3), [0.5, 0.5]))
    bad("record 1 has 16385 elements", ops.weight_blend(*table(n=ops.WBLEND_TILE_BYTES // 4 + 1), [0.5, 0.5]))
    bad("unknown dtype 2", ops.weight_blend(*table(dtype=2), [0.5, 0.5]))
    op, keep = ops.weight_blend(dev, host, [0.5, 0.5])
    op.i[0] = 0
    bad("no records", (op, keep))
    op, keep = ops.weight_blend(dev, host, [0.5, 0.5])
    op.p[1] = None
    bad("null table", (op, keep))
    op, keep = ops.weight_blend(dev, host, [0.5, 0.5])
    op.p[0] = dev.data_ptr() + 8
    bad("device table is not 16-byte aligned", (op, keep))


def test_weight_blender_checks(dry_run):
    from live2diff_amd.style_bank import WeightBlender
    d, s0, s1 = make_set(9), make_set(0), make_set(1)
    wb = WeightBlender(d, "cpu")
    wb.apply([s0, s1], [0.5, 0.5])
    t0 = wb._table([s0, s1])
    wb.apply([s0, s1], [0.25, 0.75])
    assert wb._table([s0, s1]) is t0 and len(wb._tables) == 1           # one table per tuple of source sets, whatever the weights
    wb.apply([s0, s1], [1.0, 0.0])                                       # the zero term is dropped: the K = 1 table of s0
    assert len(wb._tables) == 2 and wb._table([s0])[1]["src"][:, 1:].max() == 0
    assert wb.nbytes == sum(t.numel() * t.element_size() for t in d.values())
    for w, match in (([0.5, 0.6], "sum to"), ([0.5, 0.5 + 3e-6], "sum to"), ([float("nan"), 1.0], "finite"), ([float("inf"), 0.0], "finite"),
                     ([1.0], "one weight per source"), ([], "one weight per source")):
        with pytest.raises(ValueError, match=match):
            wb.apply([s0, s1], w)
    wb.apply([s0, s1], [0.5, 0.5 + 5e-7])                                # inside the 1e-6 bound
    five = [make_set(j) for j in range(5)]
    with pytest.raises(ValueError, match="at most 4"):
        wb.apply(five, [0.2] * 5)
    wb.apply(five, [0.25, 0.25, 0.0, 0.25, 0.25])                        # five sources, four non-zero
    with pytest.raises(TypeError, match="fp16 and fp32 only"):           # an integer tensor is refused, not skipped
        WeightBlender(make_set(9, {"idx": torch.zeros(8, dtype=torch.int32)}), "cpu")
    with pytest.raises(TypeError, match="idx.*fp16 and fp32 only"):
        both = {"idx": torch.zeros(8)}
        WeightBlender(make_set(9, both), "cpu").apply([make_set(0, {"idx": torch.zeros(8, dtype=torch.int64)})], [1.0])
    with pytest.raises(ValueError, match=r"a\.b: shape \(1024,\)"):
        wb.apply([make_set(0, {"a.b": torch.zeros(1024)})], [1.0])
    with pytest.raises(TypeError, match=r"a\.b: dtype torch.float16"):
        wb.apply([make_set(0, {"a.b": torch.zeros(1025, dtype=torch.float16)})], [1.0])
    with pytest.raises(ValueError, match="names differ"):
        wb.apply([make_set(0, {"more": torch.zeros(4)})], [1.0])
    with pytest.raises(ValueError, match="not contiguous"):
        wb.apply([make_set(0, {"a.w": torch.zeros(7, 33, dtype=torch.float16).t()})], [1.0])
    with pytest.raises(ValueError, match="empty destination"):
        WeightBlender({}, "cpu")


# ----------------------------------------------------------------------------- load_mix on CPU instances (dry run)
def test_unet_and_clip_load_mix_validate(dry_run):
    from live2diff_amd.clip_hip import HipClipTextEncoder, random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.style_bank import clone_set
    from live2diff_amd.unet_hip import HipStreamingUNet, PackedWeights
    from live2diff_amd.weights import random_state_dict
    cfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=64)
    sd = random_state_dict(cfg, dtype=torch.float16)
    a = HipStreamingUNet(sd, cfg, 16, 16, 2, device="cpu")
    assert all(t.dtype in (torch.float16, torch.float32) and t.is_contiguous() for t in a.W.values())
    # the state dict is on the instance's device in the packed dtype: no packed tensor may be one of its tensors or a view of one,
    # or the in-place blend would write into the caller's weights and into every other instance packed from them
    theirs = {v.untyped_storage().data_ptr() for v in sd.values()}
    assert not [k for k, t in a.W.items() if t.untyped_storage().data_ptr() in theirs]
    share = HipStreamingUNet(a, cfg, 16, 16, 2, device="cpu")
    st = a._plan("stream", a.prepare_cache(2))
    st2 = share._plan("stream", share.prepare_cache(2))
    a._ensure_cond(st)
    share._ensure_cond(st2)
    assert st.cond_key is not None and st2.cond_key is not None
    b = clone_set(a.packed_state())
    n_plans, ptr = len(a._plans), a.W["temb_all.w"].data_ptr()
    a.load_mix([b], [1.0])
    a.load_mix([b, clone_set(b)], [0.25, 0.75])
    assert a._w_gen is share._w_gen and a._w_gen[0] == 2
    assert len(a._plans) == n_plans and a._plans["stream"] is st and a.W["temb_all.w"].data_ptr() == ptr      # nothing was rebuilt
    for u, s in ((a, st), (share, st2)):                                 # every sharer's conditioning is stale, once
        u._cond_fresh(s)
        assert s.cond_key is None
        u._ensure_cond(s)
        u._cond_fresh(s)
        assert s.cond_key == ("external",)
    with pytest.raises(ValueError, match="own W"):
        a.load_mix([a.packed_state()], [1.0])
    with pytest.raises(TypeError, match="PackedWeights"):
        a.load_mix([a.W], [1.0])
    foreign = json.loads(b.meta["layout"])
    foreign["ws_tokens"] = [1, 2, 3, 4]
    with pytest.raises(ValueError, match="re-pack"):                      # a set with a foreign _pack_layout
        a.load_mix([PackedWeights(b.W, dict(b.meta, layout=json.dumps(foreign)))], [1.0])
    other = HipStreamingUNet(sd, cfg, 16, 32, 3, device="cpu")           # packed for another latent size and stream batch
    with pytest.raises(ValueError, match="re-pack"):
        a.load_mix([other.packed_state()], [1.0])
    with pytest.raises(ValueError, match="sum to"):
        a.load_mix([b], [0.9])
    assert a._w_gen[0] == 2                                               # a refused mix changed nothing

    ccfg = tiny_clip_config()
    e = HipClipTextEncoder(random_clip_text_state_dict(ccfg, 3), "cpu", ccfg)
    ps = e.packed_state()
    assert set(ps.W) == {"tok", "pos", "ln_g", "ln_b"} | {f"layers.{i}.{k}" for i in range(ccfg.num_hidden_layers) for k in e.layers[0]}
    assert ps.W["layers.1.fc1.w"] is e.layers[1]["fc1.w"] and ps.W["tok"] is e.tok
    f = HipClipTextEncoder(random_clip_text_state_dict(ccfg, 4), "cpu", ccfg).packed_state()
    e.load_mix([f], [1.0])
    e.load_mix([f, clone_set(f)], [0.5, 0.5])
    with pytest.raises(ValueError, match="own tensors"):
        e.load_mix([e.packed_state()], [1.0])
    with pytest.raises(ValueError, match="re-pack"):
        e.load_mix([PackedWeights(f.W, dict(f.meta, config="{}"))], [1.0])


# ----------------------------------------------------------------------------- the wrapper's argument checks (device="cpu")
def test_set_style_argument_checks(dry_run):
    from live2diff_amd.clip_hip import HipClipTextEncoder, HipPromptEncoder, random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    from live2diff_amd.config import tiny_config
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.vae_hip import HipTinyVAE, random_taesd_state_dict
    from live2diff_amd.weights import random_state_dict
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=ccfg.hidden_size)
    sd, csd = random_state_dict(ucfg, dtype=torch.float16), random_clip_text_state_dict(ccfg, 3)
    penc = HipPromptEncoder(HipClipTextEncoder(csd, "cpu", ccfg), ClipTokenizer.from_dir(os.path.join(HERE, "golden", "clip_tok")), 1)
    pipe = SimpleNamespace(device=torch.device("cpu"), vae_scale_factor=8, unet=HipStreamingUNet(sd, ucfg, 16, 16, 2, device="cpu"),
                           vae=HipTinyVAE(random_taesd_state_dict(), device="cpu"), depth_model=HipMidas(random_midas_state_dict(), device="cpu"),
                           scheduler=None, _encode_prompt=penc._encode_prompt)
    w = Wrapper.from_components(pipe, num_inference_steps=50, t_index_list=[30, 40], width=128, height=128, device="cpu",
                                warmup_frames=ucfg.sink_size, window_size=ucfg.window_size, output_type="u8")
    assert w.styles == ["default"] and w.style == {"default": 1.0}
    default = w._bank.sets["default"]
    assert all(default[0].W[k] is not t and torch.equal(default[0].W[k], t) for k, t in pipe.unet.W.items())       # a copy
    sd_b = {k: (v * 1.5 if k.endswith("to_q.weight") else v) for k, v in sd.items()}
    w.add_style("b", unet_state_dict=sd_b, text_state_dict=random_clip_text_state_dict(ccfg, 4))
    assert w.styles == ["default", "b"]
    w.set_style("b")
    assert w.style == {"b": 1.0}
    w.set_style({"default": 0.25, "b": 0.75})
    assert w.style == {"default": 0.25, "b": 0.75}
    w.set_style({"default": 1.0, "b": 0.0})
    assert w.style == {"default": 1.0}
    for style, exc, match in (("nope", KeyError, "unknown style 'nope'"), ({"b": 0.5}, ValueError, "sum to"), ({}, ValueError, "style name or a dict"),
                              (None, ValueError, "style name or a dict"), ({"b": float("nan"), "default": 1.0}, ValueError, "finite"),
                              ({"b": "much"}, ValueError, "must be numbers"),
                              ({n: 0.2 for n in "abcde"}, ValueError, "at most 4")):
        with pytest.raises(exc, match=match):
            w.set_style(style)
    assert w.style == {"default": 1.0}
    with pytest.raises(ValueError, match="registered already"):
        w.add_style("b", unet_state_dict=sd_b, text_state_dict=csd)
    with pytest.raises(ValueError, match="go together"):
        w.add_style("c", unet_state_dict=sd_b)
    with pytest.raises(ValueError, match="not both"):
        w.add_style("c", "some.safetensors", unet_state_dict=sd_b, text_state_dict=csd)
    with pytest.raises(ValueError, match="made from components"):
        w.add_style("c", "some.safetensors")
    with pytest.raises(ValueError, match="current mix"):
        w.remove_style("default")
    with pytest.raises(KeyError, match="unknown style"):
        w.remove_style("c")
    b_set = w._bank.sets["b"][0].W
    assert any(b_set is s for hit in pipe.unet._blender._tables.values() for s in hit[2])
    w.remove_style("b")
    assert w.styles == ["default"]
    assert not any(b_set is s for hit in pipe.unet._blender._tables.values() for s in hit[2])     # its blend tables went with it
    # components that are not the native ones: no bank, and the calls say so
    import pipeline_mocks as M
    mp = M.MockPipe()
    mp.unet, mp.vae, mp.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    mp.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    mock = Wrapper.from_components(mp, output_type="pt", dtype=torch.float32, device="cpu", num_inference_steps=50, t_index_list=[10, 20, 30],
                                   width=M.W, height=M.H)
    assert mock.styles == [] and mock.style == {}
    for call in (lambda: mock.set_style("default"), lambda: mock.add_style("b", unet_state_dict=sd_b, text_state_dict=csd),
                 lambda: mock.remove_style("default")):
        with pytest.raises(ValueError, match="native UNet"):
            call()


# ----------------------------------------------------------------------------- the server's /style route, no socket
class _Connection:
    """what `BaseHTTPRequestHandler` asks of a socket, on two in-memory files"""

    def __init__(self, request: bytes):
        self.rfile, self.wfile = io.BytesIO(request), io.BytesIO()
        self.wfile.close = lambda: None

    def makefile(self, mode, *a, **kw):
        return self.rfile if "r" in mode else self.wfile

    def sendall(self, data):
        self.wfile.write(data)


def _request(handler, method, path, body=b"", length=None):
    head = f"{method} {path} HTTP/1.1\r\nHost: test\r\n"
    if method == "POST":
        head += f"Content-Length: {len(body) if length is None else length}\r\n"
    conn = _Connection(head.encode() + b"\r\n" + body)
    handler(conn, ("127.0.0.1", 0), None)
    return conn.wfile.getvalue()


def test_mjpeg_server_style_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    from live2diff_amd.jpeg import mjpeg_part
    assert S.parse_style_arg("toon=models/toon.safetensors") == ("toon", "models/toon.safetensors", {})
    assert S.parse_style_arg("ink=db.ckpt,loras/ink.safetensors:0.8,l2:1") == ("ink", "db.ckpt", {"loras/ink.safetensors": 0.8, "l2": 1.0})
    assert S.parse_style_arg("soft=,loras/soft.safetensors:0.5") == ("soft", None, {"loras/soft.safetensors": 0.5})
    for text in ("toon", "=x", "a=", "a=db,lora", "a=db,:1"):
        with pytest.raises(ValueError, match="--style"):
            S.parse_style_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the style each frame ran under; posts requests from inside the loop"""

        def __init__(self):
            self.style, self.seen, self.calls = {"default": 1.0}, [], []

        def set_style(self, mix):
            self.calls.append(dict(mix))
            if "broken" in mix:
                raise ValueError("refused")
            self.style = dict(mix)

        def __call__(self, frame):
            self.seen.append((frame, dict(self.style)))
            n = len(self.seen)
            if n == 1:
                assert post({"b": 1}).startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post({"default": 0.5, "b": 0.5}).startswith(b"HTTP/1.0 204")
                assert post({"default": 0.25, "b": 0.75}).startswith(b"HTTP/1.0 204")          # the newest request wins
            elif n == 3:
                assert post({"broken": 1.0}).startswith(b"HTTP/1.0 204")
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    styles = S.StyleBox(["default", "b", "broken"], w.style)
    handler = S.make_handler(latest, None, styles)
    post = lambda mix: _request(handler, "POST", "/style", json.dumps(mix).encode())
    assert _request(S.make_handler(latest), "POST", "/style", b"{}").startswith(b"HTTP/1.0 404")        # no bank, no route
    assert _request(S.make_handler(latest), "GET", "/style").startswith(b"HTTP/1.0 404")
    for body in (b"not json", b"[1, 2]", b'"nobody"', json.dumps({"c": 1.0}).encode(), json.dumps({"b": 0.5}).encode(),
                 json.dumps({"b": "x"}).encode(), b"\xff\xfe{}", json.dumps({"default": 0.5, "b": float("nan")}).encode()):
        assert _request(handler, "POST", "/style", body).startswith(b"HTTP/1.0 400"), body
    assert _request(handler, "POST", "/style", b"{}" * 4096).startswith(b"HTTP/1.0 413")
    assert styles.take() is None                                         # nothing refused was queued
    got = _request(handler, "GET", "/style")
    assert json.loads(got.partition(b"\r\n\r\n")[2]) == {"styles": ["default", "b", "broken"], "current": {"default": 1.0}}
    frames = [b"\xff\xd8 frame %d" % i for i in range(2)]
    S.produce(w, frames, latest, stop, styles)                           # (in this thread)
    assert [s for _, s in w.seen] == [{"default": 1.0}, {"b": 1.0}, {"default": 0.25, "b": 0.75}, {"default": 0.25, "b": 0.75},
                                      {"default": 0.25, "b": 0.75}]     # applied between frames; the refused one changed nothing
    assert w.calls == [{"b": 1.0}, {"default": 0.25, "b": 0.75}, {"broken": 1.0}] and styles.failed == 1
    assert styles.current == {"default": 0.25, "b": 0.75}
    assert _request(handler, "GET", "/stream").partition(b"\r\n\r\n")[2] == mjpeg_part(frames[0])
