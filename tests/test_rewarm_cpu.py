"""CPU tests (-m "not gpu") of the re-warm: `StreamAnimateDiffusionDepth.rewarm` on the deterministic mocks of
tests/pipeline_mocks.py -- what it calls, what it writes, what it leaves alone, the shadow / commit separation --, the recent
window, the private generator, the builders of L2D_OP_SINK_COMMIT and every refusal of its launcher in dry-run mode, and the wrapper's
argument checks."""
import os

import numpy as np
import pytest
import torch

import pipeline_mocks as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 8
T_INDEX = [20, 30, 45]
N = len(T_INDEX)


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


class LoggingWarmup(M.MockWarmupUNet):
    """the mock warm-up module, with a log of what it was called with and a row it refuses"""

    def __init__(self):
        self.log, self.fail_row = [], None

    def __call__(self, x, t, temporal_attention_mask=None, depth_sample=None, encoder_hidden_states=None, kv_cache=None, return_dict=True):
        if self.fail_row is not None and len(self.log) % N == self.fail_row:
            self.log.append(None)
            raise RuntimeError("the warm-up module failed")
        self.log.append(dict(x=x.clone(), d=depth_sample.clone(), t=t.clone(), enc=encoder_hidden_states.clone(), caches=kv_cache))
        return super().__call__(x, t, temporal_attention_mask, depth_sample, encoder_hidden_states, kv_cache, return_dict)


def make_stream(monkeypatch, seed=2, frames=0, **kw):
    """a prepared stream on the mocks, `frames` frames in"""
    from live2diff_amd import pipeline_stream_animation_depth as P
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    pipe = M.MockPipe()
    pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    s = P.StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=T_INDEX, torch_dtype=torch.float32, width=M.W, height=M.H, **kw)
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = LoggingWarmup()
    s.kv_cache_list = M.make_caches(N)
    torch.manual_seed(123)
    s.prepare(M.frames(F, seed=7), "a prompt", seed=seed)
    for img in M.frames(frames, seed=11):
        s(img)
    return s


UNTOUCHED = ("x_t_latent_buffer", "depth_latent_buffer", "attn_bias", "pe_idx", "update_idx", "prompt_embeds", "init_noise", "stock_noise")


def snapshot(s):
    return dict({k: getattr(s, k).clone() for k in UNTOUCHED}, caches=[c.clone() for c in s.kv_cache_list],
                rb=[t.clone() for t in s._rb], gen=s.generator.get_state().clone(), rng=torch.get_rng_state().clone())


def test_rewarm_runs_the_row_loop_on_shadows_and_commits_the_sinks(monkeypatch):
    s = make_stream(monkeypatch, frames=3)
    warm, live_ids = s.unet_warmup, [id(c) for c in s.kv_cache_list]
    assert len(warm.log) == N                                              # prepare's own rows
    wx, wd = (t.clone() for t in s._warm_window)
    assert torch.equal(wx, warm.log[0]["x"]) and torch.equal(wd, warm.log[0]["d"])      # the window as it entered prepare's loop
    # what the mock's caches hold after `prepare` and three frames is not what a re-warm writes: shift the prompt, as a switch would
    s.prompt_embeds = s.prompt_embeds + 0.5
    before = snapshot(s)
    gen = s.rewarm_generator()
    s.rewarm()
    assert s.rewarms == 1 and len(warm.log) == 2 * N
    # one call per row, with prompt_embeds[0:1], the retained latents in row 0 and the re-noised x0 of the row before in the others
    x = wx
    for idx, call in enumerate(warm.log[N:]):
        assert torch.equal(call["enc"], s.prompt_embeds[0:1]) and torch.equal(call["t"], s.sub_timesteps_tensor[idx].view(1))
        assert torch.equal(call["x"], x) and torch.equal(call["d"], wd), idx
        assert all(c.data_ptr() == sh[idx].data_ptr() for c, sh in zip(call["caches"], s._shadow))     # it wrote into the shadows
        pred = 0.4 * x + 0.2 * wd - 0.0005 * call["t"].float().view(-1, 1, 1, 1, 1) + 0.03 * call["enc"].mean()
        x0 = s.scheduler_step_batch(pred, x, idx)
        if idx < N - 1:
            noise = torch.randn(x0.shape, generator=gen, dtype=x0.dtype)
            x = s.alpha_prod_t_sqrt[idx + 1] * x0 + s.beta_prod_t_sqrt[idx + 1] * noise
    # the sinks of every cache are what the mock writes; slots F.. are as they were
    for c, old in zip(s.kv_cache_list, before["caches"]):
        for idx, call in enumerate(warm.log[N:]):
            want = (call["x"][0].mean(dim=(0, 2, 3)) + 0.01 * call["t"].float()).view(1, 1, F, 1).expand(2, c.shape[2], F, c.shape[4])
            assert torch.equal(c[idx, :, :, :F], want), idx
        assert torch.equal(c[:, :, :, F:], old[:, :, :, F:]) and not torch.equal(c[:, :, :, :F], old[:, :, :, :F])
    # everything else is bit-equal to the snapshot, the generators included
    assert [id(c) for c in s.kv_cache_list] == live_ids
    after = snapshot(s)
    for k in UNTOUCHED + ("gen", "rng"):
        assert torch.equal(after[k], before[k]), k
    assert all(torch.equal(a, b) for a, b in zip(after["rb"], before["rb"]))


def test_frames_after_a_rewarm_equal_a_run_with_hand_patched_caches(monkeypatch):
    a, b = make_stream(monkeypatch, frames=3), make_stream(monkeypatch, frames=3)
    assert all(torch.equal(x, y) for x, y in zip(a.kv_cache_list, b.kv_cache_list))
    for s in (a, b):
        s.prompt_embeds = s.prompt_embeds + 0.5
    a.rewarm()
    # b: the same loop by hand on scratch caches, patched into the live ones
    scratch = [torch.zeros_like(c) for c in b.kv_cache_list]
    gen = b.rewarm_generator()
    b._warm_rows(*b._warm_window, scratch, lambda x: torch.randn(x.shape, generator=gen, dtype=x.dtype))
    for c, sc in zip(b.kv_cache_list, scratch):
        c[:, :, :, :F] = sc[:, :, :, :F]
    rest = M.frames(9, seed=11)[3:]
    torch.manual_seed(5)
    out_a = [a(img) for img in rest]
    torch.manual_seed(5)
    out_b = [b(img) for img in rest]
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))
    assert all(torch.equal(x, y) for x, y in zip(a.kv_cache_list, b.kv_cache_list))
    # ... and differ from a stream that was not re-warmed: the sinks matter
    c = make_stream(monkeypatch, frames=3)
    c.prompt_embeds = c.prompt_embeds + 0.5
    torch.manual_seed(5)
    assert not torch.equal(c(rest[0]), out_a[0])


def test_a_rewarm_that_fails_on_row_1_changes_no_cache(monkeypatch):
    s = make_stream(monkeypatch, frames=2)
    s.prompt_embeds = s.prompt_embeds + 0.5
    before = snapshot(s)
    s.unet_warmup.fail_row = 1
    other = (s._warm_window[0] + 1.0, s._warm_window[1])                     # (another window: row 0's sinks would change too)
    with pytest.raises(RuntimeError, match="warm-up module failed"):
        s.rewarm(*other)
    assert s.rewarms == 0
    assert s.unet_warmup.log[N] is not None and s.unet_warmup.log[N + 1] is None              # row 0 ran, into the shadows
    for sh, old in zip(s._shadow, before["caches"]):
        assert float(sh[0, :, :, :F].abs().min()) > 0 and not torch.equal(sh[0, :, :, :F], old[0, :, :, :F]) and not sh[1:].any()
    assert all(torch.equal(c, old) for c, old in zip(s.kv_cache_list, before["caches"]))      # every live cache, bit for bit
    s.unet_warmup.fail_row = None
    s.unet_warmup.log.append(None)            # (re-align the logging mock's row counter)
    s.rewarm()
    assert s.rewarms == 1


def test_rewarm_argument_checks(monkeypatch):
    from live2diff_amd import pipeline_stream_animation_depth as P
    pipe = M.MockPipe()
    pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    s = P.StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=T_INDEX, torch_dtype=torch.float32, width=M.W, height=M.H)
    s.unet_warmup = LoggingWarmup()
    for call in (s.rewarm, s.rewarm_generator, lambda: s.encode_window(M.frames(F, 1))):
        with pytest.raises(RuntimeError, match="prepare"):
            call()
    s = make_stream(monkeypatch)
    calls = len(s.unet_warmup.log)
    good = torch.zeros(1, 4, F, 8, 8)
    for x, d in ((torch.zeros(1, 4, F - 1, 8, 8), torch.zeros(1, 4, F - 1, 8, 8)), (good, torch.zeros(1, 4, F, 8, 4)), (good[0], good),
                 (torch.zeros(2, 4, F, 8, 8), good), ("frames", good)):
        with pytest.raises(ValueError, match="expected latents shaped"):
            s.rewarm(x, d)
    for x, d in ((good, None), (None, good)):
        with pytest.raises(ValueError, match="go together"):
            s.rewarm(x, d)
    assert len(s.unet_warmup.log) == calls and s._shadow is None and s.rewarms == 0           # refused before any launch
    s.rewarm(good + 1.0, good)
    assert s.rewarms == 1 and torch.equal(s.unet_warmup.log[calls]["x"], good + 1.0)


def test_encode_window_leaves_the_tap_and_the_stream_generator_alone(monkeypatch):
    s = make_stream(monkeypatch, frames=1)
    taps = []
    s.matte_tap = lambda x, dn: taps.append("frame")
    s.matte_tap.prime = lambda x, dn: taps.append("prime")
    state = s.generator.get_state().clone()
    window = M.frames(F, seed=31)
    x, d = s.encode_window(window)
    assert x.shape == d.shape == (1, 4, F, 8, 8) and taps == []
    assert torch.equal(s.generator.get_state(), state)
    # `prepare`'s encode with the re-warm's generator in the stream's place
    g = s.rewarm_generator()
    lat = M.retrieve_latents(s.vae.encode(2.0 * window - 1.0)) * s.vae.config.scaling_factor
    noise = torch.randn(lat.shape, dtype=lat.dtype, generator=g)
    assert torch.equal(x, s.add_noise(lat, noise, 0).transpose(0, 1)[None])
    with pytest.raises(ValueError, match=f"expected {F} frames"):
        s.encode_window(window[:3])
    s.rewarm(x, d)
    assert s.rewarms == 1


def test_recent_window_order_drops_and_count(monkeypatch):
    s = make_stream(monkeypatch, keep_recent=True)
    with pytest.raises(ValueError, match="0 frames since prepare"):
        s.recent_window()
    entered = []
    step = s.predict_x0_batch
    s.predict_x0_batch = lambda x, d, **kw: (entered.append((x.clone(), d.clone())), step(x, d, **kw))[1]

    class DropEveryThird:
        n = 0

        def __call__(self, x):
            self.n += 1
            return None if self.n % 3 == 0 else x

        def set_threshold(self, v):
            pass

        def set_max_skip_frame(self, v):
            pass

    imgs = M.frames(16, seed=13)
    for img in imgs[:F - 1]:
        s(img)
    with pytest.raises(ValueError, match=f"{F - 1} frames since prepare, the window needs {F}"):
        s.recent_window()
    s.similar_filter = DropEveryThird()
    s.enable_similar_image_filter()
    for img in imgs[F - 1:]:
        s(img)
    dropped = 16 - (F - 1) - len(entered[F - 1:])
    assert dropped == 3 and s._recent_seen == len(entered) == 13           # a dropped frame is not recorded
    x, d = s.recent_window()
    assert x.shape == d.shape == (1, 4, F, 8, 8)
    for k, (ex, ed) in enumerate(entered[-F:]):                              # oldest first, after the ring wrapped round
        assert torch.equal(x[0, :, k], ex[0, :, 0]) and torch.equal(d[0, :, k], ed[0, :, 0]), k
    s.rewarm(x, d)
    assert torch.equal(s.unet_warmup.log[-N]["x"], x)
    # a new prepare starts the count again
    s.disable_similar_image_filter()
    s.prepare(M.frames(F, seed=7), "a prompt", seed=2)
    with pytest.raises(ValueError, match="0 frames since prepare"):
        s.recent_window()
    with pytest.raises(ValueError, match="keep_recent=True"):
        make_stream(monkeypatch).recent_window()


def test_without_keep_recent_a_frame_issues_no_additional_copy(monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    def launches(s, img):
        with Count() as c:
            s(img)
        return c.ops

    img = M.frames(2, seed=17)
    off, on = make_stream(monkeypatch, frames=1), make_stream(monkeypatch, frames=1, keep_recent=True)
    assert off.keep_recent is False and off._recent is None
    for k in range(2):
        a, b = launches(off, img[k]), launches(on, img[k])
        extra = list(b)
        for name in a:
            extra.remove(name)
        copies = [n for n in extra if "copy_" in n]
        assert len(copies) == 2, extra                                       # the ring costs two copies (and the views they go through)
        assert not [n for n in extra if n not in copies and not any(v in n for v in ("select", "view", "reshape", "zeros", "_unsafe_view"))], extra
    assert off._recent is None and on._recent_seen == 3


def test_the_private_generator(monkeypatch):
    a, b, c = make_stream(monkeypatch, seed=2, frames=2), make_stream(monkeypatch, seed=2, frames=5), make_stream(monkeypatch, seed=3, frames=2)
    draw = lambda s: torch.randn(64, generator=s.rewarm_generator())
    assert torch.equal(draw(a), draw(b)) and not torch.equal(draw(a), draw(c))       # the stream's seed, not its position
    first = draw(a)
    state, rng = a.generator.get_state().clone(), torch.get_rng_state().clone()
    a.rewarm()
    b.rewarm()
    assert torch.equal(a.generator.get_state(), state) and torch.equal(torch.get_rng_state(), rng)
    assert torch.equal(a.unet_warmup.log[-1]["x"], b.unet_warmup.log[-1]["x"])       # two streams of one seed drew the same noise
    assert not torch.equal(draw(a), first) and torch.equal(draw(a), draw(b))         # the counter moves it on
    # a caller's generator is used as it is
    g1, g2 = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
    a.rewarm(generator=g1)
    c.rewarm(generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state()) and not torch.equal(g1.get_state(), torch.Generator().manual_seed(99).get_state())


# ----------------------------------------------------------------------------- the op's builders and its launcher, dry-run
def caches(shapes, L, F_src=None):
    return [torch.zeros(2, 2, hw, L if F_src is None else F_src, C, dtype=torch.float16) for hw, C in shapes]


SHAPES = [(1, 64), (5, 320), (64, 128)]


def test_sink_commit_builders(dry_run):
    from live2diff_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert _lib.OP_SINK_COMMIT == 64 and "L2D_OP_SINK_COMMIT = 64," in hdr and "typedef struct l2d_sink_rec" in hdr
    assert ops.SINK_REC.itemsize == 48 and ops.SINK_REC.names == ("dst", "src", "lines", "line_bytes", "dst_pitch", "src_pitch")
    for L, F_, compact in ((16, 8, False), (12, 3, False), (16, 8, True)):
        dst, src = caches(SHAPES, L), caches(SHAPES, L, F_ if compact else None)
        tab = ops.sink_commit_table(dst, src, F=F_)
        assert tab.dtype == ops.SINK_REC and len(tab) == 3
        for rec, d, s, (hw, C) in zip(tab, dst, src, SHAPES):
            assert (int(rec["dst"]), int(rec["src"])) == (d.data_ptr(), s.data_ptr())
            assert (int(rec["lines"]), int(rec["line_bytes"])) == (2 * 2 * hw, F_ * C * 2)
            assert (int(rec["dst_pitch"]), int(rec["src_pitch"])) == (L * C * 2, (F_ if compact else L) * C * 2)
        dev = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy())
        op, keep = ops.sink_commit(dev, tab)
        assert op.kind == _lib.OP_SINK_COMMIT and op.i[0] == 3 and op.p[0] == dev.data_ptr() and op.p[1] == tab.ctypes.data
        assert keep[0] is dev and keep[1] is tab
        ops.run((op, keep))                                                  # the launcher accepts it
    dst, src = caches(SHAPES, 16), caches(SHAPES, 16)
    for bad_dst, bad_src, F_, match in (
            ([], [], 8, "at least one"), (dst, src[:2], 8, "one source per destination"), (dst, src, 0, "F = 0"), (dst, src, 17, "F = 17"),
            (dst, caches(SHAPES, 16, 4), 8, "F = 8"), ([dst[0].float()], [src[0]], 8, "contiguous fp16"),
            ([dst[2][:, :, ::2]], [src[2][:, :, ::2]], 8, "contiguous fp16"), ([dst[0][0]], [src[0][0]], 8, "contiguous fp16"),
            ([dst[1]], [src[2]], 8, "does not hold the lines"), ([dst[0].numpy()], [src[0]], 8, "contiguous fp16")):
        with pytest.raises(ValueError, match=match):
            ops.sink_commit_table(bad_dst, bad_src, F=F_)


def refusals(tab):
    """(what, the table with one field spoilt, the message) for every case the launcher refuses"""
    def spoilt(**fields):
        t = tab.copy()
        for k, v in fields.items():
            t[1][k] = v
        return t
    r = tab[1]
    dst, src, lines, nb, dp = (int(r[k]) for k in ("dst", "src", "lines", "line_bytes", "dst_pitch"))
    return [("null dst", spoilt(dst=0), "null dst"), ("null src", spoilt(src=0), "null src"),
            ("misaligned dst", spoilt(dst=dst + 8), "not 16-byte aligned"), ("misaligned src", spoilt(src=src + 2), "not 16-byte aligned"),
            ("zero lines", spoilt(lines=0), "need at least one"), ("negative lines", spoilt(lines=-4), "need at least one"),
            ("bytes not a multiple of 16", spoilt(line_bytes=nb - 8), "multiples of 16"), ("zero bytes", spoilt(line_bytes=0), "multiples of 16"),
            ("dst pitch not a multiple of 16", spoilt(dst_pitch=dp + 8), "multiples of 16"),
            ("src pitch not a multiple of 16", spoilt(src_pitch=dp + 4), "multiples of 16"),
            ("bytes above the dst pitch", spoilt(dst_pitch=nb - 16), "do not fit the pitches"),
            ("bytes above the src pitch", spoilt(src_pitch=nb - 16), "do not fit the pitches"),
            ("index overflow, lines", spoilt(lines=-(-(1 << 31) // (dp // 16))), "do not fit 2\\^31"),
            ("index overflow, src pitch", spoilt(src_pitch=-(-(1 << 31) // lines) * 16), "do not fit 2\\^31"),
            ("index overflow, huge", spoilt(lines=1 << 40, src_pitch=1 << 40, dst_pitch=1 << 40), "do not fit 2\\^31"),
            ("dst is src", spoilt(src=dst), "overlaps"), ("src inside dst", spoilt(src=dst + (lines - 1) * dp), "overlaps"),
            ("dst inside src", spoilt(dst=src + 16), "overlaps")]


def test_sink_commit_refusals_in_python_and_in_the_launcher(dry_run):
    from live2diff_amd import _lib, ops
    dst, src = caches(SHAPES, 16), caches(SHAPES, 16)
    tab = ops.sink_commit_table(dst, src, F=8)
    r = tab[1]
    edge = tab.copy()
    edge[1]["lines"] = -(-(1 << 31) // (int(r["dst_pitch"]) // 16)) - 1          # the largest line count that fits: accepted
    edge[1]["src"] = int(r["dst"]) + (1 << 40)                                  # (nothing is dereferenced in dry-run mode)
    ops.sink_commit_check(edge)
    last = tab.copy()                                                            # a source that ends where the destination begins: no overlap
    last[1]["src"] = int(r["dst"]) - ((int(r["lines"]) - 1) * int(r["src_pitch"]) + int(r["line_bytes"]))
    ops.sink_commit_check(last)
    dev = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy())

    def launch(t, table_dev=dev, n=None):
        op, keep = ops._record(_lib.OP_SINK_COMMIT, (table_dev,), (len(t) if n is None else n,), at={1: t.ctypes.data}, keep=(table_dev, t))
        ops.run((op, keep))

    launch(tab), launch(edge), launch(last)
    for what, bad, match in refusals(tab):
        with pytest.raises(ValueError, match="sink_commit: record 1.*" + match):
            ops.sink_commit_check(bad)
        with pytest.raises(ValueError, match=match):
            ops.sink_commit(dev, bad)
        with pytest.raises(_lib.L2DError, match="rc=-1: sink_commit.*record 1.*" + match):
            launch(bad)
    # the tables themselves
    with pytest.raises(ValueError, match="no records"):
        ops.sink_commit_check(tab[:0])
    with pytest.raises(_lib.L2DError, match="no records"):
        launch(tab, n=0)
    for bad in (tab.view(np.uint8), [tab], tab[::2], None):
        with pytest.raises(ValueError, match="numpy array of SINK_REC"):
            ops.sink_commit(dev, bad)
    big = torch.zeros(tab.nbytes + 16, dtype=torch.uint8)
    for bad_dev in (dev[:-1], dev.to(torch.int8), big[8:8 + tab.nbytes] if big.data_ptr() % 16 == 0 else big[16 - big.data_ptr() % 16 + 8:][:tab.nbytes], None):
        with pytest.raises(ValueError, match="device table"):
            ops.sink_commit(bad_dev, tab)
    off = big[8:8 + tab.nbytes] if big.data_ptr() % 16 == 0 else big[16 - big.data_ptr() % 16 + 8:][:tab.nbytes]
    with pytest.raises(_lib.L2DError, match="device table is not 16-byte aligned"):
        launch(tab, table_dev=off)
    op, keep = ops.sink_commit(dev, tab)
    op.p[1] = None
    with pytest.raises(_lib.L2DError, match="null table"):
        ops.run((op, keep))


# ----------------------------------------------------------------------------- the wrapper's argument checks
def mock_wrapper(**kw):
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    mp = M.MockPipe()
    mp.unet, mp.vae, mp.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    mp.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    return Wrapper.from_components(mp, output_type="pt", dtype=torch.float32, device="cpu", num_inference_steps=50, t_index_list=T_INDEX,
                                   width=M.W, height=M.H, **kw)


def test_wrapper_rewarm_argument_checks():
    w = mock_wrapper()
    assert w.stream.keep_recent is False and w.rewarms == 0
    with pytest.raises(ValueError, match="needs a wrapper built with keep_recent=True"):
        w.rewarm("recent")
    for source in ("warmup", "recent"):
        with pytest.raises(ValueError, match="depths= goes with frames"):
            w.rewarm(source, depths=np.zeros((F, 8, 8), np.float32))
    with pytest.raises(ValueError, match="use 'warmup', 'recent' or a window of frames"):
        w.rewarm("latest")
    with pytest.raises(RuntimeError, match="prepare"):
        w.rewarm()
    with pytest.raises(RuntimeError, match="prepare"):
        w.rewarm(M.frames(F, 3))
    for bad in ("soon", 2, None):
        with pytest.raises(ValueError, match="rewarm="):
            w.set_style("default", rewarm=bad)
    with pytest.raises(ValueError, match="keep_recent=True"):
        w.set_style("default", rewarm="recent")
    with pytest.raises(ValueError, match="native UNet"):                     # (the mocks have no bank: the switch itself is refused)
        w.set_style("default", rewarm=True)
    k = mock_wrapper(keep_recent=True)
    assert k.stream.keep_recent is True
    with pytest.raises(RuntimeError, match="prepare"):
        k.rewarm("recent")


def test_wrapper_rewarm_on_the_mocks(monkeypatch):
    from live2diff_amd import pipeline_stream_animation_depth as P
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    w = mock_wrapper(keep_recent=True)
    s = w.stream
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = LoggingWarmup()
    w.prepare(M.frames(F, seed=7), "a prompt")
    for img in M.frames(F, seed=11):
        w(img)
    log = s.unet_warmup.log
    w.rewarm()
    assert w.rewarms == 1 and torch.equal(log[-N]["x"], s._warm_window[0])
    recent = s.recent_window()
    w.rewarm("recent")
    assert w.rewarms == 2 and torch.equal(log[-N]["x"], recent[0]) and torch.equal(log[-N]["d"], recent[1])
    window = M.frames(F, seed=23)
    want = s.encode_window(window)                                           # (the counter, and so the generator, is the call's below)
    w.rewarm(window)
    assert w.rewarms == 3 and torch.equal(log[-N]["x"], want[0]) and torch.equal(log[-N]["d"], want[1])
    with pytest.raises(ValueError, match=f"expected {F} frames"):
        w.rewarm(window[:2])
    assert w.rewarms == 3
    w.prepare(M.frames(F, seed=7), "a prompt")
    assert w.rewarms == 0
