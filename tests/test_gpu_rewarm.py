"""-m gpu: the re-warm on the tiny UNet of tests/test_gpu_style_switch.py -- channels (64,128,256,256), 64 x 64
frames, N = 2, L = 16, F = 8.

  1. L2D_OP_SINK_COMMIT alone, bit for bit against the slice copy, behind guard bands, directly and through a captured graph;
  2. a re-warm with nothing changed leaves row 0's sinks as they were, rows >= 1 are the loop restated with public calls, and
     nothing else of the stream moves;
  3. after `set_style("b", rewarm=True)` row 0's sinks are those of a stream that was switched before `prepare`;
  4. the following frames differ from a run without the re-warm; push / pop with a frame pending gives `__call__` mode's frames;
  5. "recent" is `rewarm(x, d)` fed with the latents that entered row 0.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_style_switch import DEV, N, PROMPT, add_b, bits, make_wrapper, same

pytestmark = pytest.mark.gpu
F = 8


# ----------------------------------------------------------------------------- 1. the op
SHAPES = [(1, 64), (5, 320), (64, 128)]          # (h * w, C)
GUARD = 64                                       # fp16 elements in front of and behind every tensor


def nan_bits(n, seed):
    """n fp16 words that are all NaNs, signalling and quiet, of either sign, with random payloads"""
    g = torch.Generator().manual_seed(seed)
    payload = torch.randint(1, 1024, (n,), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 15
    word = 0x7C00 | payload | sign
    return torch.where(word >= 1 << 15, word - (1 << 16), word).to(torch.int16)


def guarded(shape, seed):
    """a contiguous fp16 tensor of `shape` inside a buffer with guard bands -> (buffer as int16, the tensor: a view into it)"""
    n = int(np.prod(shape))
    buf = nan_bits(n + 2 * GUARD, seed).to(DEV)
    t = buf[GUARD:GUARD + n].view(torch.float16).view(shape)
    assert t.data_ptr() % 16 == 0
    return buf, t


@functools.lru_cache(maxsize=None)
def op_case():
    """twelve records -- three shapes x (F = 8, L = 16 | F = 3, L = 12) x (a source of the destination's pitch | a compact one) -- with
    the expected destination buffers, computed once by slice copies on the bits"""
    from live2diff_amd import ops
    recs, dsts, srcs, want = [], [], [], []
    seed = 100
    for F_, L in ((8, 16), (3, 12)):
        for compact in (False, True):
            d, s = [], []
            for hw, C in SHAPES:
                db, dt = guarded((N, 2, hw, L, C), seed)
                sb, st = guarded((N, 2, hw, F_ if compact else L, C), seed + 1)
                seed += 2
                exp = db.clone()
                exp[GUARD:GUARD + dt.numel()].view(N, 2, hw, L, C)[:, :, :, :F_] = sb[GUARD:GUARD + st.numel()].view(st.shape)[:, :, :, :F_]
                d.append(dt), s.append(st)
                dsts.append((db, dt)), srcs.append((sb, sb.clone())), want.append(exp)
            recs.append(ops.sink_commit_table(d, s, F=F_))
    host = np.ascontiguousarray(np.concatenate(recs))
    dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(DEV)
    return dict(host=host, dev=dev, dsts=dsts, srcs=srcs, want=want, start=[db.clone() for db, _ in dsts])


def check_op(c, how):
    torch.cuda.synchronize()
    for j, ((db, _), (sb, s0), exp, start) in enumerate(zip(c["dsts"], c["srcs"], c["want"], c["start"])):
        bad = int((db != exp).sum())
        moved = int((db != start).sum())
        print(f"{how} record {j}: {bad} words differ from the slice copy, {moved} of {db.numel()} words changed")
        assert bad == 0, (how, j)
        assert moved > 0 and torch.equal(sb, s0), (how, j)
        assert torch.equal(db[:GUARD], start[:GUARD]) and torch.equal(db[-GUARD:], start[-GUARD:]), (how, j, "guards")


def test_sink_commit_moves_the_sinks_bit_for_bit_in_one_launch():
    from live2diff_amd import _lib, ops
    c = op_case()
    assert len(c["host"]) == 12
    op = ops.sink_commit(c["dev"], c["host"])
    ops.run(op)
    check_op(c, "direct")
    # the window slots of one record, spelt out: slots F..L-1 of every line are the start's
    db, dt = c["dsts"][1]
    assert torch.equal(bits(dt[:, :, :, 8:]), bits(c["start"][1][GUARD:GUARD + dt.numel()].view(torch.float16).view(dt.shape)[:, :, :, 8:]))
    # a second time through a captured graph, into destinations that were put back
    for (db, _), start in zip(c["dsts"], c["start"]):
        db.copy_(start)
    pl = _lib.OpList()
    pl.append(op[0], *op[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = _lib.Graph(pl, stream=int(side.cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for (db, _), start in zip(c["dsts"], c["start"]):
        assert torch.equal(db, start)                                        # (a capture launches nothing)
    graph.launch()
    check_op(c, "graph")


# ----------------------------------------------------------------------------- 2. - 5. the wrapper
def stream_state(w):
    s = w.stream
    ds = s._device_step
    return dict(window=[c[:, :, :, F:].clone() for c in s.kv_cache_list], in_sample=ds.st.in_sample.clone(), in_depth=ds.st.in_depth.clone(),
                bias=ds.attn_bias.clone(), pe=ds.pe_idx.clone(), upd=ds.update_idx.clone(), frame_ctr=ds.frame_ctr.clone(),
                prompt=s.prompt_embeds.clone(), init_noise=s.init_noise.clone(), gen=s.generator.get_state().clone(),
                rng=torch.cuda.get_rng_state(DEV).clone(), host_rng=torch.get_rng_state().clone(),
                ids=(id(ds), id(ds._graph), id(ds.pl), [id(c) for c in s.kv_cache_list], [c.data_ptr() for c in s.kv_cache_list]))


def sinks_of(w):
    return [c[:, :, :, :F].clone() for c in w.stream.kv_cache_list]


def data():
    from test_gpu_wrapper import u8_frames
    return u8_frames(8, 96, 128, seed=1), u8_frames(6, 96, 128, seed=2)


@functools.lru_cache(maxsize=None)
def runs():
    """a control without a re-warm, and the `__call__`-mode stream with `rewarm()` behind frame 2 and nothing else changed"""
    warm, frames = data()
    ctl = make_wrapper()
    ctl.prepare(warm, PROMPT)
    want = [ctl(f) for f in frames]
    w = make_wrapper()
    w.prepare(warm, PROMPT)
    got = [w(f) for f in frames[:3]]
    torch.cuda.synchronize()
    before, sinks_before = stream_state(w), sinks_of(w)
    gen = w.stream.rewarm_generator()
    w.rewarm()
    torch.cuda.synchronize()
    after, sinks_after = stream_state(w), sinks_of(w)
    got += [w(f) for f in frames[3:]]
    return dict(w=w, want=want, got=got, before=before, after=after, sinks_before=sinks_before, sinks_after=sinks_after, gen=gen)


def test_rewarm_with_nothing_changed_keeps_row_0_and_touches_nothing_else():
    r = runs()
    w = r["w"]
    assert w.rewarms == 1 and len(w.stream.inference_time_list) == 6
    for j, (a, b) in enumerate(zip(r["sinks_before"], r["sinks_after"])):
        assert float(a[0].float().abs().max()) > 0 and same(a[0], b[0]), f"layer {j}: row 0's sinks moved"
        assert not same(a[1:], b[1:]), f"layer {j}: rows >= 1 drew the same noise as prepare"
    for k in ("in_sample", "in_depth", "bias", "pe", "upd", "frame_ctr", "prompt", "init_noise", "gen", "rng", "host_rng"):
        assert same(r["before"][k], r["after"][k]), k
    assert all(same(a, b) for a, b in zip(r["before"]["window"], r["after"]["window"]))
    assert r["before"]["ids"] == r["after"]["ids"]


def test_rows_are_the_loop_restated_with_public_calls():
    r = runs()
    s = r["w"].stream
    unet = s.unet
    scratch = unet.prepare_cache(N)
    x, d = s.warmup_window
    gen = r["gen"]
    for idx, t in enumerate(s.sub_timesteps_tensor):
        pred = unet.warmup(x, t.view(1), encoder_hidden_states=s.prompt_embeds[0:1], depth_sample=d, kv_cache=scratch, row=idx)["sample"]
        x0 = s.scheduler_step_batch(pred, x, idx)
        if idx < N - 1:
            x = s.alpha_prod_t_sqrt[idx + 1] * x0 + s.beta_prod_t_sqrt[idx + 1] * torch.randn(x0.shape, generator=gen, device=DEV, dtype=x0.dtype)
    torch.cuda.synchronize()
    for j, (c, got) in enumerate(zip(scratch, r["sinks_after"])):
        assert same(c[:, :, :, :F], got), f"layer {j}"
        assert not c[:, :, :, F:].any()                                       # (the warm-up pass fills slots 0..F-1 and nothing else)


def test_frames_after_a_rewarm_differ_from_a_run_without():
    r = runs()
    for i in range(3):
        assert np.array_equal(r["got"][i], r["want"][i]), f"frame {i}: before the re-warm the stream is the control"
    for i in range(3, 6):
        assert not np.array_equal(r["got"][i], r["want"][i]), f"frame {i}: the sinks of rows >= 1 changed, the frame did not"


def test_row_0_after_a_style_switch_is_that_of_a_stream_switched_before_prepare():
    warm, frames = data()
    w = make_wrapper()
    w.prepare(warm, PROMPT)
    add_b(w)
    for f in frames[:3]:
        w(f)
    torch.cuda.synchronize()
    before = sinks_of(w)
    kv_ids = [id(c) for c in w.stream.kv_cache_list]
    w.set_style("b", rewarm=True)
    torch.cuda.synchronize()
    assert w.rewarms == 1 and w.style == {"b": 1.0} and [id(c) for c in w.stream.kv_cache_list] == kv_ids
    ctl = make_wrapper()
    add_b(ctl)
    ctl.set_style("b")
    ctl.prepare(warm, PROMPT)
    torch.cuda.synchronize()
    assert same(w.stream.prompt_embeds, ctl.stream.prompt_embeds) and same(w.stream.warmup_window[0], ctl.stream.warmup_window[0])
    for j, (mine, old, want) in enumerate(zip(sinks_of(w), before, sinks_of(ctl))):
        assert torch.isfinite(want[0].float()).all() and same(mine[0], want[0]), f"layer {j}: row 0 is not the control's"
        assert not same(mine[0], old[0]), f"layer {j}: row 0 is still the old style's"
    out = w(frames[3])
    assert out.shape == (64, 64, 3)


def test_push_pop_with_a_frame_pending_across_the_rewarm():
    r = runs()
    warm, frames = data()
    wp = make_wrapper(frame_pipelining=True)
    wp.prepare(warm, PROMPT)
    out = []
    wp.push(frames[0])
    for i in range(6):
        if i + 1 < 6:
            wp.push(frames[i + 1])
        out.append(wp.pop())
        if i == 2:
            assert len(wp.stream._pending) == 1                                  # frame 3 is pushed and not yet popped
            wp.rewarm()
    torch.cuda.synchronize()
    for i in range(6):
        assert np.array_equal(out[i], r["got"][i]), f"push / pop frame {i} differs from __call__ with the re-warm behind frame 2"
    assert wp.rewarms == 1


def test_recent_is_rewarm_fed_with_the_latents_that_entered_row_0():
    r = runs()
    warm, frames = data()
    from test_gpu_wrapper import u8_frames
    more = list(frames) + list(u8_frames(5, 96, 128, seed=3))                   # 11 frames: the ring of 8 wraps round
    w = make_wrapper(keep_recent=True)
    w.prepare(warm, PROMPT)
    with pytest.raises(ValueError, match="0 frames since prepare"):
        w.rewarm("recent")
    s = w.stream
    entered, step = [], s.predict_x0_batch
    s.predict_x0_batch = lambda x, d, **kw: (entered.append((x.clone(), d.clone())), step(x, d, **kw))[1]
    out = [w(f) for f in more]
    for i in range(6):
        assert np.array_equal(out[i], r["want"][i]), f"frame {i}: keeping the recent window changed the stream"
    x = torch.cat([e[0] for e in entered[-F:]], dim=2)
    d = torch.cat([e[1] for e in entered[-F:]], dim=2)
    rx, rd = s.recent_window()
    assert same(rx, x) and same(rd, d)                                           # oldest first, after the wrap
    gen = s.rewarm_generator()
    w.rewarm("recent")
    torch.cuda.synchronize()
    got = sinks_of(w)
    s.rewarm(x, d, generator=gen)
    torch.cuda.synchronize()
    assert w.rewarms == 2
    for j, (a, b) in enumerate(zip(got, sinks_of(w))):
        assert float(a.float().abs().max()) > 0 and same(a, b), f"layer {j}"
    assert not same(got[0][0], r["sinks_before"][0][0])                           # (other frames than the warm-up window's)
