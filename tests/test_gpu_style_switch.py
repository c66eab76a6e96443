"""-m gpu: style switch and style blend from resident packed weight sets.

  1. L2D_OP_WEIGHT_BLEND against `style_bank.blend_ref`, bit for bit, over every path of the kernel;
  2. a switch is exact: an instance streaming on style A that does `load_mix([B], [1.0])` equals a fresh instance built from B;
  3. instances that share W follow a switch made through one of them;
  4. a blend means what it says: the 50/50 mix of two strengths of one LoRA meets the whole-UNet bound against the fp32 oracle
     evaluated on the state dict merged at the mixed strength;
  5. the wrapper mid-stream, in `__call__` and in push / pop mode.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 64
N = 2


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- 1. the kernel
SIZES = [("h1", torch.float16, 1), ("h7", torch.float16, 7), ("h8", torch.float16, 8), ("h9", torch.float16, 9),
         ("h4097", torch.float16, 4097), ("h1m", torch.float16, 1 << 20), ("f3", torch.float32, 3), ("f1025", torch.float32, 1025)]
MIXES = [[1.0], [-0.5, 1.5], [0.3, 0.3, 0.4], [0.1, 0.2, 0.3, 0.4]]


@functools.lru_cache(maxsize=None)
def synthetic():
    """four source sets on the host and on the device, and the reference of every mix, computed once"""
    from live2diff_amd.style_bank import blend_ref
    g = torch.Generator().manual_seed(5)
    srcs = []
    for k in range(4):
        s = {name: torch.randn(n, generator=g).to(dt) for name, dt, n in SIZES}
        s["f1025"][:4] = torch.tensor([-0.0, 1e-40, 1.0e38, -1.0])            # signed zero, a denormal, a large value
        s["h4097"][-3:] = torch.tensor([-0.0, 6e-8, 65504.0], dtype=torch.float16)
        rows = torch.randn(5000, 9, generator=g).to(torch.float16)              # more records than the launch has work-groups
        s.update({f"row{i}": rows[i] for i in range(5000)})
        srcs.append(s)
    refs = [blend_ref(srcs[:len(w)], w) for w in MIXES]
    return srcs, refs


@pytest.mark.parametrize("nt", [0, 1])
def test_kernel_matches_blend_ref_bit_for_bit(nt):
    from live2diff_amd.style_bank import WeightBlender
    srcs, refs = synthetic()
    pad = {torch.float16: 8, torch.float32: 4}                                # 16 canary bytes behind every destination
    bufs, dst = {}, {}
    for name, dt, n in SIZES:
        bufs[name] = torch.empty(n + pad[dt], dtype=dt, device=DEV)
        dst[name] = bufs[name][:n]
    rows = torch.empty(5000, 64, dtype=torch.float16, device=DEV)              # row{i} = 9 elements of a 128-byte row: the rest is canary
    dst.update({f"row{i}": rows[i, :9] for i in range(5000)})
    dsrc = []
    for s in srcs:
        r = torch.zeros(5000, 64, dtype=torch.float16, device=DEV)             # (every row 16-byte aligned, like the destination's)
        r[:, :9] = torch.stack([s[f"row{i}"] for i in range(5000)]).to(DEV)
        d = {name: s[name].to(DEV) for name, _, _ in SIZES}
        d.update({f"row{i}": r[i, :9] for i in range(5000)})
        dsrc.append(d)
    wb = WeightBlender(dst, DEV)

    def poison():
        for name, dt, n in SIZES:
            bufs[name].fill_(float("nan"))
            bufs[name][n:].view(torch.uint8).copy_(torch.arange(16, dtype=torch.uint8) + 0xA0)
        rows.fill_(float("nan"))
        rows[:, 9:] = 1234.0

    for w, ref in zip(MIXES, refs):
        K = len(w)
        poison()
        wb.apply(dsrc[:K], w, nt=nt)
        torch.cuda.synchronize()
        first = {k: v.clone() for k, v in dst.items() if not k.startswith("row")}
        first_rows = rows.clone()
        assert len(wb._table(dsrc[:K])[1]) == 5 + 32 + 2 + 5000                 # tiles: 2^20 halves are 32, the others one each
        for name, dt, n in SIZES:
            bad = int((bits(dst[name]) != bits(ref[name])).sum())
            print(f"K={K} nt={nt} {name}: {bad} differing bytes")
            assert bad == 0, (K, name)
            assert bits(bufs[name][n:]).tolist() == list(range(0xA0, 0xB0)), (K, name, "canary")
        want_rows = torch.stack([ref[f"row{i}"] for i in range(5000)])
        assert torch.equal(bits(rows[:, :9]), bits(want_rows)), K
        assert bool((rows[:, 9:] == 1234.0).all()), (K, "bytes behind a 9-element row were written")
        wb.apply(dsrc[:K], w, nt=nt)                                             # again into the same table
        torch.cuda.synchronize()
        assert all(same(dst[k], v) for k, v in first.items()) and same(rows, first_rows), K
    # a one-hot mix of four is the K = 1 copy
    poison()
    wb.apply(dsrc, [0.0, 0.0, 1.0, 0.0], nt=nt)
    torch.cuda.synchronize()
    assert all(same(dst[name], srcs[2][name]) for name, _, _ in SIZES)


# ----------------------------------------------------------------------------- shared: two styles of the tiny UNet
@functools.lru_cache(maxsize=None)
def env():
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import device_random_state_dict
    ccfg = tiny_clip_config()
    cfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    sd_a = device_random_state_dict(cfg, DEV)
    sd_b = {k: torch.roll(v, 1, 0).contiguous() for k, v in sd_a.items()}     # style B: the same distribution, other weights
    h, w = H // 8, W // 8
    mk = lambda sd: HipStreamingUNet(sd, cfg, h, w, N, device=DEV)
    # plan-less instances: all they cost is their weights
    return dict(cfg=cfg, ccfg=ccfg, sd_a=sd_a, sd_b=sd_b, mk=mk, set_a=mk(sd_a).packed_state(), set_b=mk(sd_b).packed_state())


def stream_inputs(cfg, n_frames, seed=21):
    from live2diff_amd.pipeline_stream_animation_depth import ring_buffer_init, ring_buffer_update
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float16)
    h, w = H // 8, W // 8
    rb = ring_buffer_init(N, cfg.window_size, cfg.sink_size)
    frames = []
    for _ in range(n_frames):
        frames.append(dict(x=rn(N, 4, 1, h, w), d=rn(N, 4, 1, h, w), bias=rb[0].half().to(DEV), pe=rb[1].to(DEV), upd=rb[2].to(DEV)))
        ring_buffer_update(*rb, cfg.window_size, cfg.sink_size)
    return dict(enc=rn(N, 77, cfg.cross_attention_dim), ts=torch.tensor([399, 199][:N], device=DEV), frames=frames)


def call(unet, inp, f, kv):
    fr = inp["frames"][f]
    out = unet(fr["x"], inp["ts"], encoder_hidden_states=inp["enc"], temporal_attention_mask=fr["bias"], depth_sample=fr["d"],
               kv_cache=kv, pe_idx=fr["pe"], update_idx=fr["upd"])["sample"].clone()
    torch.cuda.synchronize()
    return out


def random_caches(unet, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    kv = unet.prepare_cache(N)
    for c in kv:
        c.normal_(generator=g)
    return kv


# ----------------------------------------------------------------------------- 2. a switch is exact
def test_switch_is_exact_through_the_boundary_call():
    e = env()
    inp = stream_inputs(e["cfg"], 4)
    u = e["mk"](e["sd_a"])
    kv = random_caches(u, 3)
    for f in range(2):
        call(u, inp, f, kv)                                                     # streaming on A: plan built, conditioning cached
    sd_before = {k: v.clone() for k, v in e["sd_a"].items()}
    w_a = {k: v.clone() for k, v in u.W.items()}
    print("tensors of another pack of A's state dict that differ from the active W:", [k for k in w_a if not same(e["set_a"].W[k], w_a[k])][:8])
    plans, ptrs = dict(u._plans), {k: v.data_ptr() for k, v in u.W.items()}
    u.load_mix([e["set_b"]], [1.0])
    odd = [k for k in u.W if not same(u.W[k], e["set_b"].W[k])]
    print("tensors that differ from their source after the switch:", odd[:8])
    assert not odd
    fresh = e["mk"](e["sd_b"])
    kv_f = [c.clone() for c in kv]
    for f in (2, 3):
        got, want = call(u, inp, f, kv), call(fresh, inp, f, kv_f)
        assert torch.isfinite(want.float()).all() and same(got, want), f
        assert all(same(a, b) for a, b in zip(kv, kv_f)), f
    assert not torch.equal(call(e["mk"](e["sd_a"]), inp, 2, [c.clone() for c in kv]), want)    # (A and B do differ on these inputs)
    assert u._plans == plans and {k: v.data_ptr() for k, v in u.W.items()} == ptrs             # nothing was rebuilt or re-allocated
    # A -> B -> A restores every tensor of W bit for bit
    assert all(same(e["sd_a"][k], v) for k, v in sd_before.items())                            # the switch wrote into W, not into the state dict
    assert all(same(e["set_a"].W[k], w_a[k]) for k in w_a)                                     # ... nor into another instance's pack of it
    u.load_mix([e["set_a"]], [1.0])
    torch.cuda.synchronize()
    odd = [k for k in w_a if not same(u.W[k], w_a[k])]
    print("tensors that A -> B -> A did not restore:", odd[:8])
    assert not odd


def test_switch_is_exact_under_a_captured_device_step():
    from live2diff_amd.scheduler import LCMSchedule
    from live2diff_amd.stream_step_hip import HipStreamStep
    e = env()
    cfg = e["cfg"]
    h, w = H // 8, W // 8
    g = torch.Generator(device=DEV).manual_seed(31)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float16)
    sch = LCMSchedule()
    sch.set_timesteps(50)
    ts_list = [399, 199][:N]
    shp = (N, 1, 1, 1, 1)
    to = dict(device=DEV, dtype=torch.float16)
    al = torch.tensor([float(sch.alphas_cumprod[t]) ** 0.5 for t in ts_list]).view(shp).to(**to)
    be = torch.tensor([(1 - float(sch.alphas_cumprod[t])) ** 0.5 for t in ts_list]).view(shp).to(**to)
    sc = [sch.get_scalings_for_boundary_condition_discrete(t) for t in ts_list]
    cs, co = (torch.tensor([float(c[j]) for c in sc]).view(shp).to(**to) for j in (0, 1))
    ts, enc = torch.tensor(ts_list, device=DEV), rn(N, 77, cfg.cross_attention_dim)
    new = [(rn(1, 4, 1, h, w), rn(1, 4, 1, h, w), rn(N - 1, 4, 1, h, w)) for _ in range(6)]

    def stepper(unet, kv, ring_state=None):
        return HipStreamStep(unet, kv, ts, enc, al, be, cs, co, inject_noise=True, use_graph=True, ring_state=ring_state)

    def run(step, f):
        step.noise.copy_(new[f][2].reshape(-1))
        out = step.step(new[f][0], new[f][1]).clone()
        torch.cuda.synchronize()
        return out

    u = e["mk"](e["sd_a"])
    kv = random_caches(u, 4)
    sa = stepper(u, kv)
    sa.load_buffers(rn(N - 1, 4, 1, h, w), rn(N - 1, 4, 1, h, w))
    for f in range(3):
        run(sa, f)                                                              # frame 0 runs directly, frames 1 and 2 replay the graph
    graph = sa._graph
    assert graph is not None
    u.load_mix([e["set_b"]], [1.0])
    fresh = e["mk"](e["sd_b"])
    kv_f = [c.clone() for c in kv]
    sb = stepper(fresh, kv_f, ring_state=(sa.attn_bias.float().cpu(), sa.pe_idx.cpu(), sa.update_idx.cpu()))
    sb.load_buffers(sa.st.in_sample[1:].clone(), sa.st.in_depth[1:].clone())
    sb.frame_ctr.copy_(sa.frame_ctr)
    for f in (3, 4, 5):                                                         # the fresh step: directly, then its own graph
        got, want = run(sa, f), run(sb, f)
        assert torch.isfinite(want.float()).all() and same(got, want), f
        assert all(same(a, b) for a, b in zip(kv, kv_f)), f
        assert same(sa.st.in_sample, sb.st.in_sample) and same(sa.attn_bias, sb.attn_bias), f
    assert sa._graph is graph                                                   # the captured graph was replayed, not rebuilt


# ----------------------------------------------------------------------------- 3. sharers follow
def test_instances_that_share_w_follow_a_switch():
    from live2diff_amd.unet_hip import HipStreamingUNet
    e = env()
    cfg = e["cfg"]
    inp = stream_inputs(cfg, 3, seed=22)
    u1 = e["mk"](e["sd_a"])
    u2 = HipStreamingUNet(u1, cfg, H // 8, W // 8, N, device=DEV)
    assert u2.W is u1.W
    kv1, kv2 = random_caches(u1, 5), random_caches(u2, 6)
    call(u1, inp, 0, kv1)
    call(u2, inp, 0, kv2)
    st2 = u2._plans["stream"]
    assert st2.cond_key is not None and st2.w_gen == 0
    before = {name: getattr(st2, name).clone() for name in ("temb_all", "text_k", "text_vt")}
    u1.load_mix([e["set_b"]], [1.0])                                            # the switch goes through ONE of them
    fresh = e["mk"](e["sd_b"])
    kv_f = [c.clone() for c in kv2]
    got, want = call(u2, inp, 1, kv2), call(fresh, inp, 1, kv_f)                # the same tensors as before: only the generation says "stale"
    assert same(got, want) and all(same(a, b) for a, b in zip(kv2, kv_f))
    assert st2.w_gen == 1
    # its time-embedding rows and text K / V^T were recomputed: they are the fresh instance's
    stf = fresh._plans["stream"]
    for name in ("temb_all", "text_k", "text_vt"):
        assert not same(getattr(st2, name), before[name]) and same(getattr(st2, name), getattr(stf, name)), name
    got, want = call(u2, inp, 2, kv2), call(fresh, inp, 2, kv_f)                # ... and stay cached afterwards
    assert same(got, want)


# ----------------------------------------------------------------------------- 4. a blend means what it says
def lora_for(sd, rank=4, scale=1.0, seed=9):
    """a kohya LoRA over every attention projection of the spatial transformers"""
    g = torch.Generator().manual_seed(seed)
    lora = {}
    for k, v in sd.items():
        if v.dim() == 2 and ".transformer_blocks." in k and k.endswith(("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight")) \
                and ".attentions." in k:
            name = "lora_unet_" + k[: -len(".weight")].replace(".", "_")
            lora[name + ".lora_down.weight"] = torch.randn(rank, v.shape[1], generator=g) * v.shape[1] ** -0.5
            lora[name + ".lora_up.weight"] = torch.randn(v.shape[0], rank, generator=g) * (scale * rank ** -0.5)
    return lora


# The LoRA's magnitude: with the fp32 oracle on the CPU, the alpha = 0 network is rel-L2 1.2e-1 / cosine 0.9926 away from the
# alpha = 0.5 one at this scale (6e-2 / 0.9982 at half of it) -- twelve times the bound the blend has to meet, so a blend that came
# out as its first source (or as any other strength) fails; the test asserts this validity condition on the device too.
LORA_SCALE = 0.25


def test_half_way_between_two_lora_strengths_is_the_lora_at_half_strength():
    """SURVEY 8c's whole-UNet bound (rel-L2 <= 1e-2, cosine >= 0.9995) for `load_mix([S0, S1], [0.5, 0.5])` against the fp32 oracle
    on the state dict merged at alpha = 0.5."""
    from live2diff_amd import convert
    from live2diff_amd.pipeline_stream_animation_depth import ring_buffer_init
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import random_state_dict
    from oracle import unet_ref as O
    e = env()
    cfg = e["cfg"]
    h, w = H // 8, W // 8
    base = random_state_dict(cfg, dtype=torch.float16)
    lora = lora_for(base, scale=LORA_SCALE)

    def merged(alpha, dtype):
        sd = {k: v.to(dtype) for k, v in base.items()}
        touched = convert.merge_lora(sd, lora, alpha=alpha, strict=True)
        assert len(touched) == len(lora) // 2 > 0
        return sd

    mk = lambda sd: HipStreamingUNet({k: v.to(DEV) for k, v in sd.items()}, cfg, h, w, N, device=DEV)
    u0 = mk(base)
    s0, s1 = mk(base).packed_state(), mk(merged(1.0, torch.float16)).packed_state()
    g = torch.Generator().manual_seed(41)
    rn = lambda *s: torch.randn(*s, generator=g).half()
    x, d, enc, ts = rn(N, 4, 1, h, w), rn(N, 4, 1, h, w), rn(1, 77, cfg.cross_attention_dim).repeat(N, 1, 1), torch.tensor([399, 199][:N])
    rb = ring_buffer_init(N, cfg.window_size, cfg.sink_size)
    kv_ref = O.alloc_kv_cache(cfg, h, w, N)
    for c in kv_ref:
        c.copy_(torch.randn(c.shape, generator=g).half())
    kv = [c.half().to(DEV) for c in kv_ref]
    ref = O.unet_forward(merged(0.5, torch.float32), cfg, x.float(), ts, enc.float(), d.float(), [c.clone() for c in kv_ref],
                         temporal_attention_mask=rb[0].clone(), pe_idx=rb[1].clone(), update_idx=rb[2].clone())

    def run(unet):
        out = unet(x.to(DEV), ts.to(DEV), encoder_hidden_states=enc.to(DEV), temporal_attention_mask=rb[0].half().to(DEV),
                   depth_sample=d.to(DEV), kv_cache=[c.clone() for c in kv], pe_idx=rb[1].to(DEV), update_idx=rb[2].to(DEV))["sample"]
        torch.cuda.synchronize()
        return out.double().cpu()

    def rel_cos(out):
        r = ref.double()
        return ((out - r).norm() / r.norm()).item(), (out.flatten() @ r.flatten() / (out.norm() * r.norm())).item()

    r0, c0 = rel_cos(run(u0))
    print(f"alpha = 0 network vs alpha = 0.5 oracle: rel-L2 {r0:.3e} cos {c0:.6f}")
    assert r0 > 1e-2 or c0 < 0.9995, "validity: the LoRA is too weak to tell the blend from its first source"
    u0.load_mix([s0, s1], [0.5, 0.5])
    r, c = rel_cos(run(u0))
    print(f"50/50 blend vs alpha = 0.5 oracle: rel-L2 {r:.3e} cos {c:.6f}")
    assert r <= 1e-2 and c >= 0.9995, (r, c)


# ----------------------------------------------------------------------------- 5. the wrapper mid-stream
PROMPT = "a cat, paper folding"
SEED = 11


@functools.lru_cache(maxsize=None)
def wrapper_runs():
    """the `__call__`-mode stream with a switch after three frames, and a control without one"""
    from test_gpu_wrapper import u8_frames
    warm, frames = u8_frames(8, 96, 128, seed=1), u8_frames(6, 96, 128, seed=2)
    ctl = make_wrapper()
    ctl.prepare(warm, PROMPT)
    want = [ctl(f) for f in frames]
    w = make_wrapper()
    w.prepare(warm, PROMPT)
    add_b(w)
    kv_ids = [id(c) for c in w.stream.kv_cache_list]
    got = [w(f) for f in frames[:3]]
    sink = w.stream.unet.cfg.sink_size
    sinks = [c[:, :, :, :sink].clone() for c in w.stream.kv_cache_list]
    w.set_style("b")
    got += [w(f) for f in frames[3:]]
    return dict(w=w, got=got, want=want, warm=warm, frames=frames, kv_ids=kv_ids, sinks=sinks)


def make_wrapper(**more):
    from test_gpu_wrapper import Parts
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    e = env()
    parts = Parts(e["cfg"], e["ccfg"], H, W, N)                                # (its own packed weights: a switch reaches every sharer)
    torch.manual_seed(0)
    return Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, num_inference_steps=50, t_index_list=[30, 40],
                                   width=W, height=H, warmup_frames=e["cfg"].sink_size, window_size=e["cfg"].window_size, **more)


def clip_sd_b():
    from live2diff_amd.clip_hip import random_clip_text_state_dict
    return random_clip_text_state_dict(env()["ccfg"], 4)


def add_b(w):
    w.add_style("b", unet_state_dict=env()["sd_b"], text_state_dict=clip_sd_b())


def test_wrapper_switches_mid_stream():
    from test_gpu_wrapper import HERE as TESTS
    from live2diff_amd.clip_hip import HipClipTextEncoder, HipPromptEncoder
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    r = wrapper_runs()
    w, got, want = r["w"], r["got"], r["want"]
    assert w.styles == ["default", "b"] and w.style == {"b": 1.0}
    assert len(w.stream.inference_time_list) == 6
    for i in range(3):
        assert np.array_equal(got[i], want[i]), f"frame {i}: before the switch the stream is the control"
    for i in range(3, 6):
        assert not np.array_equal(got[i], want[i]), f"frame {i}: after the switch it is not"
    # the KV caches are the same objects and still hold what `prepare` wrote: the sink slots never age out
    assert [id(c) for c in w.stream.kv_cache_list] == r["kv_ids"]
    for c, s in zip(w.stream.kv_cache_list, r["sinks"]):
        assert float(s.float().abs().max()) > 0 and torch.equal(c[:, :, :, : s.shape[3]], s)
    # the prompt was re-encoded by the new text encoder
    tok = ClipTokenizer.from_dir(os.path.join(TESTS, "golden", "clip_tok"))
    penc = HipPromptEncoder(HipClipTextEncoder(clip_sd_b(), DEV, env()["ccfg"]), tok, default_clip_skip=1)
    emb = penc._encode_prompt(PROMPT, DEV, 1, False)[0]
    torch.cuda.synchronize()
    assert same(w.stream.prompt_embeds, emb.to(torch.float16).repeat(N, 1, 1))
    # back to the constructor's style: its copy, bit for bit
    w.set_style("default")
    torch.cuda.synchronize()
    kept = w._bank.sets["default"][0].W
    odd = [k for k in kept if not same(w.stream.unet.W[k], kept[k])]
    print("tensors that differ from the kept copy:", odd[:8])
    assert not odd


def test_wrapper_switches_with_a_frame_pending_in_push_pop_mode():
    r = wrapper_runs()
    frames, got = r["frames"], r["got"]
    wp = make_wrapper(frame_pipelining=True)
    wp.prepare(r["warm"], PROMPT)
    add_b(wp)
    out = []
    wp.push(frames[0])
    for i in range(6):
        if i + 1 < 6:
            wp.push(frames[i + 1])
        out.append(wp.pop())
        if i == 2:
            assert len(wp.stream._pending) == 1                                  # frame 3 was pushed under the old style ...
            wp.set_style("b")                                                    # ... and is popped under the new one
    torch.cuda.synchronize()
    for i in range(6):
        assert np.array_equal(out[i], got[i]), f"push / pop frame {i} differs from __call__ with the switch behind frame 2"
    assert len(wp.stream.inference_time_list) == 6
