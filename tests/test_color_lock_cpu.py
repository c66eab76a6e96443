"""CPU tests (-m "not gpu") of live2diff_amd/color_lock.py: the exact-integer statistics against a direct numpy computation, the
2^22-pixel bound, the identities of `lock_ref`, moment matching on unclipped frames, the launchers' argument checks (dry-run), and
`set_color_lock` / `clear_color_lock` on the wrapper built from the mock components of tests/pipeline_mocks.py: every served
output type, the lock under a matte, dropped frames, `prepare`, and the delay line the lock shares with the matte."""
import numpy as np
import pytest
import torch

from live2diff_amd import color_lock as CL
from live2diff_amd.frame_io import egress_ref
from test_matte_cpu import build, colour


def gauss(rng, H, W):
    """activation-like and unclipped: N(offset, sigma) per channel, sigma 0.1 .. 0.25, offset within +-0.3"""
    return (rng.standard_normal((3, H, W)) * rng.uniform(0.1, 0.25, (3, 1, 1)) + rng.uniform(-0.3, 0.3, (3, 1, 1))).astype(np.float16)


def bits(x):
    return np.asarray(x).view(np.uint16 if np.asarray(x).dtype == np.float16 else np.uint64)


# ----------------------------------------------------------------------------- the statistics
@pytest.mark.parametrize("shape", [(8, 8), (24, 40), (65, 64), (128, 128)])
def test_moments_ref_against_direct_int64(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = (rng.standard_normal((3, *shape)) * 0.7).astype(np.float16)
    x.reshape(3, -1)[:, :8] = np.array([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8, -6e-8, 3e-5], dtype=np.float16)
    b = egress_ref(torch.from_numpy(x))[0].numpy().astype(np.int64)                    # [H,W,3]
    n = shape[0] * shape[1]
    S1, S2, n_ = CL.sums_ref(x)
    assert n_ == n and S1.dtype == S2.dtype == np.int64
    got = CL.moments_ref(x)
    assert got.dtype == np.float64 and got.shape == (3, 2)
    for c in range(3):
        s1, s2 = int(b[..., c].sum()), int((b[..., c] ** 2).sum())
        assert (int(S1[c]), int(S2[c])) == (s1, s2)
        assert got[c, 0] == np.float64(s1) / np.float64(n)
        assert got[c, 1] == np.float64(n * s2 - s1 * s1) / np.float64(n * n)           # (Python integers: no overflow to hide)
        assert abs(got[c, 0] - b[..., c].mean()) < 1e-9 and abs(got[c, 1] - b[..., c].astype(np.float64).var()) < 1e-6
    assert np.array_equal(CL.moments_ref(torch.from_numpy(x)[None]), got)             # a [1,3,H,W] tensor is the same frame


def test_bound_at_two_to_the_22_pixels():
    """n = 2^22 is served and exact -- half the pixels 0 and half 255 is the largest n S2 - S1^2 there is -- and one row more is refused"""
    H, W = 2048, 2048
    x = np.full((3, H, W), -1.0, dtype=np.float16)
    x[:, : H // 2] = 1.0
    x[2] = 1.0                                                                         # S1 and S2 at their maxima, variance 0
    S1, S2, n = CL.sums_ref(x)
    assert n == 1 << 22 == CL.MAX_PIXELS
    assert [int(v) for v in S1] == [255 * n // 2, 255 * n // 2, 255 * n] and [int(v) for v in S2] == [65025 * n // 2, 65025 * n // 2, 65025 * n]
    m = CL.moments_from_sums(S1, S2, n)
    assert np.array_equal(m, np.array([[127.5, 127.5 ** 2], [127.5, 127.5 ** 2], [255.0, 0.0]]))
    assert n * int(S2[0]) - int(S1[0]) ** 2 == n * n * 65025 // 4 < 1 << 63
    big = np.zeros((3, H + 1, W), dtype=np.float16)
    for f in (CL.sums_ref, CL.moments_ref, lambda t: CL.lock_ref(t, None, mode="ema", init=True)):
        with pytest.raises(ValueError, match="pixels"):
            f(big)
    with pytest.raises(ValueError):
        CL.HipColorLock(H + 1, W, device="cpu")


# ----------------------------------------------------------------------------- identities of lock_ref
def test_strength_zero_returns_the_input():
    """frames inside [-1, 1], as `decode_image` returns them (a value beyond +-1 is clamped, whatever the strength): bit for bit,
    but for the sign of a zero"""
    rng = np.random.default_rng(1)
    for k, (H, W) in enumerate([(16, 16), (24, 40), (64, 64)]):
        x = gauss(rng, H, W) if k else np.clip(rng.standard_normal((3, H, W)) * 0.7, -1, 1).astype(np.float16)
        x.reshape(3, -1)[:, :6] = np.array([-1.0, 1.0, 0.0, -0.0, 6e-8, 3e-5], dtype=np.float16)
        for mode, kw in (("source", dict(source=gauss(rng, H, W))), ("ema", dict(init=False)), ("image", {})):
            out, _, coef = CL.lock_ref(x, CL.moments_ref(gauss(rng, H, W)), mode=mode, strength=0.0, with_coefficients=True, **kw)
            assert out.dtype == np.float16 and out.shape == (1, 3, H, W)
            assert np.array_equal(coef[:, 0], np.ones(3, np.float32)) and np.array_equal(coef[:, 1], coef[:, 2])
            keep = bits(x) != 0x8000                                  # (x - s) + s is +0 for x = -0: the same value, the same byte
            assert np.array_equal(out[0], x) and np.array_equal(bits(out[0])[keep], bits(x)[keep]), (H, W, mode)


def test_flat_frame_gets_gain_one_and_the_target_mean():
    H, W = 16, 24
    flat = np.full((3, H, W), 0.25, dtype=np.float16)
    target = gauss(np.random.default_rng(2), H, W)
    want = CL.moments_ref(target)
    out, state, coef = CL.lock_ref(flat, None, mode="source", source=target, with_coefficients=True)
    assert np.array_equal(state, want) and np.array_equal(coef[:, 0], np.ones(3, np.float32))
    got = CL.moments_ref(out)
    assert np.all(got[:, 1] == 0.0) and np.all(np.abs(got[:, 0] - want[:, 0]) <= 0.5)                # one byte value: the nearest one
    # and a flat TARGET leaves the contrast alone
    x = gauss(np.random.default_rng(3), H, W)
    _, _, coef = CL.lock_ref(x, None, mode="source", source=flat, with_coefficients=True)
    assert np.array_equal(coef[:, 0], np.ones(3, np.float32))


def test_gain_clamps():
    own = np.array([[100.0, 4.0]] * 3)
    for var_t, g in ((4.0 * 16.0, 4.0), (4.0 * 17.0, 4.0), (4.0 * 1e6, 4.0), (4.0 / 16.0, 0.25), (4.0 / 17.0, 0.25), (1e-30, 0.25),
                     (4.0 * 9.0, 3.0), (1.0, 0.5)):
        coef = CL.coefficients_ref(own, np.array([[100.0, var_t]] * 3), 1.0)
        assert np.array_equal(coef[:, 0], np.full(3, g, np.float32)), var_t
    half = CL.coefficients_ref(own, np.array([[100.0, 1e9]] * 3), 0.5)
    assert np.array_equal(half[:, 0], np.full(3, 2.5, np.float32))                                    # 1 + a (4 - 1)
    # a near-flat frame against a lively target: the clamp, on frames
    rng = np.random.default_rng(4)
    near_flat = (0.1 + 0.004 * rng.standard_normal((3, 16, 16))).astype(np.float16)
    _, _, coef = CL.lock_ref(near_flat, None, mode="source", source=gauss(rng, 16, 16), with_coefficients=True)
    assert np.array_equal(coef[:, 0], np.full(3, 4.0, np.float32))


def test_ema_first_frame_copies_then_follows():
    rng = np.random.default_rng(5)
    a, b = gauss(rng, 24, 40), gauss(rng, 24, 40)
    junk = np.full((3, 2), np.nan)
    _, s0 = CL.lock_ref(a, junk, mode="ema", rate=0.25, init=True)
    assert np.array_equal(s0, CL.moments_ref(a))
    _, s0_none = CL.lock_ref(a, None, mode="ema", init=True)
    assert np.array_equal(s0_none, s0)
    _, s1 = CL.lock_ref(b, s0, mode="ema", rate=0.25)
    c = CL.moments_ref(b)
    assert np.array_equal(s1, s0 + np.float64(0.25) * (c - s0)) and not np.array_equal(s1, s0)
    _, s_full = CL.lock_ref(b, s0, mode="ema", rate=1.0)
    assert np.allclose(s_full, c, rtol=1e-15, atol=0)


def test_frozen_reference_never_changes_state():
    rng = np.random.default_rng(6)
    ref = CL.moments_ref(gauss(rng, 16, 16))
    state = ref.copy()
    for _ in range(4):
        out, state = CL.lock_ref(gauss(rng, 16, 16), state, mode="image", init=True)
        assert np.array_equal(bits(state), bits(ref))
    assert state is not ref


# ----------------------------------------------------------------------------- moment matching
@pytest.mark.parametrize("shape", [(16, 16), (24, 40), (64, 64), (512, 512)])
def test_moment_matching_on_unclipped_frames(shape):
    """after the lock at strength 1 the byte mean is within 0.25 of the target's and the byte standard deviation within 2 %
    (seen on the oracle: at most 0.098 and 0.69 %)"""
    rng = np.random.default_rng(shape[0] + shape[1])
    worst_m = worst_s = 0.0
    for _ in range(20 if shape[0] < 512 else 4):
        styled, target = gauss(rng, *shape), gauss(rng, *shape)
        out, state = CL.lock_ref(styled, None, mode="source", source=target)
        got, want = CL.moments_ref(out), CL.moments_ref(target)
        assert np.array_equal(state, want)
        worst_m = max(worst_m, float(np.abs(got[:, 0] - want[:, 0]).max()))
        worst_s = max(worst_s, float(np.abs(np.sqrt(got[:, 1]) / np.sqrt(want[:, 1]) - 1).max()))
    print(f"{shape}: byte mean off by at most {worst_m:.4f}, standard deviation by at most {100 * worst_s:.3f} %")
    assert worst_m <= 0.25 and worst_s <= 0.02


def test_setting_errors():
    for bad in (dict(to="first"), dict(to=None), dict(to=3), dict(to=True), dict(strength=-0.1), dict(strength=1.5), dict(strength="1"),
                dict(strength=True), dict(rate=0), dict(rate=0.0), dict(rate=1.01), dict(rate=None), dict(strength=float("nan")),
                dict(rate=float("nan"))):
        with pytest.raises(ValueError):
            CL.check_settings(**bad)
    assert CL.check_settings() == dict(mode="source", strength=1.0, rate=0.1)
    assert CL.check_settings("ema", 0, 1) == dict(mode="ema", strength=0.0, rate=1.0)
    assert CL.check_settings(np.zeros((4, 4, 3), np.uint8), 0.5, 0.3) == dict(mode="image", strength=0.5, rate=0.3)


# ----------------------------------------------------------------------------- the launchers (dry-run)
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    import os

    from live2diff_amd import _lib, ops
    assert (_lib.OP_FRAME_MOMENTS, _lib.OP_COLOR_LOCK, _lib.ABI_VERSION) == (44, 45, 6)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_MOMENTS = 44," in hdr and "L2D_OP_COLOR_LOCK = 45," in hdr
    assert all(f"#define L2D_COLOR_LOCK_{n} {v}" in hdr for n, v in (
        ("INIT", ops.COLOR_LOCK_INIT), ("SOURCE", ops.COLOR_LOCK_SOURCE), ("FREEZE", ops.COLOR_LOCK_FREEZE),
        ("BLOCK_PIXELS", ops.COLOR_LOCK_BLOCK_PIXELS), ("MAX_PIXELS", ops.COLOR_LOCK_MAX_PIXELS)))
    assert ops.COLOR_LOCK_BLOCK_PIXELS * 255 * 255 < 1 << 32 and ops.COLOR_LOCK_BLOCK_PIXELS <= 65536
    assert [ops.color_lock_blocks(*s) for s in ((8, 8), (64, 64), (65, 64), (512, 512), (576, 1024))] == [1, 1, 2, 64, 144]
    H, W = 24, 40

    def frame(H=H, W=W, dtype=torch.float16):
        return torch.zeros(3, H, W, dtype=dtype)

    def parts(n=2, H=H, W=W):
        return torch.zeros(n, ops.color_lock_blocks(H, W), 6, dtype=torch.int32)

    def mk(H=H, W=W, **kw):
        args = dict(styled=frame(H, W), out=frame(H, W), partials=parts(2, H, W), state_in=torch.zeros(3, 2, dtype=torch.float64),
                    state_out=torch.zeros(3, 2, dtype=torch.float64), coef=torch.zeros(3, 3), H=H, W=W, strength=1.0, rate=0.1)
        args.update(kw)
        return ops.color_lock(args.pop("styled"), args.pop("out"), args.pop("partials"), args.pop("state_in"), args.pop("state_out"),
                              args.pop("coef"), **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    ops.run(ops.frame_moments(frame(), None, parts(1), H=H, W=W))
    ops.run(ops.frame_moments(frame(), frame(), parts(), H=H, W=W))
    ops.run(mk())
    ops.run(mk(source=True))
    ops.run(mk(freeze=True, strength=0.0, rate=1.0))
    ops.run(mk(init=True, H=2048, W=2048))
    # the builders: dtype, shape, record sizes
    for call in (lambda: ops.frame_moments(frame(dtype=torch.float32), None, parts(), H=H, W=W),
                 lambda: ops.frame_moments(frame(), frame(H, W + 8), parts(), H=H, W=W),
                 lambda: ops.frame_moments(frame(H + 1, W), None, parts(), H=H, W=W),
                 lambda: ops.frame_moments(frame(), frame(), parts(1), H=H, W=W),
                 lambda: ops.frame_moments(frame(), None, parts().float(), H=H, W=W),
                 lambda: mk(styled=frame(dtype=torch.bfloat16)), lambda: mk(out=frame(H, 2 * W)), lambda: mk(out=torch.zeros(3, H, W)),
                 lambda: mk(state_in=torch.zeros(3, 2)), lambda: mk(state_out=torch.zeros(6, 2, dtype=torch.float64)),
                 lambda: mk(coef=torch.zeros(3, 3, dtype=torch.float64)), lambda: mk(partials=parts(1), source=True)):
        with pytest.raises(ValueError):
            call()
    # the launchers
    bad("multiple of 8", ops.frame_moments(frame(24, 36), None, parts(), H=24, W=36))
    bad("multiple of 8", mk(H=24, W=36))
    bad("multiple of 16", mk(H=3, W=8))
    bad("above 4194304 pixels", mk(H=2049, W=2048))
    state = torch.zeros(2, 3, 2, dtype=torch.float64)
    bad("state_in and state_out overlap", mk(state_in=state[0], state_out=state[0]))
    bad("state_in and state_out overlap", mk(state_in=state.view(-1)[:6], state_out=state.view(-1)[3:9]))
    ops.run(mk(state_in=state[0], state_out=state[1]))
    x = frame()
    bad("overlaps the input frame", mk(styled=x, out=x))
    bad("exclude one another", mk(source=True, freeze=True))
    for kw in (dict(rate=0.0), dict(rate=1.5), dict(rate=float("nan")), dict(strength=-0.5), dict(strength=2.0), dict(strength=float("inf"))):
        bad("rate = .* strength = ", mk(**kw))
    op, keep = mk()
    op.i[2] = 8
    bad("unknown flag bits", (op, keep))
    op, keep = mk()
    op.i[3] += 1
    bad("partial blocks", (op, keep))
    op, keep = mk()
    op.p[4] = None
    bad("pointer 4 is null", (op, keep))
    op, keep = mk()
    op.p[0] = op.p[0] + 2
    bad("pointer 0 is not aligned", (op, keep))
    op, keep = ops.frame_moments(frame(), frame(), parts(), H=H, W=W)
    op.i[2] = 1
    bad("second tensor", (op, keep))
    op, keep = ops.frame_moments(frame(), None, parts(), H=H, W=W)
    op.i[2] = 3
    bad("need 1 or 2", (op, keep))


# ----------------------------------------------------------------------------- the wrapper on the mock components
def pre(frame):
    """the mock image processor's frame, as the delay line keeps it"""
    return (2.0 * frame - 1.0).to(torch.float16)


def frames_of(k, seed):
    import pipeline_mocks as M
    return list(M.frames(k, seed=seed))


@pytest.mark.parametrize("output_type", ["u8", "pil", "jpeg", "pt", "np"])
def test_wrapper_serves_every_output_type(monkeypatch, output_type):
    import pipeline_mocks as M
    from live2diff_amd.jpeg import encode_ref
    n_steps = 2
    warm, frames = M.frames(8, seed=7), frames_of(4, seed=8)
    torch.manual_seed(123)
    w = build(monkeypatch, n_steps, output_type=output_type)
    assert w.color_lock is None
    w.set_color_lock("source", strength=0.75)
    assert w.color_lock == dict(to="source", strength=0.75, rate=0.1) and w.stream.matte_tap is w._matte_line is not None
    w.prepare(warm, "a prompt")
    for t, f in enumerate(frames):
        got = w(f)
        source = pre(frames[t - 1] if t else warm[-1])
        locked, _ = CL.lock_ref(w.stream.prev_image_result, None, mode="source", strength=0.75, source=source)
        assert not np.array_equal(locked, w.stream.prev_image_result.to(torch.float16).numpy())          # (the lock does something)
        lt = torch.from_numpy(locked)
        u8 = egress_ref(lt)[0].numpy()
        if output_type == "u8":
            assert got.dtype == np.uint8 and np.array_equal(got, u8)
        elif output_type == "pil":
            assert got.size == (M.W, M.H) and np.array_equal(np.array(got), u8)
        elif output_type == "jpeg":
            assert got == encode_ref(u8, w.jpeg_quality)
        elif output_type == "pt":
            assert torch.equal(got, (lt / 2 + 0.5).clamp(0, 1)[0])
        else:
            assert np.array_equal(got, (lt / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().numpy()[0])


def test_wrapper_latent_raises(monkeypatch):
    w = build(monkeypatch, 2, output_type="latent")
    with pytest.raises(ValueError, match="'pil'.*'u8'.*'jpeg'"):
        w.set_color_lock("ema")
    assert w.color_lock is None and w._matte_line is None
    w.output_type = "u8"
    w.set_color_lock("ema")
    w.output_type = "latent"                                         # changed behind the lock's back: the frame says so
    import pipeline_mocks as M
    w.prepare(M.frames(8, seed=7), "a prompt")
    with pytest.raises(ValueError, match="clear_color_lock"):
        w(colour(1))
    for args in (("first",), ("ema", 1.5), ("ema", 1.0, 0.0), (None,)):
        with pytest.raises(ValueError):
            w.set_color_lock(*args)


def test_wrapper_lock_runs_before_the_matte(monkeypatch):
    import pipeline_mocks as M
    from live2diff_amd.matte import composite_ref
    warm, frames = M.frames(8, seed=7), frames_of(5, seed=9)
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_matte(0.3, 0.7, feather=2)
    w.set_color_lock("source")
    w.prepare(warm, "a prompt")
    for t, f in enumerate(frames[:3]):
        got = w(f)
        slot = w._matte_line.last
        assert torch.equal(slot.source, pre(frames[t - 1] if t else warm[-1]).float())          # one line, one take per output
        locked, _ = CL.lock_ref(w.stream.prev_image_result, None, mode="source", source=slot.source)
        want = composite_ref(torch.from_numpy(locked), slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0]
        assert np.array_equal(got, want)
        plain = composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0]
        assert not np.array_equal(got, plain)
    assert w._matte_line.tapped == w._matte_line.taken == 3
    # m == 0 everywhere: the real picture, untouched by the lock
    w.set_matte(0, 0, keep="far")
    assert np.array_equal(w(frames[3]), egress_ref(pre(frames[2]))[0].numpy())
    w.set_color_lock("ema")                                          # (the matte keeps the line)
    assert np.array_equal(w(frames[4]), egress_ref(pre(frames[3]))[0].numpy())


def test_wrapper_dropped_frame_reuses_the_locked_frame(monkeypatch):
    import pipeline_mocks as M
    frames = frames_of(7, seed=10)
    for to in ("ema", "source"):
        torch.manual_seed(123)
        w = build(monkeypatch, 2, drop={2, 3, 5})
        w.set_color_lock(to, rate=0.5)
        w.prepare(M.frames(8, seed=7), "a prompt")
        got, states, locked = [], [], []
        for f in frames:
            got.append(w(f))
            states.append(None if w._lock_state is None else w._lock_state.copy())
            locked.append(w._lock_last)
        for t in (2, 3, 5):
            assert np.array_equal(got[t], got[t - 1]) and locked[t] is locked[t - 1], (to, t)
            assert np.array_equal(bits(states[t]), bits(states[t - 1])), (to, t)
        for t in (1, 4, 6):
            assert not np.array_equal(got[t], got[t - 1]) and not np.array_equal(states[t], states[t - 1]), (to, t)
        if to == "source":
            assert w._matte_line.tapped == w._matte_line.taken == 4
        else:
            assert w._matte_line is None


def test_wrapper_prepare_resets_ema(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), frames_of(4, seed=11)
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_color_lock("ema", rate=0.25)
    w.prepare(warm, "a prompt")
    state = None
    for t, f in enumerate(frames[:3]):
        got = w(f)
        locked, state = CL.lock_ref(w.stream.prev_image_result, state, mode="ema", rate=0.25, init=t == 0)
        assert np.array_equal(got, egress_ref(torch.from_numpy(locked))[0].numpy())
        assert np.array_equal(bits(w._lock_state), bits(state))
    assert not np.array_equal(state, CL.moments_ref(w.stream.prev_image_result))
    w.prepare(warm, "a prompt")
    assert w._lock_state is None and w.color_lock["to"] == "ema"
    w(frames[3])
    assert np.array_equal(bits(w._lock_state), bits(CL.moments_ref(w.stream.prev_image_result)))   # the first frame copies
    # so does the first frame after set_color_lock
    w(frames[0])
    w.set_color_lock("ema", rate=0.25)
    w(frames[1])
    assert np.array_equal(bits(w._lock_state), bits(CL.moments_ref(w.stream.prev_image_result)))


def test_wrapper_reference_image_is_frozen(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), frames_of(3, seed=12)
    ref_image = M.frames(1, seed=99)[0]
    want = CL.moments_ref(pre(ref_image))
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_color_lock(ref_image, strength=0.5)
    assert w.color_lock == dict(to="image", strength=0.5, rate=0.1) and w._matte_line is None
    w.prepare(warm, "a prompt")
    for f in frames:
        got = w(f)
        locked, _ = CL.lock_ref(w.stream.prev_image_result, want, mode="image", strength=0.5)
        assert np.array_equal(got, egress_ref(torch.from_numpy(locked))[0].numpy())
        assert np.array_equal(bits(w._lock_state), bits(want))
    w.prepare(warm, "a prompt")
    assert np.array_equal(bits(w._lock_state), bits(want))


def test_wrapper_line_is_shared_and_released(monkeypatch):
    w = build(monkeypatch, 2)
    tap = lambda: w.stream.matte_tap
    # the matte first
    w.set_matte(0.3, 0.7)
    line = w._matte_line
    w.set_color_lock("source")
    assert w._matte_line is line is tap()
    w.clear_matte()
    assert w.matte is None and w._matte_line is line is tap()             # the lock keeps it
    w.clear_color_lock()
    assert w.color_lock is None and w._matte_line is None and tap() is None
    # the lock first
    w.set_color_lock("source")
    line = w._matte_line
    assert line is not None and line is tap()
    w.set_matte(0.3, 0.7)
    assert w._matte_line is line
    w.clear_color_lock()
    assert w._matte_line is line is tap()                                 # the matte keeps it
    w.clear_matte()
    assert w._matte_line is None and tap() is None
    # "ema" and a reference image need no line, and changing the mode lets go of it
    w.set_color_lock("ema")
    assert w._matte_line is None and tap() is None
    w.set_color_lock("source")
    assert w._matte_line is not None
    w.set_color_lock(torch.full((3, 64, 64), 0.5))
    assert w.color_lock["to"] == "image" and w._matte_line is None and tap() is None
    w.set_matte(0.3, 0.7)
    w.set_color_lock("source")
    w.set_color_lock("ema")
    assert w._matte_line is not None and w._matte_line is tap()           # (the matte's)
    w.clear_color_lock()
    w.clear_matte()
    assert w._matte_line is None


def test_wrapper_without_a_lock_is_the_twin(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), frames_of(5, seed=13)

    def run(lock):
        torch.manual_seed(123)
        w = build(monkeypatch, 2)
        if lock:
            w.set_color_lock("source")
        w.prepare(warm, "a prompt")
        out = [w(f) for f in frames[:3]]
        if lock:
            w.clear_color_lock()
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return w, out + [w(f) for f in frames[3:]]

    (w, got), (twin, plain) = run(True), run(False)
    assert not any(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3]))
    assert all(np.array_equal(a, b) for a, b in zip(got[3:], plain[3:]))
    assert w._lock is None and w._lock_last is None and w._matte_line is None and w.stream.matte_tap is None
    # mid-stream: the line starts with the next frame, and the first output uses the oldest source it has
    w.set_color_lock("source")
    w(frames[0])
    locked, _ = CL.lock_ref(w.stream.prev_image_result, None, mode="source", source=pre(frames[0]))
    assert w._lock_last is not None and np.array_equal(w._lock_last.numpy(), locked)
