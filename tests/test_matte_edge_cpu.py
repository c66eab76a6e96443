"""CPU tests (-m "not gpu") of the edge-aware matte (live2diff_amd/matte.py `edge_ref`): the identities of
the arithmetic (a constant matte comes back exactly, a flat guide gives A == 0 and the double box mean), edge snapping on a planted
case, `edge=None` leaving the three oracles bit for bit what they were, `check_edge`, the launcher's argument checks (dry-run), and
`set_matte_edge` / `clear_matte_edge` on the wrapper built from the mock components of tests/test_matte_cpu.py (the host route)."""
import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd.steady import window_sum

PLANTED_H, PLANTED_W = 48, 96


def frame_of_bytes(b) -> np.ndarray:
    """an fp16 [3,H,W] frame whose egress bytes are the uint8 [H,W] (grey) or [3,H,W] array `b`: x = 2 b / 255 - 1 lies within
    1e-3 (an fp16 step at 1 is 4.9e-4) of a value whose byte is b, and bytes are 7.8e-3 apart in x (checked by the callers)"""
    b = np.asarray(b)
    b = np.repeat(b[None], 3, 0) if b.ndim == 2 else b
    return (b.astype(np.float64) * 2.0 / 255.0 - 1.0).astype(np.float16)


def planted(H=PLANTED_H, W=PLANTED_W, seed=0):
    """(m0 float32 [H,W], source fp16 [3,H,W]): the guide is 60 left of column 40 and 190 from it on, with noise of +-6; the
    matte a smoothstep ramp from column 38 to 54 -- its middle sits 6 columns beside the frame's edge.  (Smaller images keep
    the columns that fit.)"""
    rng = np.random.default_rng(seed)
    g = np.where(np.arange(W) < 40, 60, 190)[None, :] + rng.integers(-6, 7, (H, W))
    src = frame_of_bytes(g.astype(np.uint8))
    assert np.array_equal(MT.guide_ref(src), g)
    t = np.clip((np.arange(W) - 38) / 16.0, 0.0, 1.0)
    m0 = np.ascontiguousarray(np.broadcast_to((t * t * (3 - 2 * t)).astype(np.float32), (H, W)))
    return m0, src


def random_case(H, W, seed):
    """uniform random bytes in all three channels and a uniform random matte"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    src = frame_of_bytes(b)
    from live2diff_amd.steady import source_bytes
    assert np.array_equal(source_bytes(src), b)
    return (rng.integers(0, 256, (H, W)) / 255.0).astype(np.float32), src


# ----------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("r,eps", [(1, 1.0), (4, 10.0), (8, 1.0)])
def test_constant_matte_comes_back_exactly(r, eps):
    _, src = random_case(24, 40, seed=r)
    for c in (0, 1, 77, 128, 254, 255):
        got = MT.edge_ref(np.full((24, 40), c / 255.0, np.float32), src, r, eps)
        assert got.dtype == np.float32 and np.all(got == np.float32(c / 255.0)), (c, np.unique(got))
    assert np.all(MT.edge_ref(np.ones((24, 40), np.float32), src, r, eps) == 1.0)
    assert np.all(MT.edge_ref(np.zeros((24, 40), np.float32), src, r, eps) == 0.0)
    # ... so a fully near or fully far matte still yields the bytes of `egress_ref`
    from live2diff_amd.frame_io import egress_ref
    styled = torch.from_numpy(random_case(24, 40, seed=9)[1])[None]
    source = torch.from_numpy(src)[None]
    depth = torch.zeros(1, 24, 40, dtype=torch.float16)
    edge = dict(radius=r, eps=eps)
    assert np.array_equal(MT.composite_ref(styled, source, depth, 0, 0, feather=2, edge=edge), egress_ref(styled).numpy())
    assert np.array_equal(MT.composite_ref(styled, source, depth, 0, 0, feather=2, keep="far", edge=edge), egress_ref(source).numpy())


@pytest.mark.parametrize("r,eps", [(1, 1.0), (4, 10.0), (8, 1.0)])
def test_flat_guide_gives_the_double_box_mean(r, eps):
    """var == cov == 0 in every window: A == 0, B = rint(4096 mean(P)), and m' is the box mean of that over 4096 * 255.  The
    bound: half a step of B, 0.5 / 4096 / 255 = 4.8e-7, plus one fp32 rounding of a value in [0, 1], 6e-8: below 6e-7."""
    H, W = 24, 40
    m0, _ = random_case(H, W, seed=3)
    P = np.rint(m0 * np.float32(255.0)).astype(np.int64)
    n = (2 * r + 1) ** 2
    def box(v):
        p = np.pad(v, r, mode="edge")
        return sum(p[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)) / n

    mean2 = box(box(P.astype(np.float64) / 255.0))
    for level in (0, 93, 255):
        src = frame_of_bytes(np.full((H, W), level, np.uint8))
        A, B = MT.edge_coefficients(P, MT.guide_ref(src), r, eps)
        assert np.all(A == 0)
        assert np.array_equal(B, np.rint(window_sum(P, r).astype(np.float64) / n * 4096).astype(np.int64))
        err = float(np.abs(MT.edge_ref(m0, src, r, eps).astype(np.float64) - mean2).max())
        print(f"r {r} eps {eps} level {level}: max |m' - box(box(P)) / 255| {err:.2e}")
        assert err <= 6e-7


def test_coefficients_fit_int32_on_the_worst_case():
    """random bytes with eps = 1 (the largest |a|): the oracle asserts the int32 range itself; |a| <= 127.5 / (2 eps)"""
    for r in (1, 8):
        m0, src = random_case(40, 72, seed=r)
        P = np.rint(m0 * np.float32(255.0)).astype(np.int64)
        A, B = MT.edge_coefficients(P, MT.guide_ref(src), r, 1.0)
        print(f"r {r}: max |A| {int(np.abs(A).max())}, max |B| {int(np.abs(B).max())}")
        assert int(np.abs(A).max()) <= 261120 and int(np.abs(B).max()) <= 67629056
        m = MT.edge_ref(m0, src, r, 1.0)
        assert m.dtype == np.float32 and m.min() >= 0.0 and m.max() <= 1.0


@pytest.mark.parametrize("r,eps", [(4, 10.0), (8, 10.0)])
def test_edge_snaps_to_the_frame(r, eps):
    m0, src = planted()
    m = MT.edge_ref(m0, src, r, eps)
    row = PLANTED_H // 2
    step, before = np.abs(np.diff(m[row])), np.abs(np.diff(m0[row]))
    print(f"r {r} eps {eps}: largest step {step.max():.3f} between columns {int(np.argmax(step))} and {int(np.argmax(step)) + 1}; "
          f"the input's there {before[39]:.3f}, its largest {before.max():.3f}")
    assert int(np.argmax(step)) == 39                      # between columns 39 and 40: where the frame's own edge is
    assert step[39] > 3 * before[39]


# ----------------------------------------------------------------------------- edge=None: the oracles as they were
def _matte_before(depth, lo, hi, feather=0, keep="near"):
    """`matte_ref` as it stood before the `edge` keyword, written out"""
    lo32, inv32, hard = MT.matte_params(lo, hi)
    d = MT._np16(depth).astype(np.float32)
    if d.ndim == 2:
        d = d[None]
    one, zero = np.float32(1.0), np.float32(0.0)
    if hard:
        t = np.where(d >= lo32, one, zero).astype(np.float32)
    else:
        t = np.minimum(np.maximum((d - lo32) * inv32, zero), one)
    m = (t * t) * (np.float32(3.0) - np.float32(2.0) * t)
    if keep == "far":
        m = one - m
    if feather:
        m = MT._box_pass(MT._box_pass(m, feather, 2), feather, 1)
    return m


def _composite_before(styled, source, depth, lo, hi, feather=0, keep="near", show=False):
    m = _matte_before(depth, lo, hi, feather, keep)[..., None]
    scale = np.float32(255.0)
    if show:
        return np.rint(np.repeat(m, 3, axis=-1) * scale).astype(np.uint8)
    vs, vc = MT._unit(styled), MT._unit(source)
    o = vc + m * (vs - vc)
    return np.rint(o * scale).astype(np.uint8)


def _composite_up_before(S, C, depth, lo, hi, feather=0, keep="near", show=False):
    M = MT.matte_up_ref(_matte_before(depth, lo, hi, feather, keep), S.shape[1], S.shape[2])[..., None]
    if show:
        return np.rint(np.repeat(M, 3, axis=-1) * np.float32(255.0)).astype(np.uint8)
    S, C = S.astype(np.float32), C.astype(np.float32)
    return np.rint(C + M * (S - C)).astype(np.uint8)


def test_without_edge_the_oracles_are_unchanged():
    from test_matte_cpu import data
    B, H, W = 2, 40, 72
    styled, source, depth = data(B, H, W, seed=5)
    rng = np.random.default_rng(1)
    S, C = (rng.integers(0, 256, (B, 60, 100, 3), dtype=np.uint8) for _ in range(2))
    for lo, hi in ((0.3, 0.7), (0.5, 0.5)):
        for r in (0, 3):
            for keep in ("near", "far"):
                want = _matte_before(depth, lo, hi, r, keep)
                for got in (MT.matte_ref(depth, lo, hi, r, keep), MT.matte_ref(depth, lo, hi, r, keep, edge=None, source=source)):
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
                for show in (False, True):
                    assert np.array_equal(MT.composite_ref(styled, source, depth, lo, hi, r, keep, show),
                                          _composite_before(styled, source, depth, lo, hi, r, keep, show))
                    assert np.array_equal(MT.composite_ref(styled, source, depth, lo, hi, r, keep, show, edge=None),
                                          _composite_before(styled, source, depth, lo, hi, r, keep, show))
                    assert np.array_equal(MT.composite_up_ref(S, C, depth, lo, hi, r, keep, show),
                                          _composite_up_before(S, C, depth, lo, hi, r, keep, show))
                    assert np.array_equal(MT.composite_up_ref(S, C, depth, lo, hi, r, keep, show, edge=None, source=source),
                                          _composite_up_before(S, C, depth, lo, hi, r, keep, show))
    # with the setting, the refinement sits between the ramp and the feather
    edge = dict(radius=2, eps=4.0)
    m0 = MT.matte_ref(depth, 0.3, 0.7, 0, "far")
    want = np.stack([MT.edge_ref(m0[b], source[b], 2, 4.0) for b in range(B)])
    assert not np.array_equal(want, m0)
    assert np.array_equal(MT.matte_ref(depth, 0.3, 0.7, 0, "far", edge=edge, source=source), want)
    assert np.array_equal(MT.matte_ref(depth, 0.3, 0.7, 3, "far", edge=edge, source=source), MT._box_pass(MT._box_pass(want, 3, 2), 3, 1))
    with pytest.raises(ValueError, match="needs the source frames"):
        MT.matte_ref(depth, 0.3, 0.7, edge=edge)
    with pytest.raises(ValueError, match="needs the source frames"):
        MT.composite_up_ref(S, C, depth, 0.3, 0.7, edge=edge)


def test_check_edge():
    assert MT.check_edge() == dict(radius=4, eps=10.0)
    assert MT.check_edge(np.int64(8), 1) == dict(radius=8, eps=1.0) and MT.MAX_EDGE_RADIUS == 8
    for bad in (dict(radius=0), dict(radius=9), dict(radius=-1), dict(radius=2.0), dict(radius=True), dict(radius="4"),
                dict(eps=0.99), dict(eps=0), dict(eps=-3.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps="10"), dict(eps=True)):
        with pytest.raises(ValueError, match="matte edge"):
            MT.check_edge(**bad)
    with pytest.raises(ValueError, match="matte edge"):
        MT.edge_ref(np.zeros((8, 16), np.float32), np.zeros((3, 8, 16), np.float16), 0, 10.0)
    with pytest.raises(ValueError, match="the matte is"):
        MT.edge_ref(np.zeros((8, 16), np.float32), np.zeros((3, 8, 8), np.float16), 1, 10.0)
    assert MT.edge_E(8, 1.0) == 289.0 * 289.0 and MT.edge_E(1, 2.5) == 81.0 * 6.25


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
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert _lib.OP_FRAME_MATTE_EDGE == 49 and "L2D_OP_FRAME_MATTE_EDGE = 49," in hdr
    assert f"#define L2D_MATTE_PLANE {ops.MATTE_PLANE}" in hdr and f"#define L2D_MATTE_EDGE_MAX_R {ops.MATTE_EDGE_MAX_R}" in hdr
    assert ops.MATTE_PLANE & (ops.MATTE_HARD | ops.MATTE_FAR | ops.MATTE_SHOW) == 0
    H, W = 24, 40

    def mk(H=H, W=W, **kw):
        args = dict(H=H, W=W, r=4, E=MT.edge_E(4, 10.0), lo32=-0.4, inv32=1.25, hard=False)
        args.update(kw)
        return ops.frame_matte_edge(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float16),
                                    torch.zeros(H, W, dtype=torch.float32), **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, keep = mk(far=True)
    assert op.kind == 49 and [op.i[j] for j in range(4)] == [H, W, 4, ops.MATTE_FAR] and op.p[3] is None
    assert np.int64(op.l[0]).view(np.float64) == 81.0 * 81.0 * 100.0
    ops.run((op, keep))
    ops.run(mk(r=8, E=MT.edge_E(8, 1.0), lo32=0.0, inv32=0.0, hard=True))
    ops.run(mk(H=8, W=16, r=8, E=MT.edge_E(8, 1.0)))                      # an image smaller than the window
    for r in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="use an integer from 1 to 8"):
            mk(r=r)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.frame_matte_edge(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W), torch.zeros(H, W), H=H, W=W, r=1, E=81.0,
                             lo32=0.0, inv32=1.0, hard=False)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.frame_matte_edge(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float16),
                             torch.zeros(H, W, dtype=torch.float16), H=H, W=W, r=1, E=81.0, lo32=0.0, inv32=1.0, hard=False)
    bad("multiple of 8", mk(W=36))
    bad("at least n n", mk(E=MT.edge_E(4, 0.5)))
    bad("at least n n", mk(E=float("nan")))
    bad("at least n n", mk(E=float("inf")))
    bad("hard flag", mk(inv32=0.0))
    bad(r"lo = .* must lie in", mk(lo32=1.5))
    for field, value, match in ((2, 0, "radius 0, need 1..8"), (2, 9, "radius 9"), (3, 4, "unknown flag bits"), (3, 16, "unknown flag bits"),
                                (0, 0, "non-positive size")):
        op, keep = mk()
        op.i[field] = value
        bad(match, (op, keep))
    for k in range(3):
        op, keep = mk()
        op.p[k] = op.p[k] + 4
        bad(f"pointer {k} is not 16-byte aligned", (op, keep))
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))

    # the plane flag of ops 43 and 47
    B = 2
    s, c = (torch.zeros(B, 3, H, W, dtype=torch.float16) for _ in range(2))
    o, plane = torch.zeros(B, H, W, 3, dtype=torch.uint8), torch.zeros(B, H, W)
    for r in (0, 3):
        op, keep = ops.frame_matte(s, c, None, o, B=B, H=H, W=W, r=r, show=bool(r), plane=plane)
        assert op.i[4] == ops.MATTE_PLANE | (ops.MATTE_SHOW if r else 0) and op.p[2] == plane.data_ptr() and op.f[0] == op.f[1] == 0.0
        ops.run((op, keep))
    op, keep = ops.frame_matte(s, c, None, o, B=B, H=H, W=W, plane=plane)
    op.p[2] = op.p[2] + 8
    bad("pointer 2 is not 16-byte aligned", (op, keep))
    with pytest.raises(ValueError, match="plane= goes with depth=None"):
        ops.frame_matte(s, c, torch.zeros(B, H, W, dtype=torch.float16), o, B=B, H=H, W=W, plane=plane)
    with pytest.raises(ValueError, match="plane= goes with depth=None"):
        ops.frame_matte(s, c, None, o, B=B, H=H, W=W, far=True, plane=plane)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.frame_matte(s, c, None, o, B=B, H=H, W=W, plane=plane.half())
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.frame_matte(s, c, None, o, B=B, H=H, W=W, plane=plane[:1])
    Ho, Wo = 36, 60
    S8, C8, O8 = (torch.zeros(B, Ho, Wo, 3, dtype=torch.uint8) for _ in range(3))
    tx, ty = (torch.from_numpy(MT.table_words(i, n)) for i, n in ((W, Wo), (H, Ho)))
    op, keep = ops.frame_matte_up(S8, C8, None, O8, tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo, r=2, plane=plane)
    assert op.i[6] == ops.MATTE_PLANE and op.p[2] == plane.data_ptr()
    ops.run((op, keep))
    op.p[2] = op.p[2] + 2
    bad("4-byte: a float plane", (op, keep))
    with pytest.raises(ValueError, match="plane= goes with depth=None"):
        ops.frame_matte_up(S8, C8, None, O8, tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo, hard=True, plane=plane)


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
def test_wrapper_host_route(monkeypatch):
    import pipeline_mocks as M
    from test_matte_cpu import build
    n_steps = 2
    warm, frames = M.frames(8, seed=7), M.frames(6, seed=8)
    MATTE = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)
    EDGE = dict(radius=3, eps=4.0)

    def run(edge, at_construction=False):
        torch.manual_seed(123)
        w = build(monkeypatch, n_steps)
        w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
        if edge:
            w.set_matte_edge(**EDGE)
        w.prepare(warm, "a prompt")
        return w

    def call(w, f):
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return w(f)

    def want(w, edge):
        slot = w._matte_line.last
        return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **w.matte, edge=edge)[0]

    w, twin = run(True), run(False)
    assert w.matte_edge == EDGE and twin.matte_edge is None and w.matte == MATTE and sorted(w.matte) == ["feather", "hi", "keep", "lo", "show"]
    for t in range(3):
        got, plain = call(w, frames[t]), call(twin, frames[t])
        assert got.dtype == np.uint8 and np.array_equal(got, want(w, EDGE)), t
        assert np.array_equal(plain, want(twin, None)) and not np.array_equal(got, plain), t
    # `show`, and a changed setting: the next output
    w.set_matte(0.3, 0.7, keep="far", feather=0, show=True)
    w.set_matte_edge(8, 1)
    assert w.matte_edge == dict(radius=8, eps=1.0)
    shown = call(w, frames[3])
    call(twin, frames[3])
    assert np.array_equal(shown, want(w, dict(radius=8, eps=1.0))) and np.array_equal(shown[..., 0], shown[..., 2])
    slot = w._matte_line.last
    assert np.array_equal(shown[..., 0], np.rint(MT.matte_ref(slot.depth[None], 0.3, 0.7, 0, "far", edge=w.matte_edge,
                                                              source=slot.source[None])[0] * np.float32(255)).astype(np.uint8))
    # clear_matte_edge restores the old bytes; the matte's own dict never changed its keys
    w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
    w.clear_matte_edge()
    assert w.matte_edge is None and w.matte == MATTE
    assert np.array_equal(call(w, frames[4]), call(twin, frames[4]))
    # the setting acts only while a matte is set
    w.set_matte_edge(**EDGE)
    w.clear_matte()
    twin.clear_matte()
    assert w.matte_edge == EDGE and w.stream.matte_tap is None
    assert np.array_equal(call(w, frames[5]), call(twin, frames[5]))
    for bad in (dict(radius=0), dict(radius=9), dict(eps=0.5), dict(radius=2.5)):
        with pytest.raises(ValueError, match="matte edge"):
            w.set_matte_edge(**bad)
    assert w.matte_edge == EDGE


def test_wrapper_keyword_and_repeated_frame(monkeypatch):
    """`matte_edge=` at construction is `set_matte_edge`; a frame the near-duplicate filter drops repeats the refined bytes"""
    import pipeline_mocks as M

    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    from test_matte_cpu import DropFilter, RampDepth
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)

    def make(**more):
        pipe = M.MockPipe()
        pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), RampDepth()
        pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
        pipe.similar_filter = DropFilter({1})
        w = Wrapper.from_components(pipe, output_type="u8", dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50,
                                    t_index_list=[10, 20], width=M.W, height=M.H, enable_similar_image_filter=True, **more)
        s = w.stream
        s.scheduler = M.MockScheduler()
        s.timesteps = s.scheduler.timesteps
        s.image_processor = M.MockImageProcessor()
        s.unet_warmup = M.MockWarmupUNet()
        return w

    for bad in (4, "4,10", [4, 10.0]):
        with pytest.raises(ValueError, match="matte_edge="):
            make(matte_edge=bad)
    with pytest.raises(ValueError, match="matte edge"):
        make(matte_edge=dict(radius=0))
    torch.manual_seed(123)
    w = make(matte_edge=dict(radius=2))
    assert w.matte_edge == dict(radius=2, eps=10.0) and w.matte is None
    w.set_matte(0.2, 0.8, feather=1)
    w.prepare(M.frames(8, seed=7), "a prompt")
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    frames = M.frames(3, seed=9)
    out = [w(f) for f in frames]
    slot = w._matte_line.last
    assert np.array_equal(out[1], out[0]) and w._matte_line.tapped == 2
    assert np.array_equal(out[2], MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **w.matte,
                                                   edge=w.matte_edge)[0])
