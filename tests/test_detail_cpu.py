"""CPU tests (-m "not gpu") of the detail mode (live2diff_amd/detail.py): the identities of the arithmetic,
the int32 bound of the gains, the planted case that shows what the mode is for, the settings, the launchers' argument checks in
dry-run, and the wrapper on the mock components (the host route, where the mode does not act)."""
import types

import numpy as np
import pytest
import torch

from live2diff_amd import detail as D
from live2diff_amd import matte as MT
from live2diff_amd.frame_io import ingest_ref
from live2diff_amd.resize import camera_box, resize_ref


def frame_of_bytes(b) -> np.ndarray:
    """fp16 [3,H,W] whose egress bytes are the uint8 [H,W,3] (or planar [3,H,W]) array `b`"""
    b = np.asarray(b)
    b = b.transpose(2, 0, 1) if b.shape[-1] == 3 and b.shape[0] != 3 else b
    x = (b.astype(np.float64) / 255.0 * 2.0 - 1.0).astype(np.float16)
    assert np.array_equal(D.frame_bytes(x), b.transpose(1, 2, 0))
    return x


def random_case(H, W, Ho, Wo, seed):
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    source = frame_of_bytes(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    S, C, L = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(3))
    return P, source, S, C, L


def planted(H=48, W=96):
    """the planted case of the issue: a camera frame with fine detail, and a style that follows it with a slope per region (the
    GPU tests crop a wider one)"""
    rng = np.random.default_rng(0)
    Ho, Wo = 2 * H, 2 * W
    yy, xx = np.mgrid[0:Ho, 0:Wo]
    base = 90 + 50 * np.sin(xx / 23.0) + 30 * np.cos(yy / 17.0) + np.where(xx > 101, 60, 0)
    fine = 25 * ((xx + yy) % 2) * (yy > 40) + 30 * (((xx % 7) == 3) & ((yy % 5) == 2))
    lum = np.clip(base + fine + rng.integers(-2, 3, (Ho, Wo)), 0, 255)
    cam = np.stack([lum, np.clip(lum * 0.9 + 10, 0, 255), np.clip(lum * 1.05 - 5, 0, 255)], -1).astype(np.uint8)
    slope = np.where(xx < 60, 0.6, np.where(xx < 130, -0.8, 1.2))
    lc = D.luma(cam).astype(np.float64)
    truth = np.rint(np.stack([np.clip(128 + slope * (lc - 128) + off, 0, 255) for off in (20, -10, 0)], -1)).astype(np.uint8)
    source = ingest_ref(cam[None], H, W, torch.float16)[0]
    styled = ingest_ref(truth[None], H, W, torch.float16)[0]
    assert camera_box(Ho, Wo, H, W) == (0, 0, Ho, Wo)                      # C is `cam` itself
    return dict(H=H, W=W, Ho=Ho, Wo=Wo, cam=cam, truth=truth, source=source, styled=styled)


def err(x, truth) -> int:
    return int(np.abs(x.astype(np.int64) - truth.astype(np.int64)).sum())


# ----------------------------------------------------------------------------- the identities
@pytest.mark.parametrize("show", [False, True])
def test_identities(show):
    H, W, Ho, Wo = 24, 40, 36, 60
    P, source, S, C, L = random_case(H, W, Ho, Wo, 1)
    G = D.gains_ref(P, source, 2, 1.0)
    assert G.dtype == np.int32 and G.shape == (3, H, W) and np.any(G != 0)
    flat = np.full_like(S, 128) if show else S                              # what "nothing injected" looks like
    kw = dict(H=H, W=W, radius=2, show=show)
    out = D.inject_ref(S, C, L, G, strength=1.0, limit=64.0, **kw)
    assert out.dtype == np.uint8 and out.shape == S.shape and not np.array_equal(out, flat)
    assert np.array_equal(D.inject_ref(S, C, C, G, strength=1.0, limit=64.0, **kw), flat)           # C == L
    assert np.array_equal(D.inject_ref(S, C, L, G, strength=0.0, limit=64.0, **kw), flat)           # strength == 0
    assert np.array_equal(D.inject_ref(S, C, L, np.zeros_like(G), strength=4.0, limit=255.0, **kw), flat)      # G == 0
    assert np.array_equal(D.inject_ref(S, C, L, G, strength=4.0, limit=0.0, **kw), flat)            # limit == 0
    for limit in (0.5, 8.0, 17.25, 64.0, 255.0):
        o = D.inject_ref(S, C, L, G, strength=4.0, limit=limit, **kw)
        assert int(np.abs(o.astype(np.int64) - flat.astype(np.int64)).max()) <= int(np.ceil(limit)), limit
    # the fp16 form of the frame gives the gains of its egress bytes
    assert np.array_equal(D.gains_ref(frame_of_bytes(P), source, 2, 1.0), G)
    # and the joined oracle is the parts
    cam = C
    want = D.inject_ref(resize_ref(P, Ho, Wo, "bicubic"), cam, resize_ref(D.frame_bytes(source), Ho, Wo, "bicubic"),
                        D.gains_ref(P, source, 3, 4.0), H, W, 3, 0.5, 32.0, show)
    assert np.array_equal(D.detail_ref(P, source, cam, Ho, Wo, "bicubic", radius=3, eps=4.0, strength=0.5, limit=32.0, show=show), want)


def test_float64_restatement():
    """the injected term against a float64 restatement from the integers: within one byte level (fp32 rounds five times)"""
    H, W, Ho, Wo = 24, 40, 36, 60
    P, source, S, C, L = random_case(H, W, Ho, Wo, 2)
    r, strength, limit = 2, 1.5, 40.0
    G = D.gains_ref(P, source, r, 2.0)
    x0, x1, fx = MT.up_table(W, Wo)
    y0, y1, fy = MT.up_table(H, Ho)
    g = G.astype(np.float64)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)[:, None]
    top = g[:, y0][:, :, x0] * (1 - fx) + g[:, y0][:, :, x1] * fx
    bot = g[:, y1][:, :, x0] * (1 - fx) + g[:, y1][:, :, x1] * fx
    gain = (top * (1 - fy) + bot * fy) / ((2 * r + 1) ** 2 * 4096.0)
    u = np.clip(gain * (D.luma(C) - D.luma(L)) * strength, -limit, limit)
    want = np.clip(S.transpose(2, 0, 1) + u, 0, 255).transpose(1, 2, 0)
    got = D.inject_ref(S, C, L, G, H, W, r, strength, limit).astype(np.float64)
    assert np.abs(got - want).max() <= 0.5 + 1e-3


# ----------------------------------------------------------------------------- the int32 bound
@pytest.mark.parametrize("r", [1, 8])
def test_gains_fit_int32(r):
    H, W = 40, 72
    rng = np.random.default_rng(10 + r)
    n = (2 * r + 1) ** 2
    assert D.MAX_GAIN == 261120 and D.MAX_GAIN * 289 < 1 << 31
    worst = 0
    for seed in range(3):
        P = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if seed == 2:                                                        # the style is the source's sign pattern at full swing
            src = np.where(rng.integers(0, 2, (H, W, 1)) > 0, 128, 127).astype(np.uint8).repeat(3, axis=2)
            P = np.where(src > 127, 255, 0).astype(np.uint8)
        G = D.gains_ref(P, frame_of_bytes(src), r, 1.0)
        worst = max(worst, int(np.abs(G.astype(np.int64)).max()))
        assert G.dtype == np.int32 and worst <= D.MAX_GAIN * n
    assert worst > 4096 * n                                                   # (the case is no trivial one: a mean gain above 1)


# ----------------------------------------------------------------------------- flat inputs
def test_flat_guide_or_flat_channel_adds_nothing():
    H, W, Ho, Wo = 24, 40, 36, 60
    P, source, S, C, L = random_case(H, W, Ho, Wo, 3)
    flat_source = frame_of_bytes(np.full((H, W, 3), 93, np.uint8))
    G = D.gains_ref(P, flat_source, 2, 1.0)
    assert not G.any()
    assert np.array_equal(D.inject_ref(S, C, L, G, H, W, 2, 4.0, 255.0), S)
    P2 = P.copy()
    P2[..., 1] = 200                                                          # one flat styled channel: its gain alone is 0
    G = D.gains_ref(P2, source, 2, 1.0)
    assert not G[1].any() and G[0].any() and G[2].any()
    out = D.inject_ref(S, C, L, G, H, W, 2, 1.0, 64.0)
    assert np.array_equal(out[..., 1], S[..., 1]) and not np.array_equal(out[..., 0], S[..., 0])


# ----------------------------------------------------------------------------- the settings
def test_check_settings():
    assert D.check_settings() == dict(radius=2, eps=2.0, strength=1.0, limit=64.0, show=False)
    assert D.check_settings(8, 1, 4, 255, True) == dict(radius=8, eps=1.0, strength=4.0, limit=255.0, show=True)
    assert D.check_settings(np.int64(1), np.float32(1.5), 0, 0) == dict(radius=1, eps=1.5, strength=0.0, limit=0.0, show=False)
    for bad in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(eps=0.5), dict(eps=float("nan")),
                dict(eps=float("inf")), dict(eps="2"), dict(eps=True), dict(strength=-0.1), dict(strength=4.5), dict(strength=float("nan")),
                dict(strength=None), dict(limit=-1), dict(limit=256), dict(limit=float("inf")), dict(limit="64")):
        with pytest.raises(ValueError, match="detail: "):
            D.check_settings(**bad)
    assert D.SERVED_OUTPUT_TYPES == ("u8", "pil", "jpeg")
    assert D.gain_scale(2, 1.0) == np.float32(1.0 / (25 * 4096.0)) and D.gain_scale(8, 0.0) == 0.0


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
    assert _lib.OP_FRAME_DETAIL_GAIN == 50 and "L2D_OP_FRAME_DETAIL_GAIN = 50," in hdr
    assert _lib.OP_FRAME_DETAIL == 51 and "L2D_OP_FRAME_DETAIL = 51," in hdr
    assert f"#define L2D_DETAIL_U8 {ops.DETAIL_U8}" in hdr and f"#define L2D_DETAIL_SHOW {ops.DETAIL_SHOW}" in hdr
    assert "#define L2D_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6
    H, W, Ho, Wo = 24, 40, 36, 60

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    # op 50
    def gain(H=H, W=W, u8=False, **kw):
        args = dict(H=H, W=W, r=2, E=MT.edge_E(2, 2.0))
        args.update(kw)
        frame = torch.zeros(H, W, 3, dtype=torch.uint8) if u8 else torch.zeros(3, H, W, dtype=torch.float16)
        return ops.frame_detail_gain(frame, torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(3, H, W, dtype=torch.int32), **args)

    op, keep = gain()
    assert op.kind == 50 and [op.i[j] for j in range(4)] == [H, W, 2, 0] and op.p[3] is None
    assert np.int64(op.l[0]).view(np.float64) == 25.0 * 25.0 * 4.0
    ops.run((op, keep))
    op, keep = gain(u8=True, r=8, E=MT.edge_E(8, 1.0))
    assert op.i[3] == ops.DETAIL_U8
    ops.run((op, keep))
    ops.run(gain(H=8, W=16, r=8, E=MT.edge_E(8, 1.0)))                      # an image smaller than the window
    for r in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="use an integer from 1 to 8"):
            gain(r=r)
    z16, z32 = torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(3, H, W, dtype=torch.int32)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.frame_detail_gain(torch.zeros(3, H, W), z16, z32, H=H, W=W, r=1, E=81.0)
    with pytest.raises(ValueError, match="contiguous uint8"):
        ops.frame_detail_gain(torch.zeros(3, H, W, dtype=torch.uint8), z16, z32, H=H, W=W, r=1, E=81.0)
    with pytest.raises(ValueError, match="source: expected a contiguous fp16"):
        ops.frame_detail_gain(z16, z16[:, :, :8], z32, H=H, W=W, r=1, E=81.0)
    with pytest.raises(ValueError, match="contiguous int32"):
        ops.frame_detail_gain(z16, z16, torch.zeros(3, H, W), H=H, W=W, r=1, E=81.0)
    bad("multiple of 8", gain(W=36))
    bad("at least n n", gain(E=MT.edge_E(2, 0.5)))
    bad("at least n n", gain(E=float("nan")))
    bad("at least n n", gain(E=float("inf")))
    for field, value, match in ((2, 0, "radius 0, need 1..8"), (2, 9, "radius 9"), (3, 2, "unknown flag bits"), (3, 4, "unknown flag bits"),
                                (0, 0, "non-positive size")):
        op, keep = gain()
        op.i[field] = value
        bad(match, (op, keep))
    op, keep = gain()
    op.i[0], op.i[1] = 1 << 15, 1 << 15
    bad("below 2\\^31", (op, keep))
    for k in range(3):
        op, keep = gain()
        op.p[k] = op.p[k] + 4
        bad(f"pointer {k} is not 16-byte aligned", (op, keep))
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))

    # op 51
    def inject(H=H, W=W, Ho=Ho, Wo=Wo, **kw):
        args = dict(H=H, W=W, Ho=Ho, Wo=Wo, k=D.gain_scale(2, 1.0), limit=64.0)
        args.update(kw)
        S, C, L, O = (torch.zeros(Ho, Wo, 3, dtype=torch.uint8) for _ in range(4))
        tx, ty = (torch.from_numpy(MT.table_words(i, n)) for i, n in ((W, Wo), (H, Ho)))
        return ops.frame_detail(S, C, L, torch.zeros(3, H, W, dtype=torch.int32), tx, ty, O, **args)

    op, keep = inject(show=True)
    assert op.kind == 51 and [op.i[j] for j in range(5)] == [H, W, Ho, Wo, ops.DETAIL_SHOW] and op.p[7] is None
    assert op.f[0] == np.float32(1.0 / (25 * 4096.0)) and op.f[1] == 64.0
    ops.run((op, keep))
    ops.run(inject(H=8, W=16, Ho=5, Wo=9, limit=0.0, k=0.0))
    ops.run(inject(H=8, W=16, Ho=64, Wo=128))
    S, C, L, O = keep[0], keep[1], keep[2], keep[6]
    G, tx, ty = keep[3], keep[4], keep[5]
    geo = dict(H=H, W=W, Ho=Ho, Wo=Wo, k=0.0, limit=1.0)
    with pytest.raises(ValueError, match="camera: expected a contiguous uint8"):
        ops.frame_detail(S, C[:, :8], L, G, tx, ty, O, **geo)
    with pytest.raises(ValueError, match="gains: expected contiguous int32"):
        ops.frame_detail(S, C, L, G.float(), tx, ty, O, **geo)
    with pytest.raises(ValueError, match="tx must be a contiguous int32 table"):
        ops.frame_detail(S, C, L, G, ty, ty, O, **geo)
    for name, args in (("styled", (O, C, L)), ("camera", (S, O, L)), ("low", (S, C, O))):
        with pytest.raises(ValueError, match=f"dst may not be the {name} frame"):
            ops.frame_detail(*args, G, tx, ty, O, **geo)
    for kw in (dict(limit=-1.0), dict(limit=float("inf")), dict(limit=float("nan")), dict(k=float("nan")), dict(k=-1.0)):
        with pytest.raises(ValueError, match="finite and not negative"):
            inject(**kw)
    for slot, value in ((1, float("nan")), (1, float("inf")), (1, -1.0), (0, float("nan")), (0, -1.0)):
        op, keep = inject()
        op.f[slot] = value
        bad("finite and not negative", (op, keep))
    for field, value, match in ((4, 1, "unknown flag bits"), (4, 4, "unknown flag bits"), (0, 0, "non-positive size"), (2, 11, "between half and 8"),
                                (3, 8 * W + 1, "between half and 8"), (2, 4097, "must lie in 1..4096")):
        op, keep = inject()
        op.i[field] = value
        bad(match, (op, keep))
    op, keep = inject()
    op.i[0], op.i[1], op.i[2], op.i[3] = 1 << 15, 1 << 15, 1 << 15, 1 << 15
    bad("must lie in 1..4096", (op, keep))
    for k in (3, 4, 5):
        op, keep = inject()
        op.p[k] = op.p[k] + 2
        bad(f"pointer {k} .* is not 4-byte aligned", (op, keep))
    for k in range(7):
        op, keep = inject()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    for k in range(3):                                                        # dst inside an input's bytes
        op, keep = inject()
        op.p[6] = op.p[k] + 5
        bad(f"dst overlaps input {k}", (op, keep))

    # the plan of the device class: three records, the source resize into a buffer of its own
    dt = D.HipDetail(H, W, Ho, Wo, "lanczos", device="cpu")
    settings = D.check_settings(radius=3, eps=1.5, strength=0.5, limit=20.0, show=True)
    Sd, cam = torch.zeros(Ho, Wo, 3, dtype=torch.uint8), torch.zeros(Ho, Wo, 3, dtype=torch.uint8)
    for frame in (torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, 3, dtype=torch.uint8)):
        pl = dt.plan(Sd, frame, torch.zeros(3, H, W, dtype=torch.float16), cam, settings)
        assert [op.kind for op in pl] == [50, 46, 51]
        assert pl[1].p[1] == dt.low.data_ptr() and pl[2].p[2] == dt.low.data_ptr() and pl[2].p[6] == dt.dev.data_ptr()
        assert pl[0].p[2] == dt.gains.data_ptr() == pl[2].p[3] and pl[2].p[0] == Sd.data_ptr() and pl[2].p[1] == cam.data_ptr()
        assert pl[0].i[2] == 3 and pl[2].i[4] == ops.DETAIL_SHOW and pl[2].f[0] == D.gain_scale(3, 0.5) and pl[2].f[1] == 20.0
        pl.run()
    with pytest.raises(ValueError, match="multiple of 8"):
        D.HipDetail(24, 36, 36, 54, device="cpu")


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
def test_wrapper_host_route(monkeypatch):
    import pipeline_mocks as M
    from test_matte_cpu import build
    warm, frames = M.frames(8, seed=7), M.frames(5, seed=8)
    SIZE = (M.H * 2, M.W * 2 - 8)

    def run(detail):
        torch.manual_seed(123)
        w = build(monkeypatch, 2)
        w.set_output_size(*SIZE)
        if detail:
            w.set_detail(**detail)
        w.prepare(warm, "a prompt")
        return w

    def call(w, f):
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return w(f)

    w, twin = run(dict(radius=3, eps=1.5, strength=2.0, limit=100.0)), run(None)
    assert w.detail == dict(radius=3, eps=1.5, strength=2.0, limit=100.0, show=False) and twin.detail is None
    assert w._matte_line is not None and w.stream.matte_tap is w._matte_line and twin._matte_line is None
    assert w._camera is None                      # (no device: nothing taps the camera frame)
    for t in range(2):                            # the host route: byte-identical with the mode on and off
        got, plain = call(w, frames[t]), call(twin, frames[t])
        assert got.dtype == np.uint8 and got.shape == SIZE + (3,) and np.array_equal(got, plain), t
    w.set_detail()                                # the setting round-trips, defaults included
    assert w.detail == D.check_settings()
    assert np.array_equal(call(w, frames[2]), call(twin, frames[2]))
    for bad in (dict(radius=0), dict(eps=0.5), dict(strength=5), dict(limit=300)):
        with pytest.raises(ValueError, match="detail: "):
            w.set_detail(**bad)
    assert w.detail == D.check_settings()
    # the delay line is shared: the detail mode keeps it while a matte comes and goes, and the last user releases it
    w.set_matte(0.3, 0.7)
    w.clear_matte()
    assert w._matte_line is not None and w.stream.matte_tap is w._matte_line
    w.clear_detail()
    assert w.detail is None and w._matte_line is None and w.stream.matte_tap is None and w._detail_dev is None and w._camera is None
    assert np.array_equal(call(w, frames[3]), call(twin, frames[3]))
    w.set_steady()
    w.set_detail()
    w.clear_detail()
    assert w._matte_line is not None                                           # (the steady mode still needs it)
    # an output type the mode does not serve
    for ot in ("pt", "np", "latent"):
        twin.output_type = ot
        with pytest.raises(ValueError, match="set_detail: output_type=.*'u8'.*'pil'.*'jpeg'"):
            twin.set_detail()
    assert twin.detail is None and twin._matte_line is None
    twin.output_type = "u8"
    twin.set_detail()
    twin.clear_output_size()                      # (an output size would be named first)
    twin.output_type = "np"
    with pytest.raises(ValueError, match="the detail mode is set and output_type='np'.*clear_detail"):
        twin(frames[4])


def test_wrapper_keyword_and_the_tap(monkeypatch):
    """`detail=` at construction is `set_detail`; with a device's frame I/O the mode installs the camera tap while an output size
    is set, shares it with the "camera" matte, and `clear_detail` takes it out"""
    import pipeline_mocks as M
    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    from test_matte_cpu import RampDepth
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)

    def make(**more):
        pipe = M.MockPipe()
        pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), RampDepth()
        pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
        return Wrapper.from_components(pipe, output_type="u8", dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50,
                                       t_index_list=[10, 20], width=M.W, height=M.H, **more)

    for bad in (2, "2,1", [2, 1.0]):
        with pytest.raises(ValueError, match="detail="):
            make(detail=bad)
    with pytest.raises(ValueError, match="detail: radius"):
        make(detail=dict(radius=0))
    w = make(detail=dict(radius=4, strength=0.5))
    assert w.detail == dict(radius=4, eps=2.0, strength=0.5, limit=64.0, show=False)
    assert w._matte_line is not None and w._camera is None
    # a stand-in for the device's frame I/O: what `_sync_camera` installs the tap into
    w.io = types.SimpleNamespace(camera_tap=None, device=torch.device("cpu"))
    w.set_output_size(M.H * 2, M.W * 2, "bicubic")
    tap = w._camera
    assert tap is not None and w.io.camera_tap is tap and w._matte_line.camera_source is tap
    assert tap.key == (M.H * 2, M.W * 2, "bicubic")
    w.set_detail(radius=2)                                                     # a changed setting keeps the tap
    assert w._camera is tap
    w.set_output_size(M.H * 2, M.W * 2, "lanczos")                             # a changed filter rebuilds it
    assert w._camera is not tap and w._camera.key == (M.H * 2, M.W * 2, "lanczos")
    w.set_matte(0.2, 0.8)
    w.set_matte_source("camera")
    tap = w._camera
    w.clear_detail()                                                           # the "camera" matte still needs the tap
    assert w._camera is tap and w.io.camera_tap is tap and w._matte_line is not None
    w.set_detail()
    w.clear_matte()                                                            # ... and the detail mode does, without the matte
    assert w._camera is tap and w.io.camera_tap is tap
    w.set_matte_source("stream")
    assert w._camera is tap
    # under a "stream" matte a slot's camera buffer belongs to the detail mode alone: the composite stays at the stream's size
    w.set_matte(0.2, 0.8)
    slot = types.SimpleNamespace(camera=types.SimpleNamespace(key=tap.key))
    assert not w._camera_slot(slot, torch.zeros(1))
    w.clear_matte()
    w.clear_detail()
    assert w._camera is None and w.io.camera_tap is None and w._matte_line is None and w.stream.matte_tap is None
    w.set_detail()
    w.clear_output_size()                                                      # no output size: no tap, the line stays
    assert w._camera is None and w.io.camera_tap is None and w._matte_line is not None


# ----------------------------------------------------------------------------- the planted case
@pytest.fixture(scope="module")
def case():
    c = planted()
    c["plain"] = resize_ref(D.frame_bytes(c["styled"]), c["Ho"], c["Wo"])
    c["e_plain"] = err(c["plain"], c["truth"])
    return c


@pytest.mark.parametrize("radius", [1, 2, 4, 8])
def test_planted_detail_halves_the_error(case, radius):
    """(the prototype's figures: 380 273 for the plain Lanczos resize, 93 767 at radius 2 -- a ratio of 0.247; 0.25-0.29 over
    the radii)"""
    out = D.detail_ref(case["styled"], case["source"], case["cam"], case["Ho"], case["Wo"], radius=radius, eps=1, strength=1, limit=64)
    e = err(out, case["truth"])
    print(f"radius {radius}: e(plain) {case['e_plain']}, e(detail) {e}, ratio {e / case['e_plain']:.3f}")
    assert 2 * e <= case["e_plain"]
    if radius == 2:
        assert (case["e_plain"], e) == (380273, 93767)


@pytest.mark.parametrize("radius", [1, 2, 4, 8])
def test_planted_large_eps_is_no_worse_than_plain(case, radius):
    """(the prototype's ratios: 0.81-0.99)"""
    out = D.detail_ref(case["styled"], case["source"], case["cam"], case["Ho"], case["Wo"], radius=radius, eps=30, strength=1, limit=64)
    e = err(out, case["truth"])
    print(f"radius {radius}, eps 30: ratio {e / case['e_plain']:.3f}")
    assert e <= case["e_plain"]


def test_planted_source_as_its_own_style(case):
    """the source frame as its own styled frame gets the camera frame back (the prototype: 32 717 / 457 533 = 0.072)"""
    plain = resize_ref(D.frame_bytes(case["source"]), case["Ho"], case["Wo"])
    out = D.detail_ref(case["source"], case["source"], case["cam"], case["Ho"], case["Wo"], radius=2, eps=1, limit=255)
    e_plain, e = err(plain, case["cam"]), err(out, case["cam"])
    print(f"e(plain) {e_plain}, e(detail) {e}, ratio {e / e_plain:.3f}")
    assert 5 * e <= e_plain
