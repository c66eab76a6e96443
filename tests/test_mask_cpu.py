"""CPU tests (-m "not gpu") of the matte from the caller (live2diff_amd/mask_io.py): the four exact
properties of the byte-quantised mask, `unit_ref`, `invert`, a crop offset, the ties of 255 r, the refusals, the builders and the
launchers of op 58 and of the plane flags of ops 49 and 54 (dry-run), and `mask=` / `set_mask` / `warmup_masks=` on the wrapper
built from the mock components of tests/pipeline_mocks.py -- the N - 1 delay, alternating frames, the sticky mask, a dropped
frame, and edge, hold, backdrop and `show` over a mask against the oracles composed by hand.  There is no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from live2diff_amd import backdrop as BD
from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from live2diff_amd.frame_io import egress_ref
from test_matte_cpu import build, src_bytes

H, W = 40, 72


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def frame16(seed, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(3, h, w, generator=g) * 2.2 - 1.1).to(torch.float16)


def depth16(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    d = np.clip(np.linspace(-1.0, 1.0, w)[None] + 0.2 * rng.standard_normal((h, w)), -1, 1).astype(np.float16)
    return d


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("shape", [(40, 72), (30, 54), (320, 576), (45, 100)])
def test_four_properties(shape):
    styled, source, depth = frame16(1), frame16(2), depth16(3)
    lo, hi = 0.3, 0.7
    full, none = np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)
    for keep in ("near", "far"):
        ramp = MT.matte_ref(depth, lo, hi, 0, keep)[0]
        assert float(ramp.min()) < float(ramp.max())
        # a 255 mask under "and", a 0 mask under "or": the ramp's bits
        assert np.array_equal(bits(MI.front_ref(MI.mask_ref(full, H, W), depth, lo, hi, keep, "and")), bits(ramp))
        assert np.array_equal(bits(MI.front_ref(MI.mask_ref(none, H, W), depth, lo, hi, keep, "or")), bits(ramp))
        # ... and the inverted twins
        assert np.array_equal(bits(MI.front_ref(MI.mask_ref(none, H, W, invert=True), depth, lo, hi, keep, "and")), bits(ramp))
        assert np.array_equal(bits(MI.front_ref(MI.mask_ref(full, H, W, invert=True), depth, lo, hi, keep, "or")), bits(ramp))
    # "replace" with 255: the styled frame's bytes; with 0: the source frame's -- whatever the feather
    for feather in (0, 3):
        one = MI.front_ref(MI.mask_ref(full, H, W), None, lo, hi, "near", "replace")
        zero = MI.front_ref(MI.mask_ref(none, H, W), None, lo, hi, "near", "replace")
        assert np.array_equal(bits(one), bits(np.ones((H, W)))) and np.array_equal(bits(zero), bits(np.zeros((H, W))))
        got = MT.composite_ref(styled[None], source[None], depth[None], lo, hi, feather, plane=one[None])[0]
        assert np.array_equal(got, egress_ref(styled[None])[0].numpy())
        got = MT.composite_ref(styled[None], source[None], depth[None], lo, hi, feather, plane=zero[None])[0]
        assert np.array_equal(got, egress_ref(source[None])[0].numpy())


def test_constant_masks_of_every_type():
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535), (np.float32, 1.0), (np.float16, 1.0), (np.bool_, True)):
        for shape in ((30, 54), (320, 576)):
            assert np.all(MI.mask_ref(np.full(shape, top, dtype), H, W) == 255), (dtype, shape)
            assert np.all(MI.mask_ref(np.zeros(shape, dtype), H, W) == 0), (dtype, shape)
    t = torch.full((30, 54), True)
    assert np.all(MI.mask_ref(t, H, W) == 255) and np.all(MI.mask_ref(t.to(torch.float16), H, W) == 255)
    assert np.all(MI.mask_ref(torch.full((30, 54), -1, dtype=torch.int16), H, W) == 255)       # (the bits of uint16 65535)


def test_unit_ref():
    x = np.array([[np.nan, -0.5, -0.0, 0.0, 0.25, 1.0, 1.5, np.inf, -np.inf]], np.float32)
    v = MI.unit_ref(x)
    assert v.dtype == np.float32 and np.array_equal(v, np.array([[0, 0, 0, 0, 0.25, 1, 1, 1, 0]], np.float32))
    b = np.arange(256, dtype=np.uint8)[None]
    assert np.array_equal(bits(MI.unit_ref(b)), bits(b.astype(np.float32) / np.float32(255)))
    s = np.array([[0, 1, 257, 32768, 65535]], np.uint16)
    assert np.array_equal(bits(MI.unit_ref(s)), bits(s.astype(np.float32) / np.float32(65535)))
    h = np.array([[0.5, 2.0, np.nan]], np.float16)
    assert np.array_equal(MI.unit_ref(h), np.array([[0.5, 1.0, 0.0]], np.float32))
    for bad in (np.zeros((4, 4), np.int32), np.zeros((4, 4), np.float64), np.zeros((1, 4, 4), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="mask:"):
            MI.unit_ref(bad)


def test_invert_and_a_crop_offset():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (64, 96), dtype=np.uint8)
    assert MI.tables(64, 96, 64, 64)[0] == (64, 96, 0, 16)
    P = MI.mask_ref(m, 64, 64)
    assert np.array_equal(P, m[:, 16:80])                                  # 1 : 1, the centred window
    assert np.array_equal(MI.mask_ref(m, 64, 64, invert=True), 255 - m[:, 16:80])
    m = rng.integers(0, 256, (30, 54), dtype=np.uint8)
    assert np.array_equal(MI.mask_ref(m, H, W, invert=True), 255 - MI.mask_ref(m, H, W))
    u16 = (m.astype(np.uint16) * 257)
    assert np.array_equal(MI.mask_ref(m, H, W), MI.mask_ref(m.astype(np.float32) / np.float32(255), H, W))
    assert MI.mask_ref(u16, H, W).dtype == np.uint8


def test_ties_of_255_r_round_half_to_even():
    """a 30 x 54 byte mask to 40 x 72: exact ties of 255 r do occur, so the kernel has to match r bit for bit"""
    from live2diff_amd.depth_io import _taps
    rng = np.random.default_rng(0)
    m = rng.integers(0, 256, (30, 54), dtype=np.uint8)
    _, ymin, wy, xmin, wx = MI.tables(30, 54, H, W)
    r = _taps(_taps(MI.unit_ref(m), xmin.numpy().astype(np.int64), wx.numpy(), 1), ymin.numpy().astype(np.int64), wy.numpy(), 0)
    x = np.float32(255.0) * np.minimum(np.maximum(r, np.float32(0)), np.float32(1))
    tie = x - np.floor(x) == np.float32(0.5)
    assert int(tie.sum()) >= 10
    P = MI.mask_ref(m, H, W)
    assert np.all(P[tie] % 2 == 0) and np.array_equal(P[tie], (np.floor(x[tie]) + (np.floor(x[tie]) % 2)).astype(np.uint8))
    # r itself, by Python scalars on a few pixels: the horizontal pass first, taps ascending, every step rounded
    f32 = np.float32
    v = MI.unit_ref(m)
    for y, xo in ((0, 0), (17, 33), (39, 71), (20, 5)):
        acc = f32(0)
        for k in range(wy.shape[1]):
            row = min(int(ymin[y]) + k, 29)
            h = f32(0)
            for j in range(wx.shape[1]):
                h = f32(h + f32(f32(wx[xo, j]) * v[row, min(int(xmin[xo]) + j, 53)]))
            acc = f32(acc + f32(f32(wy[y, k]) * h))
        assert bits(acc) == bits(r[y, xo])


def test_front_ref_combines():
    depth = depth16(9)
    rng = np.random.default_rng(2)
    P = rng.integers(0, 256, (H, W), dtype=np.uint8)
    mu = P.astype(np.float32) / np.float32(255)
    ramp = MT.matte_ref(depth, 0.2, 0.6, 0, "far")[0]
    assert np.array_equal(bits(MI.front_ref(P, None, 0.2, 0.6, "far", "replace")), bits(mu))
    assert np.array_equal(bits(MI.front_ref(P, depth, 0.2, 0.6, "far", "and")), bits(np.minimum(ramp, mu)))
    assert np.array_equal(bits(MI.front_ref(P, depth, 0.2, 0.6, "far", "or")), bits(np.maximum(ramp, mu)))
    assert np.array_equal(np.rint(mu * np.float32(255)).astype(np.uint8), P)       # op 49 and the backdrop recover P itself
    with pytest.raises(ValueError):
        MI.front_ref(P.astype(np.float32), depth, 0.2, 0.6)
    with pytest.raises(ValueError, match="depth plane"):
        MI.front_ref(P, depth16(1, 8, 8), 0.2, 0.6, "near", "and")


def test_value_errors():
    for kw in (dict(combine="xor"), dict(combine=None), dict(combine="AND"), dict(invert=1), dict(invert="yes"), dict(invert=None)):
        with pytest.raises(ValueError, match="mask input"):
            MI.check_settings(**kw)
    assert MI.check_settings() == MI.DEFAULTS == dict(combine="replace", invert=False)
    assert MI.check_settings("or", np.bool_(True)) == dict(combine="or", invert=True)
    for hm, wm in ((64, 64), (72, 40), (400, 721), (330, 600)):             # outside the window, above scale 8
        with pytest.raises(ValueError, match="^mask: "):
            MI.mask_ref(np.zeros((hm, wm), np.uint8), H, W)
    with pytest.raises(ValueError, match="^mask: .*down-scale above"):
        MI.tables(400, 721, H, W)
    with pytest.raises(ValueError, match="mode"):
        from PIL import Image
        MI.load(Image.new("RGB", (8, 8)))
    with pytest.raises(ValueError, match="cannot be read"):
        MI.load(os.path.abspath(__file__))


def test_plane_keyword_on_the_backdrop_oracles():
    source, depth = frame16(4), depth16(5)
    matte = dict(lo=0.3, hi=0.7, keep="far")
    ramp = MT.matte_ref(depth, 0.3, 0.7, 0, "far")[0]
    assert np.array_equal(BD.weight_ref(depth, 0.3, 0.7, "far"), BD.weight_ref(None, 0.3, 0.7, "far", plane=ramp))
    assert np.array_equal(BD.blur_ref(source, depth, 0.3, 0.7, "far", 3, 2), BD.blur_ref(source, None, 0.3, 0.7, "far", 3, 2, plane=ramp))
    st = BD.check_settings("blur", 2, 1)
    rng = np.random.default_rng(3)
    plane = MI.front_ref(rng.integers(0, 256, (H, W), dtype=np.uint8), None, 0, 1)
    a = BD.stream_ref(st, None, source, depth, matte, plane=plane)
    assert np.array_equal(a, BD.frame_of(BD.blur_ref(source, depth, 0.3, 0.7, "far", 2, 1, plane=plane)))
    assert not np.array_equal(a, BD.stream_ref(st, None, source, depth, matte))
    b = BD.output_ref(st, None, source, depth, matte, 80, 144, plane=plane)
    assert b.shape == (80, 144, 3) and not np.array_equal(b, BD.output_ref(st, None, source, depth, matte, 80, 144))
    ones = np.ones((H, W), np.float32)
    assert np.all(BD.weight_ref(None, 0, 1, plane=ones) == 1) and np.all(BD.weight_ref(None, 0, 1, plane=0 * ones) == 256)


# ----------------------------------------------------------------------------- builders and launchers (dry run)
@pytest.fixture
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    assert _lib.OP_MASK_INGEST == 58
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_MASK_INGEST = 58," in hdr
    assert all(f"#define L2D_MASK_{n} {v} " in hdr for n, v in (
        ("U16", ops.MASK_U16), ("F32", ops.MASK_F32), ("INVERT", ops.MASK_INVERT), ("AND", ops.MASK_AND), ("OR", ops.MASK_OR),
        ("RAMP_HARD", ops.MASK_RAMP_HARD), ("RAMP_FAR", ops.MASK_RAMP_FAR)))
    assert f"#define L2D_MATTE_EDGE_PLANE {ops.MATTE_EDGE_PLANE} " in hdr and f"#define L2D_BACKDROP_PLANE {ops.BACKDROP_PLANE} " in hdr
    assert ops.MATTE_EDGE_PLANE == ops.BACKDROP_PLANE == 32                          # (16 was refused by both ops before, and stays refused)

    def ingest(Hm=30, Wm=54, dtype=torch.uint8, **kw):
        geo, ymin, wy, xmin, wx = MI.tables(Hm, Wm, H, W)
        args = dict(src=torch.zeros(Hm, Wm, dtype=dtype), out=torch.zeros(H, W), depth=torch.zeros(H, W, dtype=torch.float16),
                    xmin=xmin, wx=wx, ymin=ymin, wy=wy, Hm=Hm, Wm=Wm, H=H, W=W, nh=geo[0], nw=geo[1], top=geo[2], left=geo[3])
        args.update(kw)
        return ops.mask_ingest(*[args.pop(k) for k in ("src", "out", "depth", "xmin", "wx", "ymin", "wy")], **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, keep = ingest(dtype=torch.float32, combine="or", invert=True, lo32=-0.4, inv32=1.25, far=True)
    assert op.kind == 58 and [op.p[j] for j in range(7)] == [t.data_ptr() for t in keep] and op.p[7] is None
    assert [op.i[j] for j in range(11)] == [30, 54, H, W, 40, 72, 0, 0, keep[4].shape[1], keep[6].shape[1],
                                            ops.MASK_F32 | ops.MASK_OR | ops.MASK_INVERT | ops.MASK_RAMP_FAR]
    assert (op.f[0], op.f[1]) == (float(np.float32(-0.4)), 1.25)
    ops.run((op, keep))
    op, keep = ingest(combine="replace", lo32=-0.4, inv32=1.25, far=True)           # (a replacing mask: no depth, no ramp)
    assert op.p[2] is None and op.i[10] == 0 and op.f[0] == op.f[1] == 0.0
    for kw in (dict(), dict(dtype=torch.int16), dict(dtype=torch.uint16), dict(dtype=torch.float32), dict(Hm=320, Wm=576), dict(Hm=40, Wm=72),
               dict(combine="and", lo32=0.0, inv32=0.0, hard=True), dict(combine="or", lo32=-0.2, inv32=2.0), dict(invert=True)):
        ops.run(ingest(**kw))
    for call in (lambda: ingest(dtype=torch.int32), lambda: ingest(src=torch.zeros(30, 55, dtype=torch.uint8)),
                 lambda: ingest(out=torch.zeros(H, W, dtype=torch.float16)), lambda: ingest(out=torch.zeros(H, W + 1)),
                 lambda: ingest(combine="xor"), lambda: ingest(combine="and", depth=None), lambda: ingest(combine="or", depth=torch.zeros(H, W)),
                 lambda: ingest(xmin=torch.zeros(W, dtype=torch.int64)), lambda: ingest(wy=torch.zeros(H + 1, 3))):
        with pytest.raises(ValueError, match="mask_ingest"):
            call()
    for k, v, match in ((10, 32, "unknown flag bits"), (10, 256, "unknown flag bits"), (10, 3, "two sample types"), (10, 24, "two sample types"),
                        (10, 64, "ramp flags without"), (0, 0, "non-positive size"), (3, -8, "non-positive size"), (6, 1, "crop window"),
                        (7, -1, "crop window"), (4, 3, "crop window"), (8, 0, "taps"), (9, 18, "taps"), (0, 400, "exceeds 8")):
        op, keep = ingest()
        op.i[k] = v
        bad(match, (op, keep))
    for k in range(7):
        op, keep = ingest(combine="and", lo32=-0.2, inv32=2.0)
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    op, keep = ingest()
    assert op.p[2] is None
    op, keep = ingest(dtype=torch.float32)
    op.p[0] += 2
    bad("not aligned to its element", (op, keep))
    op, keep = ingest()
    op.p[1] += 8
    bad("not aligned to its element", (op, keep))
    op, keep = ingest()
    op.p[4] += 2
    bad("pointer 4 is not 4-byte aligned", (op, keep))
    for kw in (dict(lo32=-1.5), dict(inv32=-1.0), dict(inv32=float("inf")), dict(inv32=0.0), dict(hard=True)):
        bad("must lie in \\[-1, 1\\]", ingest(combine="and", **dict(dict(lo32=-0.2, inv32=2.0), **kw)))
    x = torch.zeros(H, W)
    bad("overlaps", ingest(Hm=H, Wm=W, dtype=torch.float32, src=x, out=x))
    raw = torch.zeros(4 * H * W, dtype=torch.uint8)
    bad("overlaps", ingest(combine="or", lo32=-0.2, inv32=2.0, out=raw.view(torch.float32).view(H, W),
                           depth=raw[:2 * H * W].view(torch.float16).view(H, W)))

    # ops 49 and 54 under their plane flags
    src, d, out32, out16, pl = (torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float16), torch.zeros(H, W),
                                torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W))
    E = MT.edge_E(2, 4.0)
    op, keep = ops.frame_matte_edge(src, None, out32, H=H, W=W, r=2, E=E, plane=pl)
    assert op.kind == 49 and op.p[1] == pl.data_ptr() and op.i[3] == ops.MATTE_EDGE_PLANE and op.f[0] == op.f[1] == 0.0
    ops.run((op, keep))
    ops.run(ops.frame_matte_edge(src, d, out32, H=H, W=W, r=2, E=E, lo32=-0.4, inv32=1.25, hard=False))
    op, keep = ops.frame_backdrop_blur(src, None, out16, H=H, W=W, r=2, passes=3, plane=pl)
    assert op.kind == 54 and op.p[1] == pl.data_ptr() and op.i[4] == ops.BACKDROP_PLANE
    ops.run((op, keep))
    ops.run(ops.frame_backdrop_blur(src, d, out16, H=H, W=W, r=2, passes=3, lo32=-0.4, inv32=1.25, hard=False))
    for build_op, iflag in ((lambda **kw: ops.frame_matte_edge(src, None, out32, H=H, W=W, r=2, E=E, **kw), 3),
                            (lambda **kw: ops.frame_backdrop_blur(src, None, out16, H=H, W=W, r=2, passes=1, **kw), 4)):
        for kw in (dict(), dict(plane=pl, far=True), dict(plane=pl, hard=True), dict(plane=pl.to(torch.float16)), dict(plane=torch.zeros(H, W + 8))):
            with pytest.raises(ValueError):
                build_op(**kw)
        op, keep = build_op(plane=pl)
        op.i[iflag] |= ops.MATTE_FAR
        bad("ramp flags beside", (op, keep))
        op, keep = build_op(plane=pl)
        op.i[iflag] |= 16
        bad("unknown flag bits", (op, keep))
        op, keep = build_op(plane=pl)
        op.p[1] += 8
        bad("not 16-byte aligned", (op, keep))
    with pytest.raises(ValueError, match="plane= goes with depth=None"):
        ops.frame_matte_edge(src, d, out32, H=H, W=W, r=2, E=E, plane=pl)
    bad("overlaps the input plane", ops.frame_matte_edge(src, None, pl, H=H, W=W, r=2, E=E, plane=pl))
    bad("overlaps pointer 1", _overlapping_blur(ops, src))


def _overlapping_blur(ops, src):
    buf = torch.zeros(6 * H * W, dtype=torch.uint8)
    out = buf.view(torch.float16).view(3, H, W)
    plane = buf[2 * H * W:6 * H * W].view(torch.float32).view(H, W)          # the last 4 H W bytes of the output: an fp32 plane's reach
    return ops.frame_backdrop_blur(src, None, out, H=H, W=W, r=2, passes=1, plane=plane)


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
def call(w, f, **kw):
    torch.manual_seed(77)                        # (the host path draws its re-noising from the global generator)
    return w(f, **kw)


def made(monkeypatch, n=2, matte=dict(lo=0.3, hi=0.7, keep="near", feather=0), drop=None, warmup_masks=None, **setup):
    import pipeline_mocks as M
    torch.manual_seed(123)
    w = build(monkeypatch, n, drop=drop)
    if matte is not None:
        w.set_matte(matte["lo"], matte["hi"], keep=matte["keep"], feather=matte["feather"])
    for name, kw in setup.items():
        getattr(w, "set_" + name)(**kw)
    w.prepare(M.frames(8, seed=7), "a prompt", **({} if warmup_masks is None else {"warmup_masks": warmup_masks}))
    return w


def binary(seed, shape=(64, 64)):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < 0.5).astype(np.uint8) * np.uint8(255)


def frames_of(k, seed=8):
    import pipeline_mocks as M
    return list(M.frames(k, seed=seed))


@pytest.mark.parametrize("n", [2, 3])
def test_wrapper_delay_alternating_and_warmup_masks(monkeypatch, n):
    """"replace" with a binary 1 : 1 mask per frame: output k shows the styled frame where the mask of frame k - (N - 1) is 255
    and that frame's own source bytes where it is 0 -- a mask composited with the wrong frame shows"""
    import pipeline_mocks as M
    frames = frames_of(7)
    masks = [binary(s) if s not in (2, 5) else None for s in range(7)]            # frames 2 and 5 bring none: the ramp alone
    warm_masks = [binary(100 + j) for j in range(8)]
    w, twin = made(monkeypatch, n, warmup_masks=warm_masks), made(monkeypatch, n)
    warm_src = src_bytes(M.frames(8, seed=7)[-1])
    for k in range(7):
        got = call(w, frames[k], **({} if masks[k] is None else {"mask": masks[k]}))
        plain = call(twin, frames[k])
        styled = egress_ref(w.stream.prev_image_result)[0].numpy()
        j = k - (n - 1)
        m, src = (warm_masks[-1], warm_src) if j < 0 else (masks[j], src_bytes(frames[j]))
        if m is None:
            assert np.array_equal(got, plain), k                                   # the parent's frame, byte for byte
            continue
        assert np.array_equal(got[m == 255], styled[m == 255]) and np.array_equal(got[m == 0], src[m == 0]), k
        assert not np.array_equal(got, plain), k
    assert w._matte_line.last.mask is not None or masks[7 - n] is None


def test_wrapper_warmup_masks_none_and_value_errors(monkeypatch):
    import pipeline_mocks as M
    w, twin = made(monkeypatch, 2), made(monkeypatch, 2)
    f = frames_of(2)
    assert np.array_equal(call(w, f[0], mask=binary(1)), call(twin, f[0]))         # the primed position has no mask
    assert not np.array_equal(call(w, f[1]), call(twin, f[1]))
    for bad in ([binary(1)] * 3, [], 5):
        with pytest.raises(ValueError, match="warmup_masks"):
            w.prepare(M.frames(8, seed=7), "a prompt", warmup_masks=bad)
    with pytest.raises(ValueError, match="^mask: "):
        w(f[0], mask=np.zeros((64, 100), np.float64))
    with pytest.raises(ValueError, match="^mask: "):
        w(f[0], mask=np.zeros((600, 600), np.uint8))                               # above scale 8
    with pytest.raises(ValueError, match="mask input"):
        w.set_mask_input("both")
    # a batch of masks as a tensor
    torch.manual_seed(123)
    w.prepare(M.frames(8, seed=7), "a prompt", warmup_masks=torch.from_numpy(np.stack([binary(50 + j) for j in range(8)])))
    got = call(w, f[0])
    m = binary(57)
    assert np.array_equal(got[m == 0], src_bytes(M.frames(8, seed=7)[-1])[m == 0])


def test_a_mask_needs_a_matte(monkeypatch):
    import pipeline_mocks as M
    w = made(monkeypatch, 2, matte=None)
    f = frames_of(1)[0]
    assert w.mask is False and w.mask_input == MI.DEFAULTS
    with pytest.raises(ValueError, match="needs a matte"):
        w(f, mask=binary(1))
    with pytest.raises(ValueError, match="needs a matte"):
        w.set_mask(binary(1))
    with pytest.raises(ValueError, match="needs a matte"):
        w.prepare(M.frames(8, seed=7), "a prompt", warmup_masks=[binary(1)] * 8)
    w.set_mask_input("and", invert=True)                                           # (a setting: allowed without)
    assert w.mask_input == dict(combine="and", invert=True)
    w.set_matte(0.3, 0.7)
    w.set_mask(binary(1))
    assert w.mask is True
    w.clear_matte()
    assert w.mask is False and w._mask_tap is None


def test_wrapper_sticky_mask(monkeypatch):
    frames = frames_of(5)
    region, own = binary(40, (48, 48)), binary(41)
    w, twin = made(monkeypatch, 2), made(monkeypatch, 2)
    w.set_mask(region)
    assert w.mask is True
    region[...] = 0                                                                # (the wrapper kept a copy)
    P = MI.mask_ref(binary(40, (48, 48)), 64, 64)
    outs = []
    for k in range(5):
        if k == 3:
            w.clear_mask()
        got = call(w, frames[k], **({"mask": own} if k == 1 else {}))
        plain = call(twin, frames[k])
        slot = w._matte_line.last
        want = {0: None, 1: P, 2: MI.mask_ref(own, 64, 64), 3: P, 4: None}[k]      # (delayed by one; frame 0's slot was primed without)
        if want is None:
            assert np.array_equal(got, plain), k
        else:
            plane = MI.front_ref(want, None, 0, 1)
            assert np.array_equal(got, MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **w.matte,
                                                        plane=plane[None])[0]), k
        outs.append(got)
    assert w.mask is False


def test_wrapper_dropped_frame_ignores_its_mask(monkeypatch):
    frames = frames_of(5)
    masks = [binary(60 + k) for k in range(5)]
    w = made(monkeypatch, 2, drop={2})
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    got = [call(w, frames[k], mask=masks[k]) for k in range(5)]
    assert np.array_equal(got[2], got[1]) and w._matte_line.tapped == 4
    styled = egress_ref(w.stream.prev_image_result)[0].numpy()
    m, src = masks[3], src_bytes(frames[3])                                        # output 4 belongs to frame 3: mask 2 was never used
    assert np.array_equal(got[4][m == 255], styled[m == 255]) and np.array_equal(got[4][m == 0], src[m == 0])
    assert w._mask_tap.pending is None


class ByHand:
    """the oracles composed by hand beside a wrapper: front_ref -> edge_ref -> hold_ref -> composite_ref(plane=)"""

    def __init__(self):
        self.state = None

    def step(self, w, mask, init=False):
        slot, mt, mi = w._matte_line.last, w.matte, w.mask_input
        P = MI.mask_ref(mask, 64, 64, mi["invert"])
        raw = MI.front_ref(P, slot.depth, mt["lo"], mt["hi"], mt["keep"], mi["combine"])
        m0 = raw if w.matte_edge is None else MT.edge_ref(raw, slot.source, **w.matte_edge)
        if w.matte_hold is not None:
            m0, self.state, _ = MT.hold_ref(m0, slot.source, self.state, init=init or self.state is None, **w.matte_hold)
        more = {}
        if w.backdrop is not None and not mt["show"]:
            more["backdrop"] = BD.stream_ref(w.backdrop, None, slot.source, slot.depth, mt, plane=raw)[None]
        return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **mt, plane=m0[None], **more)[0]


def soft(seed, shape):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    blob = np.exp(-(((yy - shape[0] / 2) / (shape[0] / 4)) ** 2 + ((xx - shape[1] / 2) / (shape[1] / 4)) ** 2))
    return np.clip(blob + 0.1 * rng.standard_normal(shape), -0.2, 1.2).astype(np.float32)


@pytest.mark.parametrize("combine,invert", [("replace", False), ("and", True), ("or", False)])
def test_wrapper_edge_hold_backdrop_and_show_over_a_mask(monkeypatch, combine, invert):
    frames = frames_of(8)
    masks = [soft(70 + k, (48, 80)) if k % 2 else (soft(70 + k, (96, 96)) * 65535).clip(0, 65535).astype(np.uint16) for k in range(8)]
    w = made(monkeypatch, 2, matte=dict(lo=0.3, hi=0.7, keep="far", feather=2), warmup_masks=[masks[0]] * 8,
             mask_input=dict(combine=combine, invert=invert))
    hand = ByHand()
    seen = [masks[0]] + masks                    # the mask of output k: the one that entered a frame earlier
    k = 0

    def step(init=False):
        nonlocal k
        got = call(w, frames[k], mask=masks[k])
        assert got.dtype == np.uint8 and np.array_equal(got, hand.step(w, seen[k], init=init)), k
        k += 1
        return got

    plain = step()
    w.set_matte_edge(radius=2, eps=4.0)
    assert not np.array_equal(step(), plain)
    w.set_matte_hold(strength=0.6)
    step(init=True)
    step()
    w.set_backdrop("blur", radius=2, passes=2)
    step()
    w.clear_matte_edge()
    step(init=True)
    w.set_matte(0.3, 0.7, keep="far", feather=1, show=True)
    shown = step(init=True)
    assert np.array_equal(shown[..., 0], shown[..., 1])
    # set_mask_input applies from the next output on, to the mask that is already in the line
    w.set_mask_input("or" if combine != "or" else "and", invert=not invert)
    step(init=True)


def test_constructor_keyword(monkeypatch):
    import inspect

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["mask_input"].default is None
    for name in ("img2img", "push", "__call__"):
        assert inspect.signature(getattr(Wrapper, name)).parameters["mask"].default is None
    assert inspect.signature(Wrapper.prepare).parameters["warmup_masks"].default is None
    real = Wrapper.from_components
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, mask_input=dict(combine="and"), **kw)))
    assert build(monkeypatch, 2).mask_input == dict(combine="and", invert=False)
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, mask_input="and", **kw)))
    with pytest.raises(ValueError, match="mask_input="):
        build(monkeypatch, 2)
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, mask_input=dict(combine="nor"), **kw)))
    with pytest.raises(ValueError, match="mask input"):
        build(monkeypatch, 2)


def test_pil_images_and_paths(tmp_path):
    from PIL import Image
    m = binary(3, (30, 54))
    p = tmp_path / "m.png"
    Image.fromarray(m).save(p)
    assert np.array_equal(MI.mask_ref(MI.load(str(p)), H, W), MI.mask_ref(m, H, W))
    assert np.array_equal(MI.mask_ref(MI.load(Image.fromarray(m).convert("1")), H, W), MI.mask_ref(m, H, W))
    u16 = (m.astype(np.uint16) * 257)
    im = Image.fromarray(u16)
    assert im.mode.startswith("I;16") and np.array_equal(MI.mask_ref(MI.load(im), H, W), MI.mask_ref(u16, H, W))
    f = Image.fromarray(soft(1, (30, 54)))
    assert f.mode == "F" and np.array_equal(MI.mask_ref(MI.load(f), H, W), MI.mask_ref(soft(1, (30, 54)), H, W))
