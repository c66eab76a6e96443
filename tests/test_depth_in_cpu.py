"""CPU tests (-m "not gpu") of the depth input (live2diff_amd/depth_io.py): the numpy oracle `depth_ref`
against independent statements of what it computes, its holes, kinds, ranges and batches, the validation, the two launchers in
dry-run mode, and the pipeline and the wrapper on CPU tensors with the mocks of tests/pipeline_mocks.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from live2diff_amd import depth_io as D
from live2diff_amd.frame_io import geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24          # the relative error of one fp32 operation


def rnd(seed):
    return np.random.default_rng(seed)


def smooth(seed, B, Hd, Wd, lo=0.5, hi=5.0):
    """float32 [B,Hd,Wd] in [lo, hi]: a few low-frequency waves plus noise -- not flat, and no two frames alike"""
    g = rnd(seed)
    y, x = np.mgrid[0:Hd, 0:Wd].astype(np.float64)
    out = []
    for b in range(B):
        a = np.sin(x / Wd * (3 + b) + g.uniform(0, 6)) * np.cos(y / Hd * (2 + b) + g.uniform(0, 6)) + 0.1 * g.standard_normal((Hd, Wd))
        a = (a - a.min()) / (a.max() - a.min())
        out.append(lo + (hi - lo) * a)
    return np.stack(out).astype(np.float32)


# ----------------------------------------------------------------------------- the oracle against independent statements
@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_identity_case_against_fp64(dtype):
    """The depth frame has the output's own size and every sample is valid: the triangle filter has the weights (1, 0) -- the
    product 1 u, the sum 0 + u and the quotient u / 1 are exact --, so R = u and, with range=None,
    dn = fp16(2 (u - min) / (max - min) - 1).

    The bound.  n = fl(fl(u - mn) / fl(mx - mn)): three fp32 operations on a value in [0, 1], each within a relative 2^-24, so
    |n - n_exact| <= 3 x 2^-24 (1 + 2^-23) < 3.01 x 2^-24.  2 n is exact; fl(2 n - 1) adds at most 2^-24 (half an ulp of a value
    in [-1, 1]): the fp32 value is within (2 x 3.01 + 1) x 2^-24 < 7.1 x 2^-24 = 4.3e-7 of the exact one.  The single rounding to
    fp16 of a value in [-1, 1] is within half an ulp of the binade [0.5, 1), 2^-12 = 2.4414e-4 (11 significant bits).  Together
    2^-12 + 7.1 x 2^-24 < 2.4457e-4."""
    H, W = 40, 72
    z = smooth(1, 2, H, W)
    if dtype == "uint16":
        z = np.round(z * 1000.0).astype(np.uint16)
    dn = D.depth_ref(z, H, W, kind="inverse", invalid=None)
    assert dn.dtype == np.float16 and dn.shape == (2, 3, H, W)
    assert np.array_equal(dn[:, 0], dn[:, 1]) and np.array_equal(dn[:, 0], dn[:, 2])
    assert np.array_equal(D.resample_ref(z, H, W, kind="inverse", invalid=None), z.astype(np.float32))
    u = z.astype(np.float64)
    want = 2.0 * (u - u.min()) / (u.max() - u.min()) - 1.0
    err = np.abs(dn[:, 0].astype(np.float64) - want).max()
    print(f"identity {dtype}: max |dn - fp64| = {err:.6e}")
    assert err <= 2.0 ** -12 + 7.1 * EPS32
    assert dn.min() == -1.0 and dn.max() == 1.0


@pytest.mark.parametrize("Hd,Wd,H,W,what", [(97, 173, 64, 64, "non-integer down-scale, non-square, left > 0"),
                                            (133, 217, 64, 64, "non-integer down-scale"),
                                            (30, 54, 40, 72, "up-scale"),
                                            (320, 576, 40, 72, "exactly scale 8")])
def test_resampled_case_against_torch(Hd, Wd, H, W, what):
    """On a fully valid fp32 map the oracle's R is `F.interpolate(mode="bilinear", antialias=True)` to the resized size + the centre
    crop of `frame_io.geometry`: den = sum of the weights, num = the filtered map.

    The bound, against torch in fp32 (which forms the same fp32 weights by the same expressions, tests/test_frame_io_cpu.py, but
    may order and fuse its sums differently).  Per axis a sum of at most 17 taps is 17 products of weights <= 1 and 17 additions
    of partial sums <= M = max |u|: at most 34 roundings of 2^-24 M each.  Two axes, for num on our side and for torch's result on
    its side: 4 x 34.  den is the same sum of the weights alone, 2 x 34 roundings around 1, and the division adds one: R = num / den
    moves by at most (2 x 34 + 1) 2^-24 M more.  In all |R - torch| <= (6 x 34 + 1) 2^-24 M = 205 x 2^-24 M, 1.22e-5 M."""
    z = smooth(2, 1, Hd, Wd)
    M = float(z.max())
    R = D.resample_ref(z, H, W, kind="inverse", invalid=None)
    nh, nw, top, left = geometry(Hd, Wd, H, W)
    if "left > 0" in what:
        assert left > 0
    want = F.interpolate(torch.from_numpy(z)[None], (nh, nw), mode="bilinear", align_corners=False, antialias=True)[0]
    want = want[:, top:top + H, left:left + W].numpy()
    err = np.abs(R.astype(np.float64) - want.astype(np.float64)).max()
    print(f"{Hd}x{Wd} -> {H}x{W} ({what}): max |R - torch| = {err:.6e}, bound {205 * EPS32 * M:.6e}")
    assert (R >= 0).all()
    assert err <= 205 * EPS32 * M


# ----------------------------------------------------------------------------- holes
def footprint(Hd, Wd, H, W, ys, xs):
    """bool [H,W]: the output pixels whose taps (with a weight above 0) reach a sample of rows `ys` x columns `xs`"""
    _, ymin, wy, xmin, wx = D.tables(Hd, Wd, H, W)

    def axis(lo, w, sel, n):
        hit = np.zeros(lo.shape[0], bool)
        for j in range(w.shape[1]):
            idx = lo.numpy() + j
            hit |= (w[:, j].numpy() > 0) & np.isin(idx, sel) & (idx < n)
        return hit
    return axis(ymin, wy, ys, Hd)[:, None] & axis(xmin, wx, xs, Wd)[None, :]


def test_an_isolated_hole_is_filled_by_its_neighbours():
    Hd, Wd, H, W = 97, 173, 64, 64
    z = np.round(smooth(3, 1, Hd, Wd) * 1000).astype(np.uint16)
    full = D.resample_ref(z, H, W)
    holed = z.copy()
    holed[0, 50, 90] = 0
    R = D.resample_ref(holed, H, W)
    fp = footprint(Hd, Wd, H, W, [50], [90])
    assert fp.any() and (R >= 0).all()                                       # every pixel still has a value
    assert np.array_equal(R[0][~fp], full[0][~fp])                           # only the footprint's pixels change
    assert (R[0][fp] != full[0][fp]).any()
    _, ymin, wy, xmin, wx = D.tables(Hd, Wd, H, W)
    with np.errstate(divide="ignore"):
        u = 1.0 / holed[0].astype(np.float64)
    for y, x in zip(*np.nonzero(fp)):
        ys = np.arange(int(ymin[y]), min(int(ymin[y]) + wy.shape[1], Hd))
        xs = np.arange(int(xmin[x]), min(int(xmin[x]) + wx.shape[1], Wd))
        patch = u[np.ix_(ys, xs)]
        valid = patch[np.isfinite(patch)]
        assert valid.min() * (1 - 1e-5) <= R[0, y, x] <= valid.max() * (1 + 1e-5)


def test_large_hole_all_invalid_flat_and_nearest_point():
    Hd, Wd, H, W = 97, 173, 64, 64
    z = np.round(smooth(4, 1, Hd, Wd) * 1000).astype(np.uint16)
    holed = z.copy()
    holed[0, 30:60, 70:110] = 0                                              # far larger than the 2 x 2 support of ~1.5
    R = D.resample_ref(holed, H, W)
    dn = D.depth_ref(holed, H, W)
    inside = ~footprint(Hd, Wd, H, W, np.r_[0:30, 60:Hd], np.arange(Wd)) & ~footprint(Hd, Wd, H, W, np.arange(Hd), np.r_[0:70, 110:Wd])
    assert inside.sum() > 100
    assert (R[0][inside] == D.NO_VALUE).all() and (dn[0, 0][inside] == -1).all()
    assert (R[0][~inside] >= 0).any() and dn.max() == 1.0
    for dead in (np.zeros((Hd, Wd), np.uint16), np.full((Hd, Wd), np.nan, np.float32), np.full((Hd, Wd), -2.0, np.float32)):
        assert (D.resample_ref(dead, H, W) == D.NO_VALUE).all()
        assert (D.depth_ref(dead, H, W) == -1).all()
    assert (D.depth_ref(np.full((Hd, Wd), 1500, np.uint16), H, W) == -1).all()                      # flat: mx <= mn
    assert (D.depth_ref(np.full((Hd, Wd), 1.5, np.float32), H, W, range=(1.5, 1.5 + 1e-9)) == -1).all()         # mx <= mn once in fp32
    # a hole on the frame's nearest point moves the range to the next one
    near = z.copy()
    near[0, 40:48, 80:96] = 200                                              # much nearer than everything else (>= 500)
    a = D.resample_ref(near, H, W)
    near[0, 40:48, 80:96] = 0
    b = D.resample_ref(near, H, W)
    assert a.max() > b.max() * 2 and abs(b.max() - D.resample_ref(z, H, W).max()) / b.max() < 0.2
    dn_b = D.depth_ref(near, H, W)
    assert dn_b.max() == 1.0 and dn_b[0, 0][b[0] == b.max()][0] == 1.0


def test_float_specials_are_holes():
    z = smooth(5, 1, 40, 72)
    bad = z.copy()
    bad[0, 3, 4], bad[0, 10, 20], bad[0, 20, 30], bad[0, 30, 40], bad[0, 35, 50] = np.nan, np.inf, 0.0, -1.0, -np.inf
    for kind in D.KINDS:
        u, v = D.convert_ref(bad, kind, 0)
        assert v.sum() == v.size - 5 and np.isfinite(u).all() and (u >= 0).all()
        assert (D.resample_ref(bad, 40, 72, kind=kind) == D.NO_VALUE).sum() == 5          # identity: each hole is its own pixel
    u, v = D.convert_ref(bad, "inverse", None)
    assert v.sum() == v.size - 4                                             # 0 is a value of its own when nothing marks a hole
    u, v = D.convert_ref(bad, "distance", None)
    assert v.sum() == v.size - 5                                             # but no distance


def test_distance_is_inverse_of_the_reciprocal():
    for z in (smooth(6, 2, 97, 173), np.round(smooth(6, 2, 97, 173) * 1000).astype(np.uint16)):
        z[0, 5:9, 5:9] = 0
        with np.errstate(divide="ignore"):
            inv = (np.float32(1.0) / z.astype(np.float32))
        inv[~np.isfinite(inv)] = 0.0                                         # (1 / 0: the hole stays the value 0 marks)
        for rg in (None, (0.8, 3.0)):
            a = D.depth_ref(z, 64, 64, kind="distance", range=None if rg is None else tuple(v * (1000 if z.dtype == np.uint16 else 1) for v in rg))
            s = 1000.0 if z.dtype == np.uint16 else 1.0
            b = D.depth_ref(inv, 64, 64, kind="inverse", range=None if rg is None else
                            tuple(float(v) for v in D.fixed_range("distance", (rg[0] * s, rg[1] * s))))
            assert np.array_equal(a, b)


def test_fixed_range():
    Hd, Wd, H, W = 40, 72, 40, 72
    za, zb = smooth(7, 1, Hd, Wd, 0.5, 5.0), smooth(8, 1, Hd, Wd, 1.0, 9.0)
    za[0, 0, 0], za[0, 1, 1], za[0, 2, 2] = 0.1, 50.0, 2.0
    zb[0, 0, 0], zb[0, 1, 1], zb[0, 2, 2] = 0.2, 60.0, 2.0
    a, b = D.depth_ref(za, H, W, range=(1.0, 4.0)), D.depth_ref(zb, H, W, range=(1.0, 4.0))
    assert a[0, 0, 0, 0] == 1.0 and a[0, 0, 1, 1] == -1.0 and b[0, 0, 0, 0] == 1.0 and b[0, 0, 1, 1] == -1.0      # nearer than near, farther than far
    assert a[0, 0, 2, 2] == b[0, 0, 2, 2] and -1 < a[0, 0, 2, 2] < 1          # an equal z maps to an equal dn ...
    a0, b0 = D.depth_ref(za, H, W), D.depth_ref(zb, H, W)
    assert a0[0, 0, 2, 2] != b0[0, 0, 2, 2]                                   # ... and with range=None it does not
    far = D.depth_ref(za, H, W, range=(1.0, float("inf")))                    # far = inf: mn = 0
    want = np.clip(1.0 / za[0].astype(np.float64), 0, 1) * 2 - 1
    assert np.abs(far[0, 0].astype(np.float64) - want).max() <= 2.0 ** -12 + 8 * EPS32
    inv = D.depth_ref(za, H, W, kind="inverse", range=(1.0, 4.0))
    assert inv[0, 0, 0, 0] == -1.0 and inv[0, 0, 1, 1] == 1.0
    assert D.fixed_range("distance", (0.5, float("inf"))) == (0.0, 2.0) and D.fixed_range("inverse", (0.0, 3.0)) == (0.0, 3.0)


def test_a_batch_is_normalised_jointly():
    z = np.stack([smooth(9, 1, 48, 48, 1.0 + b, 2.0 + b)[0] for b in range(8)])
    joint = D.depth_ref(z, 64, 64)
    single = np.concatenate([D.depth_ref(z[b], 64, 64) for b in range(8)])
    assert joint.shape == (8, 3, 64, 64)
    assert all(single[b].min() == -1 and single[b].max() == 1 for b in range(8))
    assert joint[0].max() == 1 and joint[7].min() == -1 and joint[0].min() > -1 and joint[7].max() < 1
    assert not np.array_equal(joint, single)
    R = D.resample_ref(z, 64, 64)
    assert np.array_equal(joint, D.normalize_ref(R)) and np.array_equal(joint, D.normalize_ref(R, (R.min(), R.max())))
    p = D.partials_ref(R)
    assert p.shape == (8 * 4 * 2, 3) and p[:, 0].min() == R.min() and p[:, 1].max() == R.max() and (p[:, 2] == 1).all()


# ----------------------------------------------------------------------------- validation
def test_validation_names_the_keyword():
    assert D.check_settings() == dict(kind="distance", invalid=0, range=None) == D.DEFAULTS
    assert D.check_settings("inverse", None, [0, 2]) == dict(kind="inverse", invalid=None, range=(0.0, 2.0))
    assert D.check_settings(invalid=65535.0)["invalid"] == 65535 and D.check_settings(range=(0.3, float("inf")))["range"][1] == float("inf")
    for kw, match in ((dict(kind="metric"), "kind="), (dict(kind=None), "kind="), (dict(invalid="0"), "invalid="),
                      (dict(invalid=float("nan")), "invalid="), (dict(invalid=True), "invalid="), (dict(range=3.0), "range="),
                      (dict(range=(1.0,)), "range="), (dict(range=(2.0, 1.0)), "range="), (dict(range=(0.0, 1.0)), "range="),
                      (dict(range=(1.0, 1.0)), "range="), (dict(range=(float("nan"), 1.0)), "range="),
                      (dict(kind="inverse", range=(-1.0, 1.0)), "range="), (dict(kind="inverse", range=(0.0, float("inf"))), "range=")):
        with pytest.raises(ValueError, match=match):
            D.check_settings(**kw)
        with pytest.raises(ValueError, match=match):
            D.depth_ref(np.ones((8, 8), np.float32), 8, 8, **kw)
    with pytest.raises(ValueError, match="depth: .*does not lie inside"):
        D.depth_ref(np.ones((97, 173), np.uint16), 40, 72)                   # 173 / 97 is narrower than 72 / 40
    with pytest.raises(ValueError, match="depth: .*down-scale above 8"):
        D.depth_ref(np.ones((8 * 40 + 8, 8 * 72 + 15), np.uint16), 40, 72)
    with pytest.raises(ValueError, match="depth: expected uint16 or float32"):
        D.depth_ref(np.ones((8, 8), np.int32), 8, 8)
    with pytest.raises(ValueError, match=r"depth: expected \[Hd,Wd\]"):
        D.depth_ref(np.ones((1, 1, 8, 8), np.float32), 8, 8)
    # fp16 and uint8 are widened exactly
    z = smooth(10, 1, 16, 24).astype(np.float16)
    assert np.array_equal(D.depth_ref(z, 16, 24), D.depth_ref(z.astype(np.float32), 16, 24))
    z8 = rnd(10).integers(0, 256, (16, 24)).astype(np.uint8)
    assert np.array_equal(D.depth_ref(z8, 16, 24), D.depth_ref(z8.astype(np.uint16), 16, 24))
    assert np.array_equal(D.depth_ref(torch.from_numpy(z8), 16, 24), D.depth_ref(z8, 16, 24))
    z16 = rnd(11).integers(30000, 65536, (16, 24)).astype(np.uint16)         # a torch int16 tensor holds the bits of uint16 samples
    assert np.array_equal(D.depth_ref(torch.from_numpy(z16.view(np.int16)), 16, 24), D.depth_ref(z16, 16, 24))


# ----------------------------------------------------------------------------- header and the launchers (dry-run)
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def records(B=1, Hd=97, Wd=173, H=64, W=64, dtype=torch.int16, fixed=None, invalid=0, distance=True):
    from live2diff_amd import ops
    (nh, nw, top, left), ymin, wy, xmin, wx = D.tables(Hd, Wd, H, W)
    src = torch.zeros(B, Hd, Wd, dtype=dtype)
    R = torch.zeros(B, H, W)
    part = torch.zeros(B * ops.depth_tiles(H, W), 3)
    out = torch.zeros(B, 3, H, W, dtype=torch.float16)
    a = ops.depth_ingest(src, R, part, xmin, wx, ymin, wy, B=B, Hd=Hd, Wd=Wd, H=H, W=W, nh=nh, nw=nw, top=top, left=left,
                         distance=distance, invalid=invalid)
    b = ops.depth_normalize(R, part, out, B=B, H=H, W=W, fixed=fixed)
    return a, b


def test_header_and_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert "L2D_OP_DEPTH_INGEST = 52," in hdr and _lib.OP_DEPTH_INGEST == 52
    assert "L2D_OP_DEPTH_NORMALIZE = 53," in hdr and _lib.OP_DEPTH_NORMALIZE == 53
    for name in ("F32", "DISTANCE", "HAS_INVALID", "FIXED_RANGE", "TILE_H", "TILE_W", "MAX_TAPS"):
        assert f"#define L2D_DEPTH_{name} {getattr(ops, 'DEPTH_' + name)}" in hdr
    assert "#define L2D_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    # valid records pass
    for kw in (dict(), dict(B=8), dict(dtype=torch.float32, invalid=None, distance=False), dict(fixed=(0.25, 2.0)),
               dict(Hd=320, Wd=576, H=40, W=72), dict(Hd=30, Wd=54, H=40, W=72), dict(Hd=512, Wd=512)):
        a, b = records(**kw)
        ops.run(a)
        ops.run(b)
    a, b = records(dtype=torch.float32, fixed=(0.5, 2.0), invalid=0.0)
    assert a[0].kind == 52 and a[0].i[11] == ops.DEPTH_F32 | ops.DEPTH_DISTANCE | ops.DEPTH_HAS_INVALID
    assert b[0].kind == 53 and b[0].i[4] == ops.DEPTH_FIXED_RANGE and (b[0].f[0], b[0].f[1]) == (0.5, 2.0)
    assert records(invalid=None)[0][0].i[11] == ops.DEPTH_DISTANCE and records(invalid=70000)[0][0].i[11] == ops.DEPTH_DISTANCE
    # op 52
    for k in range(7):
        op, keep = records()[0]
        op.p[k] = None
        bad(f"depth_ingest.*pointer {k} is null", (op, keep))
    for field, value, match in ((0, 0, "depth_ingest.*non-positive size"), (0, -1, "depth_ingest.*non-positive size"),
                                (3, 0, "depth_ingest.*non-positive size"), (5, 12, "depth_ingest.*scale 8.083"),
                                (6, 21, "depth_ingest.*outside the resized image"), (9, 18, "depth_ingest.*taps"),
                                (10, 0, "depth_ingest.*taps"), (11, 8, "depth_ingest.*unknown flag bits"),
                                (12, 70000, "depth_ingest.*no uint16"), (7, -1, "depth_ingest.*outside the resized image")):
        op, keep = records()[0]
        if field == 5:
            op.i[3], op.i[7] = 12, 0                                         # (H = nh = 12: the window lies inside, the scale is 97 / 12)
        op.i[field] = value
        bad(match, (op, keep))
    op, keep = records()[0]
    op.i[0], op.i[1], op.i[2] = 8, 1 << 14, 1 << 14
    bad("depth_ingest.*below 2\\^31", (op, keep))
    op, keep = records(dtype=torch.float32)[0]
    op.p[0] = op.p[0] + 2
    bad("depth_ingest.*not aligned", (op, keep))
    # op 53
    for k in range(3):
        op, keep = records()[1]
        op.p[k] = None
        bad(f"depth_normalize.*pointer {k} is null", (op, keep))
    for field, value, match in ((0, 0, "depth_normalize.*non-positive size"), (0, -2, "depth_normalize.*non-positive size"),
                                (3, 7, "depth_normalize.*7 partials"), (4, 1, "depth_normalize.*unknown flag bits")):
        op, keep = records()[1]
        op.i[field] = value
        bad(match, (op, keep))
    op, keep = records()[1]
    op.i[1], op.i[2] = 63, 60
    bad("depth_normalize.*multiple of 8", (op, keep))
    op, keep = records(fixed=(0.0, 1.0))[1]
    op.f[1] = float("nan")
    bad("depth_normalize.*NaN", (op, keep))
    with pytest.raises(ValueError, match="depth: .*down-scale above 8"):
        records(Hd=8 * 64 + 8, Wd=8 * 64 + 8)
    with pytest.raises(ValueError, match="expected uint16 or float32"):
        ops.depth_ingest(torch.zeros(1, 8, 8, dtype=torch.int32), *[None] * 6, B=1, Hd=8, Wd=8, H=8, W=8, nh=8, nw=8, top=0, left=0,
                         distance=True, invalid=0)


# ----------------------------------------------------------------------------- the pipeline and the wrapper on CPU tensors
class CountingDepth:
    dtype = torch.float32

    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def __call__(self, x):
        self.calls += 1
        return self.inner(x)


class Tap:
    def __init__(self):
        self.seen, self.primed = [], []

    def __call__(self, x, dn):
        self.seen.append((x.clone(), dn.clone()))

    def prime(self, x, dn):
        self.primed.append((x.clone(), dn.clone()))


def build(monkeypatch, **kw):
    from test_matte_cpu import build as build_wrapper
    w = build_wrapper(monkeypatch, 2)
    s = w.stream
    s.depth_detector = CountingDepth(s.depth_detector)
    s.vae = CountingVAE(s.vae)
    return w


class CountingVAE:
    def __init__(self, inner):
        self.inner, self.encoded = inner, []
        self.dtype, self.config = inner.dtype, inner.config

    def encode(self, x):
        self.encoded.append(x.clone())
        return self.inner.encode(x)

    def decode(self, *a, **kw):
        return self.inner.decode(*a, **kw)


def test_pipeline_on_cpu_tensors(monkeypatch):
    import pipeline_mocks as M
    w = build(monkeypatch)
    s = w.stream
    tap = s.matte_tap = Tap()
    warm, frames = M.frames(8, seed=7), M.frames(4, seed=8)
    wd = np.round(smooth(11, 8, 48, 80) * 1000).astype(np.uint16)
    wd[:, 10:12, 10:12] = 0
    d = np.round(smooth(12, 4, 48, 80) * 1000).astype(np.uint16)

    w.prepare(warm, "a prompt", warmup_depths=wd)
    assert s.depth_detector.calls == 0 and len(tap.primed) == 1
    want = torch.from_numpy(D.depth_ref(wd, M.H, M.W)).float()
    assert torch.equal(tap.primed[0][1], want)                               # the warm-up batch, normalised jointly
    assert torch.equal(s.vae.encoded[1], want)                               # (encoded[0]: the frames themselves)

    n = len(s.vae.encoded)
    w(frames[0], depth=d[0])
    assert s.depth_detector.calls == 0 and len(tap.seen) == 1
    want = torch.from_numpy(D.depth_ref(d[0], M.H, M.W)).float()
    assert torch.equal(tap.seen[0][1], want) and torch.equal(tap.seen[0][0], 2.0 * frames[0][None] - 1.0)
    assert len(s.vae.encoded) == n + 2 and torch.equal(s.vae.encoded[n + 1], want)
    lat = M.MockVAE().encode(want).latents * M.MockVAE.config.scaling_factor
    assert torch.equal(s.depth_latent_buffer[0, :, 0], lat[0])               # the depth latent: the VAE mock's encode of that map

    w.set_depth_input(kind="distance", invalid=0, range=(0.5 * 1000, 5.0 * 1000))
    assert w.depth_input == dict(kind="distance", invalid=0, range=(500.0, 5000.0))
    w(frames[1], depth=torch.from_numpy(d[1].astype(np.float32)))            # a float32 tensor, the new settings
    assert torch.equal(tap.seen[1][1], torch.from_numpy(D.depth_ref(d[1].astype(np.float32), M.H, M.W, range=(500.0, 5000.0))).float())
    assert s.depth_detector.calls == 0
    w(frames[2])                                                             # mixing is allowed: this one takes the detector
    assert s.depth_detector.calls == 1 and len(tap.seen) == 3


def test_without_depth_the_call_sequence_is_the_parents(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), M.frames(3, seed=8)
    outs, logs = [], []
    for settings in (None, dict(kind="inverse", invalid=None, range=(0.0, 2.0))):
        torch.manual_seed(0)                                                 # (`prepare` draws from the global generator)
        w = build(monkeypatch)
        if settings is not None:
            w.set_depth_input(**settings)                                    # settings alone change nothing
        w.prepare(warm, "a prompt")
        got = [w(f) for f in frames]
        outs.append(got)
        logs.append((w.stream.depth_detector.calls, len(w.stream.vae.encoded)))
    assert logs[0] == logs[1] == (1 + 3, 2 + 2 * 3)                          # prepare + 3 frames: the detector each time, two encodes each
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_depth_source_input_and_the_wrapper_arguments(monkeypatch, tmp_path):
    import pipeline_mocks as M
    from PIL import Image
    from live2diff_amd import wrapper as Wr
    from test_matte_cpu import build as build_wrapper
    warm, frames = M.frames(8, seed=7), M.frames(3, seed=8)
    wd = np.round(smooth(14, 8, 48, 80) * 1000).astype(np.uint16)
    d = np.round(smooth(15, 1, 48, 80) * 1000).astype(np.uint16)[0]
    w = build(monkeypatch)
    assert w.depth_source == "detector" and w.depth_input == D.DEFAULTS
    w.prepare(warm, "a prompt", warmup_depths=list(wd))
    tap = w.stream.matte_tap = Tap()
    Image.fromarray(d).save(tmp_path / "d.png")                              # a 16-bit PNG
    assert Image.open(tmp_path / "d.png").mode in ("I;16", "I")
    for arg in (d, torch.from_numpy(d.astype(np.float32)), Image.fromarray(d), str(tmp_path / "d.png"), Image.fromarray(d.astype(np.float32))):
        w(frames[0], depth=arg)
    assert all(torch.equal(dn, tap.seen[0][1]) for _, dn in tap.seen[1:]) and w.stream.depth_detector.calls == 0
    with pytest.raises(ValueError, match="depth: a depth image must have mode"):
        w(frames[0], depth=Image.new("RGB", (8, 8)))
    with pytest.raises(ValueError, match="depth: expected one depth frame per frame"):
        w(frames[0], depth=wd)
    with pytest.raises(ValueError, match="warmup_depths: expected a batch"):
        w.prepare(warm, "a prompt", warmup_depths=wd[:3])
    with pytest.raises(ValueError, match="kind="):
        w.set_depth_input(kind="metric")
    assert w.depth_input == D.DEFAULTS

    # depth_source="input": no detector is needed or built, and a frame without depth says so
    import live2diff_amd.pipeline_stream_animation_depth as P
    pipe = M.MockPipe()
    pipe.unet, pipe.vae = M.MockStreamUNet(), M.MockVAE()                    # (no depth_model)
    pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    wi = Wr.StreamAnimateDiffusionDepthWrapper.from_components(
        pipe, output_type="u8", dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50, t_index_list=[10, 20], width=M.W,
        height=M.H, depth_source="input", depth_input=dict(kind="inverse", invalid=None))
    s = wi.stream
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor, s.unet_warmup = M.MockImageProcessor(), M.MockWarmupUNet()
    assert wi.depth_source == "input" and s.depth_detector is None and wi.depth_input == dict(kind="inverse", invalid=None, range=None)
    with pytest.raises(ValueError, match="warmup_depths"):
        wi.prepare(warm, "a prompt")
    wi.prepare(warm, "a prompt", warmup_depths=wd)
    assert wi(frames[0], depth=d).shape == (M.H, M.W, 3)
    with pytest.raises(ValueError, match="depth"):
        wi(frames[1])
    with pytest.raises(ValueError, match="depth"):
        s(frames[1])                                                         # the pipeline itself: no detector to fall back to
    for kw, match in ((dict(depth_source="camera"), "depth_source="), (dict(depth_input="distance"), "depth_input=")):
        with pytest.raises(ValueError, match=match):
            Wr.StreamAnimateDiffusionDepthWrapper.from_components(pipe, num_inference_steps=50, t_index_list=[10, 20], width=M.W,
                                                                  height=M.H, device="cpu", dtype=torch.float32, **kw)
    with pytest.raises(ValueError, match="depth_source="):
        Wr.load_components({}, height=64, width=64, denoising_steps_num=2, depth_source="none")


def test_a_dropped_frame_ignores_its_depth(monkeypatch):
    import pipeline_mocks as M
    from test_matte_cpu import build as build_wrapper
    w = build_wrapper(monkeypatch, 2, drop={1})
    tap = w.stream.matte_tap = Tap()
    w.prepare(M.frames(8, seed=7), "a prompt")
    frames = M.frames(3, seed=8)
    d = np.round(smooth(16, 1, 48, 80) * 1000).astype(np.uint16)[0]
    a = w(frames[0], depth=d)
    b = w(frames[1], depth=np.zeros((3, 3, 3), np.int64))                    # dropped: what came with it is never looked at
    assert len(tap.seen) == 1 and np.array_equal(a, b)


def test_stream_frames_reads_depth_by_file_name(tmp_path):
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import stream_frames as S
    finally:
        sys.path.pop(0)
    os.makedirs(tmp_path / "rgb")
    os.makedirs(tmp_path / "depth")
    for i in range(3):
        Image.fromarray(np.full((8, 12, 3), i, np.uint8)).save(tmp_path / "rgb" / f"{i:03d}.jpg")
        Image.fromarray(np.full((6, 10), 1000 + i, np.uint16)).save(tmp_path / "depth" / f"{i:03d}.png")
    z = S.read_depths(str(tmp_path / "depth"), str(tmp_path / "rgb"))
    assert z.shape == (3, 6, 10) and z.dtype == np.uint16 and list(z[:, 0, 0]) == [1000, 1001, 1002]
    os.remove(tmp_path / "depth" / "001.png")
    with pytest.raises(FileNotFoundError, match="001.png"):
        S.read_depths(str(tmp_path / "depth"), str(tmp_path / "rgb"))
    np.save(tmp_path / "d.npy", z.astype(np.float32))
    assert S.read_depths(str(tmp_path / "d.npy"), "frames.npy").dtype == np.float32
    with pytest.raises(ValueError, match="--depth"):
        S.read_depths(str(tmp_path / "depth"), "frames.npy")


def test_flat_margin_is_noise_only():
    """the flat rule (`depth_io.FLAT`) swallows the rounding noise of a constant frame at a non-integer scale, and nothing a
    sensor can resolve: a range of one part in a thousand is stretched to [-1, 1] like any other"""
    Hd, Wd, H, W = 97, 173, 64, 64
    R = D.resample_ref(np.full((Hd, Wd), 1.7, np.float32), H, W)
    spread = float(R.max() - R.min()) / float(R.max())
    print(f"constant frame at scale 1.52: R spreads by {spread:.3e} of its value")
    assert 0 < spread <= 274 * EPS32 < float(D.FLAT)                         # (the noise is there, within its bound, below the margin)
    assert (D.normalize_ref(R) == -1).all()
    z = np.full((Hd, Wd), 1.7, np.float32)
    z[40:60, 60:120] = 1.7017
    dn = D.depth_ref(z, H, W)
    assert dn.min() == -1 and dn.max() == 1


def test_a_narrow_fixed_range_is_taken_at_its_word():
    """the flat margin belongs to range=None; a fixed range inside it still clamps to +-1, and only mx <= mn is flat"""
    z = np.full((1, 40, 72), 2.0, np.float32)
    z[0, :20] = 2.00002                                                      # a relative range of 1e-5: inside the margin
    assert (D.depth_ref(z, 40, 72, kind="inverse", invalid=None) == -1).all()
    dn = D.depth_ref(z, 40, 72, kind="inverse", invalid=None, range=(2.000005, 2.00001))
    assert (dn[0, :, :20] == 1).all() and (dn[0, :, 20:] == -1).all()
    assert (D.normalize_ref(z, (2.0, 2.0)) == -1).all() and (D.normalize_ref(z, (2.1, 2.0)) == -1).all()
    with pytest.raises(ValueError, match="depth: a mode 'I' depth image must hold 16-bit samples"):
        from PIL import Image
        from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
        Wrapper._depth_arg(Wrapper.__new__(Wrapper), Image.fromarray(np.full((4, 4), 70000, np.int32)))
