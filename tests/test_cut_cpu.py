"""CPU tests (-m "not gpu") of the cut detector: the arithmetic of live2diff_amd/cut.py on hand-computed and
synthetic cases, `check_settings`, the builders of L2D_OP_FRAME_CUT_SIG / L2D_OP_FRAME_CUT and every refusal of their launchers in
dry-run mode, the detector inside `StreamAnimateDiffusionDepth` on the deterministic mocks of tests/pipeline_mocks.py (what a
frame launches with it off, that it adds no synchronisation when on) and the wrapper's automatic re-warm."""
import os

import numpy as np
import pytest
import torch

import pipeline_mocks as M
from test_rewarm_cpu import F, N, T_INDEX, LoggingWarmup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 30


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def f16(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float16))


def smooth(H, W, seed, cells=4):
    """a smooth picture in [-1, 1]: random colours on a cells x cells grid, bilinearly enlarged"""
    g = torch.Generator().manual_seed(seed)
    small = torch.rand(1, 3, cells, cells, generator=g) * 2.0 - 1.0
    return torch.nn.functional.interpolate(small, (H, W), mode="bilinear", align_corners=True)[0].numpy()


# ----------------------------------------------------------------------------- the arithmetic
def test_identical_frames_have_no_distance():
    from live2diff_amd import cut
    x = f16(smooth(64, 72, 1))
    recs = cut.cut_ref([x, x, x])
    assert recs.dtype == np.int32 and recs.shape == (3, 8)
    assert list(recs[0]) == [0, 0, 0, NEVER, 0, 0, 0, 0]
    assert list(recs[1]) == [0, 0, 0, NEVER, 1, 0, 0, 1] and list(recs[2]) == [0, 0, 0, NEVER, 2, 0, 0, 1]
    thumb, hist = cut.signature_ref(x)
    assert thumb.dtype == np.uint16 and thumb.shape == (8, 9) and hist.dtype == np.uint32 and hist.shape == (64,) and int(hist.sum()) == 64 * 72


def test_a_hand_computed_8_x_16_case():
    """x = -1, 0, 1 are the bytes 0, 128 (127.5, half to even), 255; the luma of a grey byte v is (256 v + 128) >> 8 = v.
    A: block 0 black, block 1 white.  B: block 0 grey.  C: B with the green of one pixel of block 0 at 255: Y = (77 * 128 + 150 * 255
    + 29 * 128 + 128) >> 8 = 51946 >> 8 = 202, bin 50.  D: C again.  thumb = 20 -> Tt = 20 * 64 * 2 = 2560; hist = 0.35 -> Th =
    rint(0.35 * 2 * 128) = rint(89.6) = 90."""
    from live2diff_amd import cut
    A = np.full((3, 8, 16), -1.0)
    A[:, :, 8:] = 1.0
    B = A.copy()
    B[:, :, :8] = 0.0
    C = B.copy()
    C[1, 3, 5] = 1.0
    assert cut.cut_params(8, 16) == (2560, 90, 768, 8)
    ta, ha = cut.signature_ref(f16(A))
    assert ta.tolist() == [[0, 16320]] and ha[0] == 64 and ha[63] == 64 and int(ha.sum()) == 128
    tb, hb = cut.signature_ref(f16(B))
    assert tb.tolist() == [[8192, 16320]] and hb[32] == 64 and hb[63] == 64
    tc, hc = cut.signature_ref(f16(C))
    assert tc.tolist() == [[8192 - 128 + 202, 16320]] and hc[32] == 63 and hc[50] == 1
    recs = cut.cut_ref([f16(A), f16(B), f16(C), f16(C)])
    assert recs[0].tolist() == [0, 0, 0, NEVER, 0, 0, 0, 0]
    assert recs[1].tolist() == [1, 8192, 128, 0, 1, 0, 0, 0]                 # a cut: since = 0, no level is formed from it
    assert recs[2].tolist() == [0, 74, 2, 1, 2, 256 * 74, 0, 1]              # the first frame that was no cut sets the level
    assert recs[3].tolist() == [0, 0, 0, 2, 3, 18944 - 2368, 0, 1]           # E + ((0 - 18944) >> 3)
    d = cut.record_dict(recs[2])
    assert d == dict(cut=False, Dt=74, Dh=2, since=1, n=2, level=74.0, has_level=True)


def sig_of(thumb, hist=None):
    hist = np.zeros(64, np.uint32) if hist is None else hist
    return np.asarray(thumb, dtype=np.uint16), np.asarray(hist, dtype=np.uint32)


def test_the_level_update_floors_and_spans_both_halves():
    from live2diff_amd import cut
    quiet = (1 << 30, 1 << 30, 0, 0)                                        # thresholds nothing reaches
    zero = sig_of(np.zeros((1, 2)))
    prev = np.array([0, 0, 0, 5, 7, 1001, 0, 1], dtype=np.int32)
    rec = cut.measure_ref(zero, zero, prev, quiet)
    assert rec.tolist() == [0, 0, 0, 6, 8, 1001 + (-126), 0, 1]              # (0 - 1001) >> 3 = floor(-125.125) = -126, not -125
    rec = cut.measure_ref(sig_of([[1, 0]]), zero, prev, quiet)
    assert rec.tolist() == [0, 1, 0, 6, 8, 1001 + (-94), 0, 1]               # (256 - 1001) >> 3 = floor(-93.125) = -94
    rec = cut.measure_ref(sig_of([[100, 0]]), zero, prev, quiet)
    assert rec.tolist() == [0, 100, 0, 6, 8, 1001 + (25600 - 1001) // 8, 0, 1]
    # 65,536 blocks that all move by 16,320: Dt = 1,069,547,520 < 2^30, 256 Dt = 63 * 2^32 + 3,221,225,472 needs both halves
    big = sig_of(np.full((256, 256), 16320))
    rec = cut.measure_ref(big, sig_of(np.zeros((256, 256))), np.array([0, 0, 0, NEVER, 0, 0, 0, 0], np.int32), quiet)
    Dt = 16320 * 65536
    assert rec.tolist() == [0, Dt, 0, NEVER, 1, (256 * Dt & 0xFFFFFFFF) - (1 << 32), 63, 1] and cut.level_of(rec) == 256 * Dt
    back = cut.measure_ref(sig_of(np.zeros((256, 256))), big, rec, quiet)    # ... and is read back from both
    assert cut.level_of(back) == 256 * Dt and back[1] == Dt
    # `since` saturates at 2^30
    assert cut.measure_ref(zero, zero, np.array([0, 0, 0, NEVER, 3, 0, 0, 1], np.int32), quiet)[3] == NEVER


def test_a_pan_is_no_cut_and_a_brightness_step_is_no_cut_and_another_picture_is():
    from live2diff_amd import cut
    H, W = 64, 128
    wide = smooth(H, W + 8, 3, cells=5)
    a, b = f16(wide[:, :, :W]), f16(wide[:, :, 8:])                           # the same smooth scene, 8 pixels on
    Tt, Th, _, _ = cut.cut_params(H, W)
    recs = cut.cut_ref([a, b])
    print("pan", recs[1].tolist(), Tt, Th)
    assert recs[1][0] == 0 and recs[1][2] < Th // 2                           # Dh is small: the same picture, nearly
    # + 12 byte levels everywhere: every pixel changes bin (12 >> 2 = 3 bins on), the block sums move by 12 * 64 < 20 * 64
    # (flat patches, so the histogram is a set of spikes; a smooth ramp's histogram is broad and overlaps itself three bins on)
    g = torch.Generator().manual_seed(4)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, 4, 8, generator=g) - 0.5, (H, W))[0].numpy()
    up = base + 2.0 * 12.0 / 255.0
    recs = cut.cut_ref([f16(base), f16(up)])
    print("step", recs[1].tolist(), Tt, Th)
    assert recs[1][0] == 0 and recs[1][1] < Tt and recs[1][2] > Th
    # two unrelated pictures of flat patches.  (Two smooth ramps of similar brightness can share most of their histogram: a pair
    # whose Dh is 0.25 of its largest value is missed at hist = 0.35 -- DESIGN.md section 8.z21 says so.)
    patches = lambda seed: f16(torch.nn.functional.interpolate(torch.rand(1, 3, 4, 8, generator=torch.Generator().manual_seed(seed)) * 2 - 1,
                                                               (H, W))[0].numpy())
    for seed in (5, 6, 7):
        recs = cut.cut_ref([patches(seed), patches(seed + 1)])
        print("cut", recs[1].tolist(), Tt, Th)
        assert recs[1][0] == 1 and recs[1][1] >= Tt and recs[1][2] >= Th and recs[1][3] == 0


def test_gap_suppresses_a_second_cut_and_reports_one_just_past_it():
    from live2diff_amd import cut
    a, b = f16(smooth(64, 64, 7)), f16(smooth(64, 64, 8))
    # a cut at frame 2; the next change of picture `k` frames behind it
    for k, want in ((3, 0), (4, 1)):
        frames = [a, a] + [b] * k + [a, a]
        recs = cut.cut_ref(frames, gap=3, ratio=0.0)
        cuts = [int(r[4]) for r in recs if r[0]]
        print(k, cuts, [int(r[3]) for r in recs])
        assert cuts == ([2, 2 + k] if want else [2])
        if not want:
            assert recs[2 + k][1] >= cut.cut_params(64, 64)[0] and recs[2 + k][3] == k     # it was far enough; `since` counts on


def test_steady_fast_motion_is_held_back_by_the_level():
    from live2diff_amd import cut
    H, W = 64, 64
    g = torch.Generator().manual_seed(9)
    # blocks of random grey, every frame a new draw: Dt and Dh pass their thresholds on EVERY frame
    frames = [f16(torch.nn.functional.interpolate(torch.rand(1, 1, 8, 8, generator=g) * 2 - 1, (H, W)).expand(1, 3, H, W)[0].numpy())
              for _ in range(21)]
    Tt, Th, _, _ = cut.cut_params(H, W)
    held = cut.cut_ref(frames, ratio=3.0, gap=8)
    assert all(r[1] >= Tt and r[2] >= Th for r in held[1:])
    # frame 1 has no level to be held against and is a cut; the frames inside its gap are no cuts and form the level; from there on
    # no frame moves three times as far as the frames before it
    assert [int(r[4]) for r in held if r[0]] == [1], held[:, :2].tolist()
    assert all(r[7] == 1 for r in held[2:]) and held[1][7] == 0
    free = cut.cut_ref(frames, ratio=0.0, gap=8)
    assert [int(r[4]) for r in free if r[0]] == [1, 10, 19]                 # with the level test off only the gap holds them back
    # ... and a sequence of nothing but cuts never forms a level: `E stays`
    bare = cut.cut_ref(frames[:6], ratio=3.0, gap=0)
    assert [int(r[0]) for r in bare] == [0, 1, 1, 1, 1, 1] and not bare[:, 5:].any()


def test_check_settings_and_sizes():
    from live2diff_amd import cut
    assert cut.check_settings() == dict(thumb=20.0, hist=0.35, ratio=3.0, gap=8)
    assert cut.check_settings(0, 1, 0, 255) == dict(thumb=0.0, hist=1.0, ratio=0.0, gap=255)
    assert cut.check_settings(255.0, 0.0, 64, 0)["ratio"] == 64.0 and cut.check_settings(ratio=1)["ratio"] == 1.0
    for kw, match in ((dict(thumb=-0.1), "thumb="), (dict(thumb=255.5), "thumb="), (dict(thumb="20"), "thumb="), (dict(thumb=True), "thumb="),
                      (dict(thumb=float("nan")), "thumb="), (dict(hist=-0.01), "hist="), (dict(hist=1.01), "hist="), (dict(hist=None), "hist="),
                      (dict(ratio=0.5), "ratio="), (dict(ratio=64.5), "ratio="), (dict(ratio=-1), "ratio="), (dict(ratio=False), "ratio="),
                      (dict(ratio="3"), "ratio="), (dict(gap=-1), "gap="), (dict(gap=256), "gap="), (dict(gap=2.0), "gap="), (dict(gap=True), "gap=")):
        with pytest.raises(ValueError, match=match):
            cut.check_settings(**kw)
    assert cut.cut_params(512, 512) == (20 * 512 * 512, int(np.rint(0.35 * 2 * 512 * 512)), 768, 8)
    assert cut.cut_params(2048, 2048, dict(thumb=255, hist=1, ratio=64, gap=255)) == (255 << 22, 2 << 22, 16384, 255)
    for H, W in ((0, 8), (8, 0), (12, 8), (8, 12), (2048, 2056), (-8, 8)):
        with pytest.raises(ValueError, match="multiples of 8"):
            cut.cut_params(H, W)
    with pytest.raises(ValueError, match="multiples of 8"):
        cut.signature_ref(np.zeros((3, 12, 8), np.float16))


# ----------------------------------------------------------------------------- the builders and the launchers, dry-run
def aligned(n, dtype, off=0):
    """a tensor of n elements at `off` bytes behind a 16-byte boundary"""
    item = torch.empty(0, dtype=dtype).element_size()
    buf = torch.zeros(n + 32 // item, dtype=dtype)
    skip = ((-buf.data_ptr()) % 16 + off) // item
    return buf[skip:skip + n]


def operands(H, W):
    from live2diff_amd import ops
    nwg = ops.frame_cut_tiles(H, W)
    st = lambda: (aligned(H * W // 64, torch.uint16).view(H // 8, W // 8), aligned(64, torch.uint32), aligned(8, torch.int32))
    return dict(x=aligned(3 * H * W, torch.float16).view(3, H, W), partials=aligned(nwg * 68, torch.uint32).view(nwg, 68), a=st(), b=st(), nwg=nwg)


def test_the_builders_fill_the_records(dry_run):
    from live2diff_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert _lib.OP_FRAME_CUT_SIG == 65 and _lib.OP_FRAME_CUT == 66
    assert "L2D_OP_FRAME_CUT_SIG = 65," in hdr and "L2D_OP_FRAME_CUT = 66," in hdr
    for name, v in (("INIT", ops.CUT_INIT), ("BLOCK", ops.CUT_BLOCK), ("BINS", ops.CUT_BINS), ("TILE", ops.CUT_TILE), ("PARTIAL", ops.CUT_PARTIAL),
                    ("MAX_PIXELS", ops.CUT_MAX_PIXELS), ("NEVER", ops.CUT_NEVER), ("MIN_R", ops.CUT_MIN_R), ("MAX_R", ops.CUT_MAX_R),
                    ("MAX_GAP", ops.CUT_MAX_GAP)):
        assert f"#define L2D_CUT_{name} {v} " in hdr or f"#define L2D_CUT_{name} {v}\n" in hdr, name
    assert [ops.frame_cut_tiles(*s) for s in ((8, 8), (64, 64), (72, 136), (8, 520), (512, 512), (2048, 2048))] == [1, 1, 6, 9, 64, 1024]
    H, W = 72, 136
    o = operands(H, W)
    op, keep = ops.frame_cut_sig(o["x"], None, o["a"][0], o["partials"], H=H, W=W)
    assert op.kind == 65 and list(op.i[:4]) == [H, W, 1, 6] and op.p[1] is None and op.p[2] == o["a"][0].data_ptr()
    ops.run((op, keep))
    op, keep = ops.frame_cut_sig(o["x"], o["a"][0], o["b"][0], o["partials"], H=H, W=W)
    assert list(op.i[:4]) == [H, W, 0, 6] and [op.p[k] for k in range(4)] == [t.data_ptr() for t in (o["x"], o["a"][0], o["b"][0], o["partials"])]
    ops.run((op, keep))
    op, keep = ops.frame_cut(o["partials"], None, o["a"], H=H, W=W, Tt=1, Th=2, R=0, gap=3)
    assert op.kind == 66 and list(op.i[:8]) == [H, W, 6, 1, 1, 2, 0, 3] and op.p[1] is None and op.p[2] is None
    assert [op.p[3], op.p[4]] == [o["a"][1].data_ptr(), o["a"][2].data_ptr()]
    ops.run((op, keep))
    op, keep = ops.frame_cut(o["partials"], o["a"], o["b"], H=H, W=W, Tt=255 * H * W, Th=2 * H * W, R=16384, gap=255)
    assert list(op.i[:8]) == [H, W, 6, 0, 255 * H * W, 2 * H * W, 16384, 255]
    assert [op.p[k] for k in range(5)] == [t.data_ptr() for t in (o["partials"], o["a"][1], o["a"][2], o["b"][1], o["b"][2])]
    ops.run((op, keep))
    big = operands(2048, 2048)
    ops.run(ops.frame_cut_sig(big["x"], big["a"][0], big["b"][0], big["partials"], H=2048, W=2048))      # the largest size


def test_the_builders_refusals(dry_run):
    from live2diff_amd import ops
    H, W = 64, 72
    o = operands(H, W)
    x, P, a, b = o["x"], o["partials"], o["a"], o["b"]
    sig = lambda **kw: ops.frame_cut_sig(**{**dict(source=x, prev_thumb=a[0], thumb=b[0], partials=P, H=H, W=W), **kw})
    cutop = lambda **kw: ops.frame_cut(**{**dict(partials=P, prev=a, state=b, H=H, W=W, Tt=10, Th=10, R=768, gap=8), **kw})
    sig(), cutop()
    off = aligned(H * W // 64, torch.uint16, off=8).view(H // 8, W // 8)
    for kw, match in ((dict(H=60), "multiples of 8"), (dict(W=76), "multiples of 8"), (dict(H=0), "multiples of 8"),
                      (dict(H=2048, W=2056), "multiples of 8"), (dict(source=x.float()), "source"), (dict(source=x[:, :, ::2]), "source"),
                      (dict(source=None), "source"), (dict(prev_thumb=a[0].view(-1)), "prev_thumb"), (dict(prev_thumb=a[1]), "prev_thumb"),
                      (dict(thumb=None), "thumb"), (dict(thumb=off), "thumb"), (dict(prev_thumb=off), "prev_thumb"),
                      (dict(partials=P[:-1]), "partials"), (dict(partials=P.float()), "partials"), (dict(partials=P.view(-1)), "partials"),
                      (dict(thumb=a[0]), "overlap"), (dict(partials=aligned(o["nwg"] * 68, torch.int32).view(-1, 68), thumb=b[0]), None)):
        if match is None:
            sig(**kw)                                                       # (int32: the bits of uint32 counts)
            continue
        with pytest.raises(ValueError, match="frame_cut_sig.*" + match):
            sig(**kw)
    for kw, match in ((dict(H=60), "multiples of 8"), (dict(partials=P[:-1]), "partials"), (dict(prev=a[:2]), "prev"), (dict(state=None), "state"),
                      (dict(state=(b[0], b[1], b[2].float())), "state: rec"), (dict(state=(b[0], b[1][:32], b[2])), "state: hist"),
                      (dict(prev=(a[0].view(-1), a[1], a[2])), "prev: thumb"), (dict(Tt=-1), "Tt"), (dict(Tt=255 * H * W + 1), "Tt"), (dict(Tt=1.5), "Tt"),
                      (dict(Th=-1), "Th"), (dict(Th=2 * H * W + 1), "Th"), (dict(R=255), "R"), (dict(R=1), "R"), (dict(R=16385), "R"), (dict(R=-1), "R"),
                      (dict(R=True), "R"), (dict(gap=-1), "gap"), (dict(gap=256), "gap"), (dict(state=a), "overlap"),
                      (dict(state=(b[0], b[1], a[2])), "overlap"), (dict(state=(b[0], a[1], b[2])), "overlap")):
        with pytest.raises(ValueError, match="frame_cut: .*" + match):
            cutop(**kw)


def test_the_launchers_refuse_the_same(dry_run):
    from live2diff_amd import _lib, ops
    H, W = 64, 72
    o = operands(H, W)
    x, P, a, b = o["x"], o["partials"], o["a"], o["b"]

    def launch(kind, ptrs, i):
        ops.run(ops._record(kind, ptrs, i, keep=tuple(t for t in ptrs if torch.is_tensor(t))))

    SIG, CUT = _lib.OP_FRAME_CUT_SIG, _lib.OP_FRAME_CUT
    good_sig, good_i = (x, a[0], b[0], P), (H, W, 0, 2)
    good_cut, good_j = (P, a[1], a[2], b[1], b[2]), (H, W, 2, 0, 10, 10, 768, 8)
    launch(SIG, good_sig, good_i), launch(SIG, (x, None, b[0], P), (H, W, 1, 2)), launch(CUT, good_cut, good_j)
    launch(CUT, (P, None, None, b[1], b[2]), (H, W, 2, 1, 0, 0, 0, 0))
    off16 = aligned(H * W // 64, torch.uint16, off=8)
    off32 = aligned(64, torch.uint32, off=4)
    for ptrs, i, match in (
            (good_sig, (60, W, 0, 2), "multiples of 8"), (good_sig, (H, 76, 0, 2), "multiples of 8"), (good_sig, (0, W, 0, 2), "multiples of 8"),
            (good_sig, (2048, 2056, 0, 1056), "multiples of 8"), (good_sig, (H, W, 0, 1), "nwg = 1"), (good_sig, (H, W, 0, 3), "nwg = 3"),
            (good_sig, (H, W, 2, 2), "unknown flag"), ((None, a[0], b[0], P), good_i, "pointer 0 is null"), ((x, None, b[0], P), good_i, "pointer 1 is null"),
            ((x, a[0], None, P), good_i, "pointer 2 is null"), ((x, a[0], b[0], None), good_i, "pointer 3 is null"),
            ((x, off16, b[0], P), good_i, "pointer 1 is not 16-byte"), ((x, a[0], off16, P), good_i, "pointer 2 is not 16-byte"),
            ((x, a[0], a[0], P), good_i, "overlap"), ((x, a[0], x, P), good_i, "overlap"), ((x, a[0], b[0], x), good_i, "overlap"),
            ((x, a[0], P, P), good_i, "overlap"), ((x, P, b[0], P), good_i, "overlap")):
        with pytest.raises(_lib.L2DError, match="rc=-1: frame_cut_sig.*" + match):
            launch(SIG, ptrs, i)
    for ptrs, i, match in (
            (good_cut, (60, W, 2, 0, 10, 10, 768, 8), "multiples of 8"), (good_cut, (H, W, 1, 0, 10, 10, 768, 8), "nwg = 1"),
            (good_cut, (H, W, 2, 4, 10, 10, 768, 8), "unknown flag"), ((None,) + good_cut[1:], good_j, "pointer 0 is null"),
            ((P, None, a[2], b[1], b[2]), good_j, "pointer 1 is null"), ((P, a[1], None, b[1], b[2]), good_j, "pointer 2 is null"),
            ((P, a[1], a[2], None, b[2]), good_j, "pointer 3 is null"), ((P, a[1], a[2], b[1], None), good_j, "pointer 4 is null"),
            ((P, off32, a[2], b[1], b[2]), good_j, "pointer 1 is not 16-byte"), ((P, a[1], a[2], b[1], off32), good_j, "pointer 4 is not 16-byte"),
            (good_cut, (H, W, 2, 0, -1, 10, 768, 8), "Tt = -1"), (good_cut, (H, W, 2, 0, 255 * H * W + 1, 10, 768, 8), "Tt = "),
            (good_cut, (H, W, 2, 0, 10, -1, 768, 8), "Th = -1"), (good_cut, (H, W, 2, 0, 10, 2 * H * W + 1, 768, 8), "Th = "),
            (good_cut, (H, W, 2, 0, 10, 10, 255, 8), "R = 255"), (good_cut, (H, W, 2, 0, 10, 10, 16385, 8), "R = 16385"),
            (good_cut, (H, W, 2, 0, 10, 10, -1, 8), "R = -1"), (good_cut, (H, W, 2, 0, 10, 10, 768, 256), "gap = 256"),
            (good_cut, (H, W, 2, 0, 10, 10, 768, -1), "gap = -1"), ((P, a[1], a[2], a[1], b[2]), good_j, "overlap"),
            ((P, a[1], a[2], b[1], a[2]), good_j, "overlap"), ((P, a[1], a[2], P, b[2]), good_j, "overlap"), ((P, a[1], a[2], b[1], b[1]), good_j, "overlap")):
        with pytest.raises(_lib.L2DError, match="rc=-1: frame_cut\\(.*" + match):
            launch(CUT, ptrs, i)


# ----------------------------------------------------------------------------- the detector on the host route
def test_the_detector_on_cpu_tensors_is_cut_ref():
    from live2diff_amd import cut
    H, W = 64, 72
    frames = [f16(smooth(H, W, s)) for s in (1, 1, 2, 2, 2, 3)]
    det = cut.HipCutDetect(H, W, dict(gap=1), device="cpu")
    for k, x in enumerate(frames):
        assert det.measure(torch.from_numpy(x)[None]) == k and det.in_flight == k % 2 + 1
        if k % 2:
            got = det.collect()
            assert len(got) == 2 and det.in_flight == 0 and det.collect() == []
            assert np.array_equal(np.stack(got), cut.cut_ref(frames, gap=1)[k - 1:k + 1])
    det.restart()
    det.measure(torch.from_numpy(frames[5]))
    assert det.collect()[0].tolist() == [0, 0, 0, NEVER, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="expected a \\[3,64,72\\] frame"):
        det.measure(torch.zeros(3, 64, 64))
    det.configure(dict(thumb=1.0))
    assert det.params == cut.cut_params(H, W, dict(thumb=1.0)) and det.frames == 1


# ----------------------------------------------------------------------------- the pipeline on the mocks
def scene(seed, k, noise_seed=0):
    """k frames in [0, 1] of one scene: 8 x 8 cells of random colour, and a little noise that differs from frame to frame"""
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, 8, 8, generator=g), (M.H, M.W))[0]
    n = torch.Generator().manual_seed(1000 * seed + noise_seed)
    return [(base * 0.9 + 0.02 * torch.rand(3, M.H, M.W, generator=n)) for _ in range(k)]


def make_stream(monkeypatch, **kw):
    from live2diff_amd import pipeline_stream_animation_depth as P
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    pipe = M.MockPipe()
    pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    s = P.StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=T_INDEX, torch_dtype=torch.float32, width=M.W, height=M.H, **kw)
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = LoggingWarmup()
    s.kv_cache_list = M.make_caches(N)
    return s


def test_off_by_default_and_with_it_off_a_frame_launches_what_it_did(monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode

    from live2diff_amd import cut

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    syncs = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append(1))

    def frame(s, img):
        n = len(syncs)
        with Count() as c:
            s(img)
        return c.ops, len(syncs) - n

    off, on = make_stream(monkeypatch), make_stream(monkeypatch)
    assert off.cut_detector is None and len(off.cut_records) == 0
    on.cut_detector = cut.HipCutDetect(M.H, M.W, device="cpu")
    for s in (off, on):
        torch.manual_seed(123)
        s.prepare(M.frames(F, seed=7), "a prompt", seed=2)
    measured = []
    real = cut.HipCutDetect.measure
    monkeypatch.setattr(cut.HipCutDetect, "measure", lambda self, x: (measured.append(self), real(self, x))[1])
    imgs = scene(1, 2) + scene(2, 1)
    for k, img in enumerate(imgs):
        torch.manual_seed(5)
        a, sync_a = frame(off, img)
        assert len(measured) == k                                            # the stream without a detector never reaches one
        torch.manual_seed(5)
        b, sync_b = frame(on, img)
        assert len(measured) == k + 1 and measured[-1] is on.cut_detector
        assert sync_a == sync_b == 1                                         # no synchronisation is added
        # the plain frame's launches and copies, in their order, with the oracle's own tensor operations in ONE place between them
        # (the host route fetches the frame for numpy through `egress_ref`; the device route launches its two ops through the C ABI)
        first = next(j for j in range(len(b)) if j >= len(a) or a[j] != b[j])
        extra = len(b) - len(a)
        print(k, len(a), extra, b[first:first + extra])
        assert 0 < extra < 40 and b[:first] + b[first + extra:] == a
    assert len(off.cut_records) == 0 and [int(r[4]) for r in on.cut_records] == [0, 1, 2]
    assert [int(r[0]) for r in on.cut_records] == [0, 0, 1]
    want = cut.cut_ref([f16((2.0 * i - 1.0).numpy()) for i in imgs])
    assert np.array_equal(np.stack(list(on.cut_records)), want)
    # prepare restarts it: the next frame is INIT again
    on.prepare(M.frames(F, seed=7), "a prompt", seed=2)
    assert len(on.cut_records) == 0
    on(imgs[2])
    assert on.cut_records[0].tolist() == [0, 0, 0, NEVER, 0, 0, 0, 0]


# ----------------------------------------------------------------------------- the wrapper's policy on the mocks
def mock_wrapper(monkeypatch, **kw):
    from live2diff_amd import pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    mp = M.MockPipe()
    mp.unet, mp.vae, mp.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
    mp.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    w = Wrapper.from_components(mp, output_type="pt", dtype=torch.float32, device="cpu", num_inference_steps=50, t_index_list=T_INDEX,
                                width=M.W, height=M.H, **kw)
    s = w.stream
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = LoggingWarmup()
    w.entered = []
    step = s.predict_x0_batch
    s.predict_x0_batch = lambda x, d, **k: (w.entered.append((x.clone(), d.clone())), step(x, d, **k))[1]
    return w


def window_of(entered, n):
    """frames n .. n + F - 1 of what entered row 0, as `recent_window` forms them"""
    return tuple(torch.cat([e[j] for e in entered[n:n + F]], dim=2) for j in (0, 1))


def test_a_cut_rewarms_once_at_the_head_of_frame_n_plus_F_with_the_new_scene(monkeypatch):
    w = mock_wrapper(monkeypatch, keep_recent=True)
    assert w.cut_detect is None and w.auto_rewarm is False and w.stream.cut_detector is None
    w.set_cut_detect()
    w.set_auto_rewarm()
    assert w.cut_detect == dict(thumb=20.0, hist=0.35, ratio=3.0, gap=8) and w.auto_rewarm is True
    w.prepare(M.frames(F, seed=7), "a prompt")
    log = w.stream.unet_warmup.log
    k = 5
    frames = scene(1, k) + scene(2, F + 4)
    seen = []
    for i, img in enumerate(frames):
        w(img)
        seen.append((w.rewarms, w.auto_rewarms, len(log)))
        assert w.last_cut_record["n"] == i and w.last_cut_record["cut"] == (i == k)
    assert list(w.cuts) == [k]
    # nothing up to and including frame k + F - 1's call; frame k + F's call begins with the re-warm; none after it
    assert all(s == (0, 0, N) for s in seen[:k + F]) and all(s == (1, 1, 2 * N) for s in seen[k + F:]), seen
    x, d = window_of(w.entered, k)
    assert torch.equal(log[N]["x"], x) and torch.equal(log[N]["d"], d)       # the ring's frames k .. k + F - 1, and no frame of the old scene
    # ... and in front of frame k + F's own step: the window does not hold that frame
    assert not torch.equal(log[N]["x"][0, :, -1], w.entered[k + F][0][0, :, 0])
    # a new prepare starts everything again
    w.prepare(M.frames(F, seed=7), "a prompt")
    assert list(w.cuts) == [] and w.auto_rewarms == 0 and w.last_cut_record is None and w._rewarm_due is None
    w(frames[0])
    assert w.last_cut_record["n"] == 0 and w.last_cut_record["since"] == NEVER


def test_a_second_cut_moves_the_rewarm_and_a_manual_one_cancels_it(monkeypatch):
    w = mock_wrapper(monkeypatch, keep_recent=True)
    w.cut_detect = dict(gap=2)
    w.auto_rewarm = True
    w.prepare(M.frames(F, seed=7), "a prompt")
    log = w.stream.unet_warmup.log
    frames = scene(1, 3) + scene(2, 4) + scene(3, F + 3)                     # cuts at 3 and 7
    counts = []
    for img in frames:
        w(img)
        counts.append(w.auto_rewarms)
    assert list(w.cuts) == [3, 7]
    assert counts == [0] * (7 + F) + [1] * 3 and w.rewarms == 1              # once, at the head of frame 7 + F, not at 3 + F
    x, d = window_of(w.entered, 7)
    assert torch.equal(log[N]["x"], x) and torch.equal(log[N]["d"], d)
    # a manual re-warm between the cut and its due point cancels the automatic one
    w.prepare(M.frames(F, seed=7), "a prompt")
    del w.entered[:]
    for i, img in enumerate(scene(1, 3) + scene(2, F + 4)):
        w(img)
        if i == 5:
            assert w._rewarm_due == 3 + F
            w.rewarm()
            assert w._rewarm_due is None
    assert list(w.cuts) == [3] and w.rewarms == 1 and w.auto_rewarms == 0
    # switching it off drops a pending one as well
    w.prepare(M.frames(F, seed=7), "a prompt")
    for i, img in enumerate(scene(1, 3) + scene(2, F + 4)):
        w(img)
        if i == 5:
            w.set_auto_rewarm(False)
    assert list(w.cuts) == [3] and w.rewarms == 0 and w.auto_rewarm is False


def test_a_dropped_frame_keeps_n_and_the_ring_aligned(monkeypatch):
    class DropEveryThird:
        n = 0

        def __call__(self, x):
            self.n += 1
            return None if self.n % 3 == 0 else x

        def set_threshold(self, v):
            pass

        def set_max_skip_frame(self, v):
            pass

    w = mock_wrapper(monkeypatch, keep_recent=True)
    w.set_cut_detect()
    w.set_auto_rewarm(True)
    w.prepare(M.frames(F, seed=7), "a prompt")
    w.stream.similar_filter = DropEveryThird()
    w.stream.enable_similar_image_filter()
    monkeypatch.setattr("time.sleep", lambda s: None)
    frames = scene(1, 7) + scene(2, 16)                                     # calls 2, 5 (0-based) are dropped: call 7 enters as frame 5
    log = w.stream.unet_warmup.log
    fired = None
    for i, img in enumerate(frames):
        w(img)
        if fired is None and w.auto_rewarms:
            fired = len(w.entered)                                           # frames that had entered, the current call's included
    assert list(w.cuts) == [5] and w.stream._recent_seen == len(w.entered) == len(frames) - len(frames) // 3
    assert fired == 5 + F + 1 and w.auto_rewarms == 1                        # at the head of the call that entered frame 5 + F
    x, d = window_of(w.entered, 5)
    assert torch.equal(log[N]["x"], x) and torch.equal(log[N]["d"], d)


def test_the_wrappers_argument_checks(monkeypatch):
    plain = mock_wrapper(monkeypatch)
    plain.set_cut_detect(thumb=10)
    with pytest.raises(ValueError, match="keep_recent=True"):
        plain.set_auto_rewarm()
    assert plain.auto_rewarm is False
    plain.set_auto_rewarm(False)                                             # switching it off is always legal
    w = mock_wrapper(monkeypatch, keep_recent=True)
    with pytest.raises(ValueError, match="needs a cut detector"):
        w.set_auto_rewarm(True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="use True or False"):
            w.set_auto_rewarm(bad)
    with pytest.raises(ValueError, match="thumb="):
        w.set_cut_detect(thumb=300)
    with pytest.raises(ValueError, match="use a dict"):
        w.cut_detect = (20, 0.35)
    assert w.cut_detect is None and w.stream.cut_detector is None
    w.set_cut_detect(hist=0.5)
    det = w.stream.cut_detector
    w.set_auto_rewarm(True)
    w.set_cut_detect(hist=0.25)                                              # new thresholds, the same detector and state
    assert w.stream.cut_detector is det and det.settings["hist"] == 0.25 and w.auto_rewarm is True
    w.clear_cut_detect()
    assert w.cut_detect is None and w.stream.cut_detector is None and w.auto_rewarm is False
    w.cut_detect = None


def test_a_detector_switched_on_mid_stream_counts_frames_since_prepare(monkeypatch):
    """`n`, `cuts` and the due point are indices since `prepare` (ring indices), not since the detector's first frame"""
    w = mock_wrapper(monkeypatch, keep_recent=True)
    w.prepare(M.frames(F, seed=7), "a prompt")
    log = w.stream.unet_warmup.log
    frames = scene(1, 7) + scene(2, F + 3)                                   # the cut is frame 7 of the stream
    counts = []
    for i, img in enumerate(frames):
        if i == 4:                                                           # four frames in: what POST /cut-detect and /auto-rewarm do
            w.set_cut_detect()
            w.set_auto_rewarm()
        w(img)
        counts.append(w.auto_rewarms)
        if i >= 4:
            assert w.last_cut_record["n"] == i and w.last_cut_record["cut"] == (i == 7)
    assert w.stream.cut_detector.base == 4 and w.stream.cut_detector.frames == len(frames) - 4
    assert list(w.cuts) == [7] and w._rewarm_due is None
    assert counts == [0] * (7 + F) + [1] * 3 and w.rewarms == 1              # at the head of frame 7 + F, not of frame 8
    x, d = window_of(w.entered, 7)
    assert torch.equal(log[N]["x"], x) and torch.equal(log[N]["d"], d)       # the ring's frames 7 .. 7 + F - 1: nothing of the old scene
    # off and on again: a new detector, a new base, the same count
    w.clear_cut_detect()
    w(frames[-1])
    w.set_cut_detect()
    w.set_auto_rewarm()
    more = scene(2, 2, noise_seed=5) + scene(3, F)
    first = len(frames) + 1
    for img in more:
        w(img)
    assert w.stream.cut_detector.base == first and list(w.cuts) == [7, first + 2]
    assert w.auto_rewarms == 1 and w._rewarm_due == first + 2 + F            # due, and run at the head of the next call
    w(scene(3, 1, noise_seed=10)[0])                                         # ... now they have: the head of this call re-warms
    assert w.auto_rewarms == 2
    x, d = window_of(w.entered, first + 2)
    assert torch.equal(log[2 * N]["x"], x) and torch.equal(log[2 * N]["d"], d)
    # without a recent window the indices are still those since `prepare`
    p = mock_wrapper(monkeypatch)
    p.prepare(M.frames(F, seed=7), "a prompt")
    for i, img in enumerate(scene(1, 5) + scene(2, 2)):
        if i == 3:
            p.set_cut_detect()
        p(img)
    assert list(p.cuts) == [5] and p.last_cut_record["n"] == 6


def test_a_manual_rewarm_that_raises_leaves_the_pending_one(monkeypatch):
    w = mock_wrapper(monkeypatch, keep_recent=True)
    w.set_cut_detect()
    w.set_auto_rewarm()
    w.prepare(M.frames(F, seed=7), "a prompt")
    for img in scene(1, 2) + scene(2, 2):
        w(img)
    assert w._rewarm_due == 2 + F
    with pytest.raises(ValueError, match="use 'warmup', 'recent'"):
        w.rewarm("latest")
    with pytest.raises(ValueError, match="frames since prepare"):
        w.rewarm("recent")                                                   # four frames in: the window needs F
    assert w._rewarm_due == 2 + F and w.rewarms == 0


def test_records_nobody_collects_are_refused_not_hoarded():
    from live2diff_amd import cut
    det = cut.HipCutDetect(64, 64, device="cpu")
    x = torch.zeros(3, 64, 64)
    for _ in range(cut.MAX_IN_FLIGHT):
        det.measure(x)
    with pytest.raises(RuntimeError, match="same current stream"):
        det.measure(x)
    assert len(det.collect()) == cut.MAX_IN_FLIGHT
    det.measure(x)
