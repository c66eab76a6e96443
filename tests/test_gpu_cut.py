"""-m gpu: the cut detector.

  1. L2D_OP_FRAME_CUT_SIG and L2D_OP_FRAME_CUT bit for bit against `cut.signature_ref` / `cut.measure_ref`, INIT and compared, at
     8 x 8 (one block), 64 x 64 (one full tile), 72 x 136 (ragged in both axes), 8 x 520 (nine tiles in a row, the last ragged) and
     512 x 512 (the full size), every output pre-filled with 0xFF bytes and inside guard bands, on frames with values outside
     [-1, 1], +-0 and fp16 extremes;
  2. ten frames through `HipCutDetect` with a planted cut, a pan and a brightness step against `cut_ref`, collected frame by frame
     and all at once (one pinned slot per frame in flight);
  3. the wrapper on the tiny UNet of tests/test_gpu_style_switch.py (64 x 64, N = 2, F = 8): a stream whose input changes scene at
     frame k re-warms by itself, and every output frame and every sink equals a stream with the detector off and
     `rewarm("recent")` called by hand at the head of frame k + F -- in `__call__` mode and through push / pop with two frames in flight.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_style_switch import DEV, PROMPT, make_wrapper, same

pytestmark = pytest.mark.gpu
F = 8
NEVER = 1 << 30
GUARD = 64                                       # bytes in front of and behind every output
SIZES = [(8, 8), (64, 64), (72, 136), (8, 520), (512, 512)]


# ----------------------------------------------------------------------------- 1. the ops
def wild_frame(H, W, seed):
    """fp16 [3,H,W]: mostly within [-1.5, 1.5], with +-0, the fp16 extremes, subnormals and the clamp's corners sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(3, H, W, generator=g) * 3.0 - 1.5).to(torch.float16)
    special = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 6e-8, -6e-8, 1.0, -1.0, 1.0009765625, -1.0009765625, 0.00390625, 2.0, -2.0],
                           dtype=torch.float16)
    where = torch.randint(0, x.numel(), (max(8, x.numel() // 16),), generator=g)
    x.view(-1)[where] = special[torch.randint(0, len(special), where.shape, generator=g)]
    return x


def halves(H, W, flip):
    """the left half black and the right half white, or with `flip` the other way round: Dt is 255 per pixel, Dh is 0"""
    x = torch.full((3, H, W), -1.0, dtype=torch.float16)
    x[:, :, W // 2:] = 1.0
    return -x if flip else x


class Guarded:
    """a 16-byte aligned device tensor inside a buffer of 0xFF bytes"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0

    def refill(self):
        self.buf.fill_(0xFF)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == 0xFF).all()) and bool((self.buf[GUARD + self.n:] == 0xFF).all())


def tile_partials(x, prev_thumb):
    """the uint32 [nwg,68] partials of the fp16 frame `x`, per 64 x 64 tile, from the oracle's pieces"""
    from live2diff_amd import cut
    from live2diff_amd.matte import luma
    from live2diff_amd.steady import source_bytes
    Y = luma(source_bytes(x).transpose(1, 2, 0))
    thumb, _ = cut.signature_ref(x)
    H, W = Y.shape
    out = []
    for ty in range(0, H, 64):
        for tx in range(0, W, 64):
            hist = np.bincount((Y[ty:ty + 64, tx:tx + 64] >> 2).reshape(-1), minlength=64)
            share = 0
            if prev_thumb is not None:
                a, b = thumb[ty // 8:ty // 8 + 8, tx // 8:tx // 8 + 8].astype(np.int64), prev_thumb[ty // 8:ty // 8 + 8, tx // 8:tx // 8 + 8].astype(np.int64)
                share = int(np.abs(a - b).sum())
            out.append(list(hist) + [share, 0, 0, 0])
    return np.array(out, dtype=np.uint32)


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_both_ops_bit_for_bit_behind_guard_bands(H, W):
    from live2diff_amd import cut, ops
    nwg = ops.frame_cut_tiles(H, W)
    # two sequences, each begun by INIT: wild frames; then the halves, swapped (the level's first value, 256 * 255 H W), and a wild one
    # against that level
    frames = [wild_frame(H, W, 1), wild_frame(H, W, 2), None, halves(H, W, False), halves(H, W, True), wild_frame(H, W, 3)]
    params = cut.cut_params(H, W)
    states = [(Guarded((H // 8, W // 8), torch.uint16), Guarded((64,), torch.uint32), Guarded((8,), torch.int32)) for _ in range(2)]
    partials = Guarded((nwg, 68), torch.uint32)
    prev_sig = prev_rec = None
    cur = 0
    for k, x in enumerate(frames):
        if x is None:
            prev_sig = prev_rec = None
            continue
        xd = x.to(DEV)
        src = xd.clone()
        prev, nxt = states[cur], states[1 - cur]
        for gd in nxt + (partials,):
            gd.refill()                                                      # nothing is zeroed beforehand: every entry must be written
        kept = [gd.t.clone() for gd in prev]
        init = prev_sig is None
        ops.run(ops.frame_cut_sig(xd, None if init else prev[0].t, nxt[0].t, partials.t, H=H, W=W))
        ops.run(ops.frame_cut(partials.t, None if init else tuple(gd.t for gd in prev), tuple(gd.t for gd in nxt), H=H, W=W,
                              Tt=params[0], Th=params[1], R=params[2], gap=params[3]))
        torch.cuda.synchronize()
        sig = cut.signature_ref(x.numpy())
        rec = cut.measure_ref(sig, prev_sig, prev_rec, params)
        got_thumb, got_hist, got_rec = (gd.t.cpu().numpy() for gd in nxt)
        got_part = partials.t.cpu().numpy()
        want_part = tile_partials(x.numpy(), None if init else prev_sig[0])
        print(f"{H}x{W} frame {k}: record {got_rec.tolist()} want {rec.tolist()}; thumb {int((got_thumb != sig[0]).sum())} hist "
              f"{int((got_hist != sig[1]).sum())} partials {int((got_part != want_part).sum())} entries differ")
        assert np.array_equal(got_thumb, sig[0]) and np.array_equal(got_hist, sig[1])
        assert np.array_equal(got_part, want_part)
        assert np.array_equal(got_rec, rec)
        assert all(gd.guards_intact() for gd in states[0] + states[1] + (partials,))
        assert same(xd, src) and all(same(gd.t, t) for gd, t in zip(prev, kept))      # what a launch reads is as it was
        prev_sig, prev_rec, cur = sig, rec, 1 - cur
        if k == 4 and W % 16 == 0:                                              # the swapped halves: all thumbnail, no histogram
            assert rec.tolist()[:4] == [0, 255 * H * W, 0, NEVER] and cut.level_of(rec) == 256 * 255 * H * W
            assert (rec[6] > 0) == (H * W == 512 * 512)                          # the level needs its upper half at the full size


# ----------------------------------------------------------------------------- 2. a sequence through HipCutDetect
def sequence(H, W):
    """ten frames: a scene, its pan by 2 pixels a frame, a cut, the new scene, a +12 level step, the scene again"""
    def patches(seed, w):
        g = torch.Generator().manual_seed(seed)
        return torch.nn.functional.interpolate(torch.rand(1, 3, 5, 9, generator=g) * 1.6 - 0.8, (H, w))[0]             # (flat patches)
    a, b = patches(1, W + 32), patches(2, W)
    noise = lambda k: 0.01 * torch.rand(3, H, W, generator=torch.Generator().manual_seed(100 + k))
    frames = [a[:, :, 2 * k:2 * k + W] for k in range(4)] + [b + noise(k) for k in range(3)] + [b + 24.0 / 255.0 + noise(7)] + [b + noise(k) for k in (8, 9)]
    return [f.to(torch.float16).contiguous() for f in frames]


def test_ten_frames_through_the_detector_equal_cut_ref():
    from live2diff_amd import cut
    H, W = 72, 136
    frames = sequence(H, W)
    want = cut.cut_ref([f.numpy() for f in frames], gap=2)
    assert [int(r[0]) for r in want] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0], want[:, :4].tolist()      # the cut, and neither the pan nor the step
    dev = [f.to(DEV) for f in frames]
    det = cut.HipCutDetect(H, W, dict(gap=2), device=DEV)
    for k, x in enumerate(dev):
        assert det.measure(x[None]) == k
        torch.cuda.synchronize()
        got = det.collect()
        assert len(got) == 1 and np.array_equal(got[0], want[k]), (k, got[0].tolist(), want[k].tolist())
    assert len(det._slots) == 1                                                  # one frame in flight: one slot, used again
    # all ten measured before anything is collected: a slot per frame in flight, nothing overwritten
    det.restart()
    for x in dev:
        det.measure(x)
    assert det.in_flight == 10 and len(det._slots) == 10
    other = torch.cuda.Stream(device=DEV)
    assert det.collect(other) == [] and det.in_flight == 10                      # nothing was measured on that stream
    torch.cuda.current_stream().synchronize()
    got = det.collect(torch.cuda.current_stream())
    assert np.array_equal(np.stack(got), want) and det.in_flight == 0
    # a restart makes the next frame INIT again, whatever the states hold
    det.restart()
    det.measure(dev[5])
    det.measure(dev[4])
    torch.cuda.synchronize()
    assert np.array_equal(np.stack(det.collect()), cut.cut_ref([frames[5].numpy(), frames[4].numpy()], gap=2))


# ----------------------------------------------------------------------------- 3. the wrapper
K = 3                                            # the scene changes at frame K


def scene_u8(seed, n, Hs=96, Ws=128):
    """n uint8 [Hs,Ws,3] frames of one scene: flat patches of random colour, and noise of +-4 levels that differs per frame"""
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, 4, 4, generator=g) * 200.0 + 20.0, (Hs, Ws))[0].permute(1, 2, 0)
    return [(base + torch.randint(-4, 5, (Hs, Ws, 3), generator=g)).clamp(0, 255).to(torch.uint8).numpy() for _ in range(n)]


def data():
    from test_gpu_wrapper import u8_frames
    return u8_frames(8, 96, 128, seed=1), scene_u8(1, K) + scene_u8(2, F + 3)


def sinks_of(w):
    return [c[:, :, :, :F].clone() for c in w.stream.kv_cache_list]


@functools.lru_cache(maxsize=None)
def by_hand():
    """the control: no detector, `rewarm("recent")` by hand at the head of frame K + F"""
    warm, frames = data()
    w = make_wrapper(keep_recent=True)
    assert w.stream.cut_detector is None
    w.prepare(warm, PROMPT)
    out = []
    for i, f in enumerate(frames):
        if i == K + F:
            w.rewarm("recent")
        out.append(w(f))
    torch.cuda.synchronize()
    assert w.rewarms == 1 and w.auto_rewarms == 0 and list(w.cuts) == []
    return dict(out=out, sinks=sinks_of(w))


def test_a_scene_change_rewarms_by_itself_and_equals_the_rewarm_by_hand():
    want = by_hand()
    warm, frames = data()
    w = make_wrapper(keep_recent=True)
    w.set_cut_detect()
    w.set_auto_rewarm()
    w.prepare(warm, PROMPT)
    out, counts = [], []
    for f in frames:
        out.append(w(f))
        counts.append(w.auto_rewarms)
    torch.cuda.synchronize()
    print("cuts", list(w.cuts), "last record", w.last_cut_record)
    assert list(w.cuts) == [K] and w.auto_rewarms == 1 and w.rewarms == 1
    assert counts == [0] * (K + F) + [1] * (len(frames) - K - F)
    assert w.last_cut_record["n"] == len(frames) - 1 and w.stream.cut_detector.in_flight == 0
    for i, (a, b) in enumerate(zip(out, want["out"])):
        assert np.array_equal(a, b), f"frame {i} differs from the stream re-warmed by hand"
    for j, (a, b) in enumerate(zip(sinks_of(w), want["sinks"])):
        assert float(a.float().abs().max()) > 0 and same(a, b), f"layer {j}: the sinks differ"
    # ... and the re-warm mattered: a stream that never re-warms gives other frames from K + F on
    plain = make_wrapper()
    plain.prepare(warm, PROMPT)
    rest = [plain(f) for f in frames]
    assert all(np.array_equal(a, b) for a, b in zip(rest[:K + F], out[:K + F])), "the detector changed a frame by itself"
    assert not np.array_equal(rest[K + F], out[K + F])


def test_push_pop_with_two_frames_in_flight_rewarms_at_the_same_frame():
    want = by_hand()
    warm, frames = data()
    w = make_wrapper(keep_recent=True, frame_pipelining=True)
    w.set_cut_detect()
    w.set_auto_rewarm()
    w.prepare(warm, PROMPT)
    out, counts = [], []
    w.push(frames[0])
    w.push(frames[1])
    for i in range(len(frames)):
        assert len(w.stream._pending) == min(2, len(frames) - i)
        out.append(w.pop())
        counts.append(w.auto_rewarms)
        if i + 2 < len(frames):
            w.push(frames[i + 2])
    torch.cuda.synchronize()
    assert list(w.cuts) == [K] and w.auto_rewarms == 1 and w.rewarms == 1
    assert counts == [0] * (K + F) + [1] * (len(frames) - K - F)
    assert w.stream.cut_detector.in_flight == 0 and w.last_cut_record["n"] == len(frames) - 1
    for i, (a, b) in enumerate(zip(out, want["out"])):
        assert np.array_equal(a, b), f"push / pop frame {i} differs from __call__ mode re-warmed by hand"
    for j, (a, b) in enumerate(zip(sinks_of(w), want["sinks"])):
        assert same(a, b), f"layer {j}: the sinks differ"


def test_a_detector_switched_on_mid_stream_rewarms_at_the_same_frame():
    """`set_cut_detect` between two frames, two frames in: `cuts` and the due point still count frames since `prepare`"""
    want = by_hand()
    warm, frames = data()
    w = make_wrapper(keep_recent=True)
    w.prepare(warm, PROMPT)
    out, counts = [], []
    for i, f in enumerate(frames):
        if i == K - 1:
            w.set_cut_detect()
            w.set_auto_rewarm()
        out.append(w(f))
        counts.append(w.auto_rewarms)
    torch.cuda.synchronize()
    assert w.stream.cut_detector.base == K - 1 and list(w.cuts) == [K] and w.last_cut_record["n"] == len(frames) - 1
    assert counts == [0] * (K + F) + [1] * (len(frames) - K - F) and w.rewarms == 1
    for i, (a, b) in enumerate(zip(out, want["out"])):
        assert np.array_equal(a, b), f"frame {i} differs from the stream re-warmed by hand"
    for j, (a, b) in enumerate(zip(sinks_of(w), want["sinks"])):
        assert same(a, b), f"layer {j}: the sinks differ"
