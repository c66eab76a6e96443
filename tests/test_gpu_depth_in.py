"""-m gpu: the depth input on the device (csrc/depth_in.hip, live2diff_amd/depth_io.py).  Ops 52 and 53
against the numpy oracle with `torch.equal` -- the resampled plane R, the partials and the fp16 map, each NaN-poisoned before
every launch --, `HipDepthIngest`'s buffers, and the wrapper with small synthetic weights."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

OUTPUTS = [(40, 72), (64, 64)]        # 40 x 72: partial tiles on both axes whatever the tile between 8 and 32
SOURCES = [(40, 72), (30, 54), (97, 173), (320, 576), (64, 64), (512, 512)]
# (identity at 40 x 72 | up-scale | odd, non-integer scale, left > 0 at 64 x 64 | exactly scale 8 at 40 x 72: 17 taps |
#  one partial per tile row at 64 x 64 | 8 partials per frame, 64 for the batch of 8)
SETTINGS = [dict(kind="distance", range=None), dict(kind="inverse", range=None), dict(kind="distance", range=(0.8, 3.0)),
            dict(kind="distance", range=(1.0, float("inf"))), dict(kind="inverse", range=(0.25, 1.5))]


def smooth(seed, B, Hd, Wd, lo=0.5, hi=5.0):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:Hd, 0:Wd].astype(np.float64)
    out = []
    for b in range(B):
        a = np.sin(x / Wd * (3 + b) + g.uniform(0, 6)) * np.cos(y / Hd * (2 + b) + g.uniform(0, 6)) + 0.1 * g.standard_normal((Hd, Wd))
        a = (a - a.min()) / (a.max() - a.min())
        out.append(lo + (hi - lo) * a)
    return np.stack(out).astype(np.float32)


def source(dtype, B, Hd, Wd, seed=0):
    """a frame with the hole patterns of the CPU file: isolated invalid samples, one hole larger than any footprint (a quarter of
    the frame), one on the frame's nearest point; fp32 frames carry NaN, inf, 0 and negative samples"""
    z = smooth(100 + seed, B, Hd, Wd)
    g = np.random.default_rng(seed)
    iso = g.random((B, Hd, Wd)) < 0.02
    near = np.unravel_index(np.argmin(z[0]), z[0].shape)
    if dtype == "uint16":
        z = np.round(z * 1000.0).astype(np.uint16)
        z[iso] = 0
    else:
        z[iso] = g.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], np.float32), int(iso.sum()))
    z[:, Hd // 4:Hd // 4 + Hd // 2, Wd // 8:Wd // 8 + Wd // 2] = 0
    z[0, max(near[0] - 1, 0):near[0] + 2, max(near[1] - 1, 0):near[1] + 2] = 0
    return z


def to_dev(z):
    return torch.from_numpy(z.view(np.int16) if z.dtype == np.uint16 else z).to(DEV)


def launch(z, H, W, kind="distance", invalid=0, range=None):
    """ops 52 + 53 on poisoned buffers -> (R, partials, out) as numpy"""
    from live2diff_amd import _lib, ops
    from live2diff_amd import depth_io as D
    z = z if z.ndim == 3 else z[None]
    B, Hd, Wd = z.shape
    (nh, nw, top, left), ymin, wy, xmin, wx = D.tables(Hd, Wd, H, W)
    src = to_dev(z)
    R = torch.full((B, H, W), float("nan"), device=DEV)
    part = torch.full((B * ops.depth_tiles(H, W), 3), float("nan"), device=DEV)
    out = torch.full((B, 3, H, W), float("nan"), dtype=torch.float16, device=DEV)
    tabs = [t.to(DEV) for t in (xmin, wx, ymin, wy)]
    pl = _lib.OpList()
    op, keep = ops.depth_ingest(src, R, part, *tabs, B=B, Hd=Hd, Wd=Wd, H=H, W=W, nh=nh, nw=nw, top=top, left=left,
                                distance=kind == "distance", invalid=invalid)
    pl.append(op, *keep)
    op, keep = ops.depth_normalize(R, part, out, B=B, H=H, W=W, fixed=D.fixed_range(kind, range))
    pl.append(op, *keep)
    pl.run()
    torch.cuda.synchronize()
    return R.cpu().numpy(), part.cpu().numpy(), out.cpu().numpy()


def check(z, H, W, what, **s):
    from live2diff_amd import depth_io as D
    R, part, out = launch(z, H, W, **s)
    want_R = D.resample_ref(z, H, W, s.get("kind", "distance"), s.get("invalid", 0))
    want = D.depth_ref(z, H, W, **s)
    nR, nP, nO = int((R != want_R).sum()), int((part != D.partials_ref(want_R)).sum()), int((out != want).sum())
    print(f"{what} {s}: R {nR} partials {nP} out {nO} differing elements; holes {int((want_R < 0).sum())} of {want_R.size}")
    assert not np.isnan(R).any() and not np.isnan(part).any() and not np.isnan(out.astype(np.float32)).any()
    assert nR == 0 and nP == 0 and nO == 0, what
    return want_R, want


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("out", OUTPUTS, ids=lambda s: f"to{s[0]}x{s[1]}")
def test_kernels_equal_the_oracle(out, src, dtype):
    """every source of the table at every output its geometry allows (a window that does not lie inside the resized image is a
    ValueError by the same rule as the colour ingest's), both dtypes, both kinds, auto and fixed ranges"""
    from live2diff_amd import depth_io as D
    (H, W), (Hd, Wd) = out, src
    try:
        D.tables(Hd, Wd, H, W)
    except ValueError as e:
        assert "does not lie inside" in str(e) and (out, src) in {((40, 72), (97, 173)), ((40, 72), (64, 64)), ((40, 72), (512, 512))}
        with pytest.raises(ValueError, match="depth: .*does not lie inside"):
            launch(source(dtype, 1, Hd, Wd), H, W)
        return
    z = source(dtype, 1, Hd, Wd)
    for s in SETTINGS:
        scale = 1000.0 if dtype == "uint16" and s["range"] else 1.0                    # (uint16 frames hold millimetres)
        s = dict(s, range=tuple(v * scale for v in s["range"])) if s["range"] else s
        R, dn = check(z, H, W, f"{Hd}x{Wd}->{H}x{W} {dtype}", **s)
        assert (R < 0).any() and (R >= 0).any() and dn.max() > -1                # holes and values both, and a map that is not empty
    check(z, H, W, "every value counts", kind="inverse", invalid=None)
    if dtype == "uint16":
        check(z, H, W, "another invalid value", kind="distance", invalid=int(z[0, 0, 0]))


def test_scale_8_has_17_taps_and_many_partials():
    from live2diff_amd import depth_io as D
    from live2diff_amd import ops
    _, ymin, wy, xmin, wx = D.tables(320, 576, 40, 72)
    assert max(int((wy > 0).sum(1).max()), int((wx > 0).sum(1).max())) >= 15 and wy.shape[1] <= ops.DEPTH_MAX_TAPS
    with pytest.raises(ValueError, match="down-scale above 8"):
        launch(np.ones((1, 328, 591), np.uint16), 40, 72)
    assert ops.depth_tiles(64, 64) == 8 and ops.depth_tiles(40, 72) == 9


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_hole_patterns(dtype):
    Hd, Wd, H, W = 97, 173, 64, 64
    one = (lambda v: np.full((1, Hd, Wd), v, np.uint16)) if dtype == "uint16" else (lambda v: np.full((1, Hd, Wd), v / 1000.0, np.float32))
    R, dn = check(one(0), H, W, "all invalid")
    assert (R == -1).all() and (dn == -1).all()
    R, dn = check(one(1500), H, W, "flat")
    assert (R >= 0).all() and (dn == -1).all()
    if dtype == "float32":
        for v in (np.nan, np.inf, -2.0):
            R, dn = check(np.full((1, Hd, Wd), v, np.float32), H, W, f"all {v}")
            assert (R == -1).all() and (dn == -1).all()
    z = np.round(smooth(5, 1, Hd, Wd) * 1000).astype(np.uint16) if dtype == "uint16" else smooth(5, 1, Hd, Wd)
    z[0, 50, 90] = 0                                                         # an isolated hole: every pixel keeps a value
    R, dn = check(z, H, W, "isolated hole")
    assert (R >= 0).all()
    z[0, 30:60, 70:110] = 0                                                  # a hole larger than the footprint
    R, dn = check(z, H, W, "large hole")
    assert (R[0, 24:36, 24:38] == -1).all() and (dn[0, :, 24:36, 24:38] == -1).all() and dn.max() == 1
    z[0, 10:13, 85:88] = 300 if dtype == "uint16" else 0.3                   # the frame's nearest point, inside the window ...
    before, _ = check(z, H, W, "nearest point in")
    z[0, 8:15, 83:90] = 0                                                    # ... under a hole
    after, dn = check(z, H, W, "nearest point out")
    assert after.max() < before.max() and dn.max() == 1                      # the range moved to the next one


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_a_batch_of_8_is_normalised_jointly(dtype):
    H = W = 64
    z = np.stack([smooth(9 + b, 1, 97, 173, 1.0 + 0.3 * b, 2.0 + 0.3 * b)[0] for b in range(8)])
    z[:, 10:13, 20:24] = 0
    if dtype == "uint16":
        z = np.round(z * 1000).astype(np.uint16)
    _, joint = check(z, H, W, "batch of 8")
    singles = np.concatenate([launch(z[b], H, W)[2] for b in range(8)])
    assert not np.array_equal(joint, singles) and joint[0].max() == 1 and joint[7].min() == -1 and joint[7].max() < 1
    assert all(singles[b].max() == 1 for b in range(8))
    check(z, H, W, "batch of 8, fixed", range=(1000.0, 4000.0) if dtype == "uint16" else (1.0, 4.0))
    check(np.stack([source(dtype, 1, 512, 512, seed=b)[0] for b in range(8)]), H, W, "batch of 8, 64 partials")


@pytest.mark.parametrize("B,H,W,npart", [(1, 272, 520, 289), (3, 144, 520, 459)])
def test_more_partials_than_one_block_has_lanes(B, H, W, npart):
    """Op 53 reduces the partials with 256 lanes striding over them, shuffles inside each of four waves, then four LDS records.
    At 64 x 64 a frame has 8 tiles, so only lanes of the first wave ever hold one.  Here there are more than 256, and no multiple
    of 256: the stride loop runs a second, partial turn.  The frames are nearly flat (values 0.999 .. 1.001 of 2.0) with the
    call's minimum and its maximum planted, each alone, in one tile of every kind -- below 64 (the first wave), 64 .. 255 (the
    other waves' LDS records) and from 256 on (the second turn) --, so a partial dropped anywhere moves the range and with it
    every pixel of the map."""
    from live2diff_amd import ops
    assert B * ops.depth_tiles(H, W) == npart and npart > 256 and npart % 256
    tw = (W + ops.DEPTH_TILE_W - 1) // ops.DEPTH_TILE_W
    per = ops.depth_tiles(H, W)
    base = (2.0 * (1.0 + 0.001 * np.random.default_rng(3).uniform(-1, 1, (B, H, W)))).astype(np.float32)
    kinds = {"first wave": lambda t: t < 64, "other waves": lambda t: 64 <= t < 256, "second turn": lambda t: t >= 256}
    tiles = {k: [t for t in range(npart) if f(t)] for k, f in kinds.items()}
    for lo_kind, hi_kind in (("second turn", "other waves"), ("other waves", "second turn"), ("first wave", "second turn"),
                             ("second turn", "first wave"), ("second turn", "second turn")):
        z = base.copy()
        t_lo, t_hi = tiles[lo_kind][len(tiles[lo_kind]) // 2], tiles[hi_kind][-1 if hi_kind != lo_kind else 0]
        assert t_lo != t_hi
        for t, v in ((t_lo, 1.0), (t_hi, 4.0)):
            b, ty, tx = t // per, (t % per) // tw, t % tw
            z[b, ty * ops.DEPTH_TILE_H + 3, tx * ops.DEPTH_TILE_W + 5] = v
        R, dn = check(z, H, W, f"min in tile {t_lo} ({lo_kind}), max in tile {t_hi} ({hi_kind})", kind="inverse", invalid=None)
        assert R.min() == 1.0 and R.max() == 4.0 and dn.min() == -1 and dn.max() == 1
        assert (np.abs(dn.astype(np.float32) + 1.0 / 3.0) < 0.01).sum() >= dn.size - 6      # everything else sits at (2 - 1) / 3


def test_a_narrow_fixed_range_on_the_device():
    z = np.full((1, 40, 72), 2.0, np.float32)
    z[0, :20] = 2.00002
    _, dn = check(z, 40, 72, "inside the flat margin, auto", kind="inverse", invalid=None)
    assert (dn == -1).all()
    _, dn = check(z, 40, 72, "inside the flat margin, fixed", kind="inverse", invalid=None, range=(2.000005, 2.00001))
    assert (dn[0, :, :20] == 1).all() and (dn[0, :, 20:] == -1).all()


# ----------------------------------------------------------------------------- HipDepthIngest
def test_ingest_buffers():
    from live2diff_amd import depth_io as D
    H, W, Hd, Wd = 64, 64, 97, 173
    ing = D.HipDepthIngest(H, W, device=DEV)
    z = [source("uint16", 1, Hd, Wd, seed=s)[0] for s in range(4)]
    want = [torch.from_numpy(D.depth_ref(f, H, W)) for f in z]
    a = ing.ingest(z[0])
    b = ing.ingest(z[1])
    assert a.data_ptr() != b.data_ptr() and a.shape == (1, 3, H, W) and a.dtype == torch.float16      # two frames, two slots
    assert torch.equal(a.cpu(), want[0]) and torch.equal(b.cpu(), want[1])   # the first slot's view is intact behind the next ingest
    c = ing.ingest(z[2])
    assert c.data_ptr() == a.data_ptr() and torch.equal(c.cpu(), want[2]) and torch.equal(b.cpu(), want[1])
    built = ing.plans_built
    assert built == 2                                                        # one kept plan per slot
    for f, w_ in zip(z, want):
        assert torch.equal(ing.ingest(f).cpu(), w_)
    assert ing.plans_built == built
    # settings change between two frames; torch and float32 frames
    got = ing.ingest(torch.from_numpy(z[0].astype(np.float32)), kind="inverse", invalid=None, range=(500.0, 4000.0))
    assert torch.equal(got.cpu(), torch.from_numpy(D.depth_ref(z[0].astype(np.float32), H, W, kind="inverse", invalid=None, range=(500.0, 4000.0))))
    # a device tensor is read in place: no copy, and the same pointer met twice keeps its plans
    dev = to_dev(z[3])                                                       # (int16: the bits of the uint16 samples)
    before = dev.clone()
    built = ing.plans_built
    outs = [ing.ingest(dev) for _ in range(2)]       # a pointer met for the first time fills its records; met again, its plan is kept
    assert ing.plans_built == built + 2 and all(torch.equal(o.cpu(), want[3]) for o in outs)
    outs = [ing.ingest(dev) for _ in range(2)]                               # the first slot's plan is made once more and kept ...
    assert ing.plans_built == built + 3
    outs = [ing.ingest(dev) for _ in range(4)]                               # ... and from here both slots reuse theirs
    assert ing.plans_built == built + 3 and all(torch.equal(o.cpu(), want[3]) for o in outs)
    assert len(ing._device_plans) == 2 and torch.equal(dev, before)
    plan = next(iter(ing._device_plans.values()))
    assert plan[0].p[0] == dev.data_ptr()                                    # the record points at the caller's tensor itself
    dev32 = torch.from_numpy(z[3].astype(np.float32)).to(DEV)
    assert torch.equal(ing.ingest(dev32).cpu(), torch.from_numpy(D.depth_ref(z[3].astype(np.float32), H, W)))
    # a batch: fresh tensors, normalised jointly; another source size replans
    zb = np.stack(z)
    got = ing.ingest(zb)
    assert got.shape == (4, 3, H, W) and torch.equal(got.cpu(), torch.from_numpy(D.depth_ref(zb, H, W)))
    assert got.data_ptr() not in (a.data_ptr(), b.data_ptr())
    small = source("uint16", 1, 30, 54)[0]
    assert torch.equal(ing.ingest(small).cpu(), torch.from_numpy(D.depth_ref(small, H, W)))
    ev = torch.cuda.Event()
    ev.record()
    ing.release(ing.last_view, ev)
    assert torch.equal(ing.ingest(small).cpu(), ing.ingest(small).cpu())
    with pytest.raises(ValueError, match="release"):
        ing.release(got, ev)
    with pytest.raises(ValueError, match="depth: expected uint16 or float32"):
        ing.ingest(torch.zeros(8, 8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="range="):
        ing.ingest(small, range=(2.0, 1.0))


# ----------------------------------------------------------------------------- the wrapper with synthetic weights
class Counting:
    """a depth detector that counts its calls"""

    def __init__(self, inner):
        self.inner, self.calls, self.dtype = inner, 0, inner.dtype

    def __call__(self, x):
        self.calls += 1
        return self.inner(x)

    def __getattr__(self, name):
        return getattr(self.inner, name)


def record_depth_latents(w):
    """wrap `encode_depth` of a wrapper's stream: every depth latent it returns is kept (a copy)"""
    log, inner = [], w.stream.encode_depth

    def encode_depth(*a, **kw):
        out = inner(*a, **kw)
        log.append(out.clone())
        return out
    w.stream.encode_depth = encode_depth
    return log


def test_wrapper_with_external_depth():
    """Frames with and without `depth=` in one stream.  The stream carries history (the KV cache, the latent rows of the stream
    batch), so an output behind a frame with external depth legitimately differs from a stream that never saw one; what belongs
    to a frame alone is its depth latent, and the outputs in front of the first `depth=`: those are compared bit for bit with a
    wrapper that never saw a `depth=`."""
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd import depth_io as D
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.matte import composite_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(6, 96, 128, seed=2)
    depths = [source("uint16", 1, 120, 160, seed=10 + i)[0] for i in range(6)]
    warm_d = np.stack([source("uint16", 1, 120, 160, seed=20 + i)[0] for i in range(8)])
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(pipe=None, warm_depths=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        pipe = pipe or parts.pipe()
        if getattr(pipe, "depth_model", None) is not None:
            pipe.depth_model = Counting(pipe.depth_model)
        w = Wrapper.from_components(pipe, output_type="u8", seed=SEED, device=DEV, **kw, **more)
        w.prepare(warm, PROMPT, warmup_depths=warm_depths)
        return w

    # never a depth= | alternating | every frame
    plain, mixed, every = wrapper(), wrapper(), wrapper()
    logs = [record_depth_latents(w) for w in (plain, mixed, every)]
    with_depth = (1, 3, 4)
    outs = [[], [], []]
    for i, f in enumerate(frames):
        outs[0].append(plain(f))
        calls = mixed.stream.depth_detector.calls
        outs[1].append(mixed(f, depth=depths[i]) if i in with_depth else mixed(f))
        assert mixed.stream.depth_detector.calls == calls + (0 if i in with_depth else 1)      # depth= never calls the detector
        outs[2].append(every(f, depth=depths[i]))
        if i in with_depth:
            # its depth latent is vae.encode of the kernel's map (an ingest of its own; the map is the oracle's)
            dn = D.HipDepthIngest(H, W, device=DEV).ingest(depths[i])
            assert torch.equal(dn.cpu(), torch.from_numpy(D.depth_ref(depths[i], H, W)))
            vae = mixed.stream.vae
            want = P.retrieve_latents(vae.encode(dn.to(vae.dtype)), None) * vae.config.scaling_factor
            assert torch.equal(logs[1][i], want) and torch.equal(logs[2][i], want)
    assert every.stream.depth_detector.calls == 1                            # (prepare's, without warmup_depths)
    assert np.array_equal(outs[0][0], outs[1][0])                            # in front of the first depth=
    for i in range(len(frames)):
        if i not in with_depth:
            assert torch.equal(logs[0][i], logs[1][i]), f"frame {i} without depth: the detector path is untouched"
        else:
            assert not torch.equal(logs[0][i], logs[1][i])
    assert all(o.shape == (H, W, 3) and o.dtype == np.uint8 and o.std() > 0 for o in outs[1] + outs[2])
    assert not np.array_equal(outs[0][2], outs[1][2])                        # (the conditioning does reach the picture)

    # push / pop with depth equals __call__ with depth, bit for bit
    wp = wrapper(frame_pipelining=True)
    out = []
    wp.push(frames[0], depth=depths[0])
    for i in range(len(frames)):
        if i + 1 < len(frames):
            wp.push(frames[i + 1], depth=depths[i + 1])
        out.append(wp.pop())
    torch.cuda.synchronize()
    for i in range(len(frames)):
        assert np.array_equal(out[i], outs[2][i]), f"push / pop frame {i} differs from __call__"

    # a matte: the composite of a frame with external depth is composite_ref fed depth_ref's plane
    wm = wrapper()
    wm.set_matte(0.3, 0.7, feather=2)
    srcs = []
    for i, f in enumerate(frames[:4]):
        got = wm(f, depth=depths[i])
        srcs.append(wm.io.last_view[0].clone())
        if i >= N - 1:
            j = i - (N - 1)                                                  # the frame this output belongs to
            plane = torch.from_numpy(D.depth_ref(depths[j], H, W)[0, 0])
            want = composite_ref(wm.stream.prev_image_result, srcs[j][None], plane[None], 0.3, 0.7, feather=2)[0]
            assert 0 < np.count_nonzero(want != egress_ref(wm.stream.prev_image_result)[0].numpy())
            assert np.array_equal(got, want), f"matte, frame {i}"

    # depth_source="input": no depth model is needed, and a frame (or a prepare) without depth says so
    pipe = parts.pipe()
    del pipe.depth_model
    wi = wrapper(pipe, warm_depths=warm_d, depth_source="input", depth_input=dict(kind="distance", invalid=0, range=(500.0, 5000.0)))
    assert wi.stream.depth_detector is None and wi.depth_input["range"] == (500.0, 5000.0)
    got = [wi(f, depth=depths[i]) for i, f in enumerate(frames[:2])]
    assert all(o.shape == (H, W, 3) and o.std() > 0 for o in got)
    with pytest.raises(ValueError, match="depth"):
        wi(frames[2])
    with pytest.raises(ValueError, match="warmup_depths"):
        wi.prepare(warm, PROMPT)
    # the warm-up batch is normalised jointly: with the detector's wrapper and range=None the prepared stream differs from the
    # detector's, and a device tensor is taken as it is
    wj = wrapper(warm_depths=torch.from_numpy(warm_d.view(np.int16)).to(DEV))
    assert wj.stream.depth_detector.calls == 0
    assert not np.array_equal(wj(frames[0], depth=depths[0]), outs[2][0])
