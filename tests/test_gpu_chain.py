"""-m gpu: the output chain as a whole on the device route: the wrapper with small native components
against tests/chain_model.py, byte for byte on every output and launch for launch -- the walk of tests/test_chain_cpu.py plus
what only the device has (the camera route and detail, and the frames they do not act on; a change of output size with frames
of the old key in the line; a second camera geometry; JPEG in and out), push / pop with one and two frames in flight, and
three of the CPU file's seeded scripts extended with the device-only events.  Nothing here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import chain_model as CM
from test_chain_cpu import SIZE_A, SIZE_B, check_cleared, random_script

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 64
HS, WS = 96, 128
T_INDEX = {2: [30, 40], 3: [20, 30, 40]}
DEVICE_SEEDS = (101, 106, 110)                   # of test_chain_cpu.SEEDS[2]
DEVICE_MODES = ("lock", "steady", "matte", "edge", "size", "detail", "camera")

LOCK, JPEG = ("OP_FRAME_MOMENTS", "OP_COLOR_LOCK"), ("OP_JPEG_DCT", "OP_JPEG_HUFF", "OP_JPEG_PACK")
STAGE_OPS = {                                    # per stage, the launches the per-feature device tests pin
    "camera": ("OP_FRAME_RESIZE",),              # the camera tap, inside the ingest (test_gpu_matte_up.INGEST)
    "lock": LOCK, "steady": ("OP_FRAME_STEADY",), "edge": ("OP_FRAME_MATTE_EDGE",), "matte": ("OP_FRAME_MATTE",),
    "resize": ("OP_FRAME_RESIZE",), "detail": ("OP_FRAME_DETAIL_GAIN", "OP_FRAME_RESIZE", "OP_FRAME_DETAIL"),
    "matte_up": ("OP_FRAME_MATTE_UP",), "egress": ("OP_FRAME_EGRESS",), "jpeg": JPEG,
}
FRAME_OPS = frozenset(op for ops in STAGE_OPS.values() for op in ops)


def source_of(x, kind):
    """the model's own expectation of the frame the pipeline keeps: `ingest_ref` of the uint8 frame (of the decoded file, of the
    host-resized PIL image), 2 x - 1 of a float frame"""
    from live2diff_amd import jpeg
    from live2diff_amd.frame_io import ingest_ref
    if kind == "float":
        return 2.0 * x.float() - 1.0
    if kind == "jpeg":
        x = jpeg.decode_ref(bytes(x))
    elif kind == "pil":
        x = np.array(x.convert("RGB").resize((W, H)))
    return ingest_ref(x, H, W)[0]


# ----------------------------------------------------------------------------- frames
def camera_frames(n, seed, hs=HS, ws=WS):
    """a moving camera: one random uint8 frame, +-1 level of noise per frame, a band of fresh content that walks"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (hs, ws, 3))
    out = []
    for k in range(n):
        x = np.clip(base + rng.integers(-1, 2, base.shape), 0, 255)
        x0 = (16 * k) % (ws - 32)
        x[:, x0:x0 + 32] = rng.integers(0, 256, (hs, 32, 3))
        out.append(x.astype(np.uint8))
    return out


def unrelated(n, seed, hs=HS, ws=WS):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8) for _ in range(n)]


def as_float(frame):
    """the frame's stream-sized window as a float [3,H,W] tensor in [0, 1], in steps of 1 / 256 (2 x - 1 is exact in fp16)"""
    x = torch.from_numpy(frame[16:80, 32:96].astype(np.int64) + 1).clamp(0, 256).permute(2, 0, 1).float() / 256.0
    return x.contiguous()


def as_pil(frame):
    from PIL import Image
    return Image.fromarray(frame)


def as_jpeg(frame):
    from live2diff_amd import jpeg
    return jpeg.encode_ref(frame, 90)


# ----------------------------------------------------------------------------- one wrapper, one model, one twin
@functools.lru_cache(maxsize=None)
def parts(n_steps):
    from test_gpu_wrapper import Parts

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    return Parts(ucfg, ccfg, H, W, n_steps), ucfg


def start(monkeypatch, n_steps, twin=True, **more):
    from test_gpu_wrapper import PROMPT, SEED, u8_frames
    from test_matte_cpu import DropFilter

    from live2diff_amd import _lib
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    p, ucfg = parts(n_steps)
    kw = dict(num_inference_steps=50, t_index_list=T_INDEX[n_steps], width=W, height=H, warmup_frames=ucfg.sink_size,
              window_size=ucfg.window_size, output_type="u8", seed=SEED, device=DEV, jpeg_quality=75)

    def wrapper():
        torch.manual_seed(0)
        w = Wrapper.from_components(p.pipe(), **kw, **more)
        w.stream.similar_filter, w.stream.similar_image_filter = DropFilter(set()), True
        return w

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, real = [], _lib.OpList.run

    def recording(self, *a, **k):
        ran.extend(kinds[op.kind] for op in self._ops if kinds[op.kind] in FRAME_OPS)
        return real(self, *a, **k)

    monkeypatch.setattr(_lib.OpList, "run", recording)
    rec = CM.TapRecorder(monkeypatch)
    w, t = wrapper(), (wrapper() if twin else None)
    model = CM.ChainModel(n_steps, H, W, source_of, source_tol=5e-4, device_route=True, jpeg_quality=75)
    run = CM.ChainRun(w, model, rec, filt=w.stream.similar_filter, twin=t, twin_filt=t.stream.similar_filter if twin else None,
                      prompt=PROMPT, launches=ran, stage_ops=STAGE_OPS, sync=torch.cuda.synchronize)
    return run, u8_frames(8, HS, WS, seed=1)


SEVEN = {"lock", "steady", "matte", "edge", "size", "detail"}


def longest_run(outs, cond):
    best = cur = 0
    for e in outs:
        cur = cur + 1 if e != "raised" and cond(e) else 0
        best = max(best, cur)
    return best


# ----------------------------------------------------------------------------- the scenario
def scenario(part, warm):
    """The walk, in two parts of about 40 and 30 frames with a wrapper, a model and a twin each (one part ran longer than twice
    the slowest per-feature wrapper test).  "a": modes set before `prepare`, the seven modes coming on one by one on the
    "stream" and then on the "camera" route, every output and input type, a change of size and of camera geometry, `show` of
    matte, steady and detail, restarts with a drop directly behind them, the ValueError of "pt".  "b": mid-stream starts of the
    line, a second `prepare` with modes set, a reference image, the rings in steady state.  Both end cleared, on the twin's bytes."""
    mv = camera_frames(30, seed=41)
    un = unrelated(8, seed=42)
    mw = camera_frames(12, seed=43)
    big = camera_frames(1, seed=44, hs=80, ws=144)[0]
    image = unrelated(1, seed=45, hs=H, ws=W)[0]
    S = lambda name, *a, **kw: ("set", name, a, kw)
    F, D = (lambda x: ("frame", x)), (lambda x: ("drop", x))
    if part == "a":
        return [
            S("set_matte", 0.3, 0.7, feather=2), S("set_steady"), S("set_output_size", *SIZE_A), ("prepare", warm),
            F(mv[0]), F(mv[1]),                                                    # steady + matte + size, the "stream" route
            S("set_color_lock", "ema", 0.8, 0.3), F(mv[2]),                        # + lock
            S("set_matte_edge", 2, 4.0), D(mv[3]), F(mv[3]),                       # + edge; a drop directly behind a settings change
            S("set_detail"), F(mv[4]), F(mv[5]), F(mv[6]), F(mv[7]), F(mv[8]), F(mv[9]),    # + detail: the first outputs pair frames
                                                                                   # from before the tap; then all seven, "stream"
            S("set_matte_source", "camera"), F(mv[10]), F(mv[11]),                 # all seven on the "camera" route
            ("type", "pil"), F(mv[12]), ("type", "jpeg"), F(mv[13]), ("type", "u8"), F(mv[14]),
            D(mv[15]),                                                             # repeated: computed again from the same slot
            F(as_float(mv[15])), F(mv[16]), F(mv[17]),                             # a float frame has no camera frame
            F(as_pil(mv[18])), F(mv[19]),                                          # nor has a PIL image
            F(as_jpeg(mv[20])), F(as_jpeg(mv[21])), F(mv[22]),                     # JPEG files decoded on the device have one
            S("set_output_size", *SIZE_B), F(mv[23]), F(mv[24]), F(mv[25]),        # frames of the old key are still in the line
            F(big), F(mv[26]), F(mv[27]),                                          # another source size: the tap rebuilds
            S("set_matte", 0.3, 0.7, feather=2, show=True), F(mv[28]), S("set_matte", 0.2, 0.8, keep="far", feather=1),
            S("set_steady", 2, 10, show=True), F(mv[29]), S("set_steady", 3, 12, strength=0.5, radius=1), D(mw[0]),
            S("set_detail", 3, 1.0, 2.5, 20.0, True), F(mw[0]), F(mw[1]), S("set_detail"),
            S("set_color_lock", "ema", 0.6, 0.5), D(mw[2]), F(mw[2]),              # the lock restarted, a drop directly behind it
            ("type", "pt"), S("set_matte", 0.1, 0.9), F(mw[3]),                    # both raise: matte, size and detail do not serve "pt"
            S("clear_matte"), S("clear_output_size"), S("clear_detail"), S("clear_matte_edge"),
            F(mw[4]), ("type", "np"), F(mw[5]), ("type", "u8"),                    # lock + steady as "pt" and "np"
            S("clear_steady"), S("clear_color_lock"), S("set_matte_source", "stream"), ("twin",),
            F(un[0]), D(un[1]), F(un[1]),
        ]
    return [
        ("prepare", warm), F(un[0]),                                               # nothing set: no line
        S("set_steady"), F(un[1]), F(un[2]), F(un[3]), F(un[4]),                   # a mid-stream start on unrelated frames
        S("clear_steady"), F(un[5]),
        S("set_color_lock", "source"), D(un[6]), F(un[6]),                         # a drop directly behind a mid-stream start
        S("set_matte", 0.4, 0.6, feather=1), S("set_matte_edge", 1, 2.0), S("set_output_size", *SIZE_A), S("set_detail"),
        S("set_matte_source", "camera"),
        ("prepare", warm),                                                         # a second prepare, modes set
        F(mw[6]), F(mw[7]), S("set_color_lock", image, 0.9), S("set_steady"), F(mw[8]), F(mw[9]), F(mw[10]),
        ("mark",), F(mw[11]), F(mv[0]), F(mv[1]), F(mv[2]), F(mv[3]), F(mv[4]), F(mv[5]), F(mv[6]), ("still",),
        S("clear_matte_edge"), S("clear_matte"), S("clear_steady"), S("clear_output_size"), S("clear_color_lock"), S("clear_detail"),
        S("set_matte_source", "stream"), ("twin",),
        F(mv[7]), F(mv[8]), D(mv[9]), F(mv[9]),
    ]


@pytest.mark.parametrize("part", ["a", "b"])
@pytest.mark.parametrize("n_steps", [2, 3])
def test_everything_scenario(monkeypatch, n_steps, part):
    run, warm = start(monkeypatch, n_steps)
    w = run.w
    grown = []
    for ev in scenario(part, warm):
        if ev[0] in ("mark", "still"):                                             # the rings over the last 8 frames before the clears
            grown.append((w._camera.allocated, len(w._matte_line.slots)))
        else:
            run.play([ev])
    log = run.log
    outs = [e for e in log if e != "raised"]
    check_cleared(w)
    assert w.io.camera_tap is None
    if part == "a":
        assert log.count("raised") == 1 and len(outs) >= 40
        stream7 = longest_run(log, lambda e: SEVEN <= e.acts and "camera" not in e.acts)
        camera7 = longest_run(log, lambda e: SEVEN | {"camera"} <= e.acts)
        print(f"N = {n_steps}, part a: {len(outs)} outputs equal the model; all seven modes act on {stream7} consecutive outputs on "
              f"the 'stream' route and on {camera7} on the 'camera' route")
        assert stream7 >= 4 and camera7 >= 4
        assert {e.output_type for e in outs} == {"u8", "pil", "jpeg", "pt", "np"}
        # what only the device has did act, and did not where it must not
        assert sum(1 for e in outs if "detail" in e.acts) >= 20 and sum(1 for e in outs if "camera" in e.acts) >= 15
        assert sum(1 for e in outs if e.acts >= {"matte", "size"} and "camera" not in e.acts) >= 10
    else:
        assert "raised" not in log and len(outs) >= 25
        print(f"N = {n_steps}, part b: {len(outs)} outputs equal the model; camera buffers and ring slots before and after the "
              f"last 8 frames {grown}")
        assert grown[0] == grown[1], grown
        assert run.m.line_starts == 2
    for i, e in enumerate(log):
        print(f"  {i:2d} " + ("raised" if e == "raised" else f"{e.output_type:4s} {'rep ' if e.repeated else ''}{' '.join(e.stages)}"))


# ----------------------------------------------------------------------------- push / pop
def push_pop_script(warm):
    f = camera_frames(12, seed=51)
    S = lambda name, *a, **kw: ("set", name, a, kw)
    P, O = (lambda x: ("push", x)), ("pop",)
    return [
        S("set_color_lock", "ema", 0.8, 0.3), S("set_output_size", *SIZE_A), ("prepare", warm),
        P(f[0]), S("set_steady"),                                                  # one frame pending: its output has no slot
        P(f[1]), O, P(f[2]), O, P(f[3]), O, P(f[4]), O, O,                         # a foreign slot, then the init frame, then steady acts
        S("clear_steady"),
        P(f[5]), P(f[6]),                                                          # two frames pending
        S("set_matte", 0.3, 0.7, feather=2), S("set_matte_edge", 2, 4.0), S("set_detail"), S("set_matte_source", "camera"),
        P(f[7]), O, P(f[8]), O, P(f[9]), O, P(f[10]), O, P(f[11]), O, O, O,
    ]


def test_everything_push_pop(monkeypatch):
    """N = 2, one and two frames in flight; modes set before `prepare` and mid-stream while frames are pending, so that one and
    two outputs have no slot at all; the mid-stream steady start among them."""
    run, warm = start(monkeypatch, 2, twin=False, frame_pipelining=True)
    run.play(push_pop_script(warm))
    log = run.log
    assert len(log) == 12 and "raised" not in log
    acts = [sorted(e.acts) for e in log]
    print("\n".join(f"  pop {i:2d}: own {e.own!s:5s} {' '.join(e.stages)}" for i, e in enumerate(log)))
    assert [e.own for e in log] == [False, False, True, True, True] + [False, False, False] + [True] * 4
    assert "steady" not in log[1].acts and "steady" in log[2].acts and "steady" in log[4].acts
    assert not log[5].acts - {"lock", "size"} and not log[6].acts - {"lock", "size"}            # no slot at all: neither matte nor detail
    assert {"matte", "edge", "camera"} <= log[7].acts and "detail" not in log[7].acts           # the oldest entry: a matte, no detail
    assert all({"matte", "edge", "camera", "detail", "lock", "size"} <= e.acts for e in log[8:]), acts[8:]


# ----------------------------------------------------------------------------- seeded scripts
def device_hooks(warm):
    def fresh(g):
        return torch.randint(0, 256, (HS, WS, 3), dtype=torch.uint8, generator=g).numpy()

    def move(base, k, g):
        x = (torch.from_numpy(base).int() + torch.randint(-1, 2, base.shape, generator=g).int()).clamp(0, 255).to(torch.uint8)
        x0 = (16 * k) % (WS - 32)
        x[:, x0:x0 + 32] = torch.randint(0, 256, (HS, 32, 3), dtype=torch.uint8, generator=g)
        return x.numpy()

    def dress(x, rng):
        r = rng.random()
        return as_jpeg(x) if r < 0.10 else as_float(x) if r < 0.15 else as_pil(x) if r < 0.20 else x

    return dict(warm=warm, fresh=fresh, move=move, dress=dress, modes=DEVICE_MODES + ("size", "detail"),
                image=lambda g: torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).numpy(),
                types=["u8", "u8", "u8", "pil", "jpeg"], preset=0.9, sticky=("size", "detail", "matte", "camera"))


def on_device_routes(logs):
    outs = [e for log in logs for e in log if e != "raised"]
    return sum(1 for e in outs if e.acts & {"detail", "camera"}), len(outs)


def test_seeded_scripts_on_device(monkeypatch):
    """three of the CPU file's seeds with the device-only events: 24 events each, and at least half of the outputs on the
    device-only routes (the camera composite or detail), from the model"""
    logs = []
    for seed in DEVICE_SEEDS:
        with monkeypatch.context() as mp:
            run, warm = start(mp, 2, twin=False)
            try:
                logs.append(run.play(random_script(seed, hooks=device_hooks(warm))))
            except AssertionError as e:
                raise AssertionError(f"seed {seed}: {e}") from e
    n, total = on_device_routes(logs)
    print(f"{len(logs)} scripts, {total} outputs, {n} on the device-only routes")
    assert 2 * n >= total and total >= 30


# ----------------------------------------------------------------------------- the two findings, on the device
@pytest.mark.parametrize("n_steps", [2, 3])
def test_mid_stream_steady_start_on_device(monkeypatch, n_steps):
    """tests/test_steady_cpu.py::test_wrapper_mid_stream_start_never_holds_a_foreign_source on the device route: `set_steady()`
    with its defaults behind two plain frames, then unrelated frames -- every output is the unsteadied frame, byte for byte"""
    from live2diff_amd.frame_io import egress_ref
    run, warm = start(monkeypatch, n_steps, twin=False)
    frames = unrelated(7, seed=61)
    run.prepare(warm)
    for f in frames[:2]:
        run.frame(f)
    run.settings("set_steady")
    diffs = []
    for f in frames[2:]:
        got = run.frame(f)
        plain = egress_ref(run.w.stream.prev_image_result)[0].numpy()
        diffs.append(int(np.abs(got.astype(int) - plain.astype(int)).max()))
    own = [e.own for e in run.log[2:]]
    print(f"N = {n_steps}: own slot {own}, largest byte difference to the unsteadied frame {diffs}")
    assert own == [False] * (n_steps - 1) + [True] * (6 - n_steps) and diffs == [0] * 5
    assert ["steady" in e.stages for e in run.log[2:]] == own                      # no launch on a foreign slot


def test_pil_frame_has_no_camera_frame(monkeypatch):
    """A PIL image is resized on the host and reaches the ingest at the stream's size: it has no camera frame (`set_detail`,
    `set_matte_source`), so its output takes the "stream" route without detail.  With the tap left in the ingest of such a
    frame -- the wrapper before `_camera_begin` -- the stream-sized picture passes for the camera's and the model fails."""
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    f = camera_frames(5, seed=62)
    S = lambda name, *a, **kw: ("set", name, a, kw)
    script = [S("set_matte", 0.3, 0.7, feather=2), S("set_output_size", *SIZE_A), S("set_detail"), S("set_matte_source", "camera"),
              ("prepare", None), ("frame", f[0]), ("frame", as_pil(f[1])), ("frame", f[2]), ("frame", f[3])]
    run, warm = start(monkeypatch, 2, twin=False)
    script[4] = ("prepare", warm)
    log = run.play(script)
    assert ["matte_up" in e.stages for e in log] == [False, True, False, True] and "detail" not in log[2].stages

    def begin(self, image):
        if self._camera is not None:
            self._camera.begin()

    with monkeypatch.context() as mp:
        run, _ = start(mp, 2, twin=False)
        mp.setattr(Wrapper, "_camera_begin", begin)
        with pytest.raises(CM.ChainMismatch) as caught:
            run.play(script)
        print(f"the tap left in a PIL frame's ingest: {caught.value}")
        assert len(run.log) == 2                                                   # the PIL frame's own call: a launch too many
