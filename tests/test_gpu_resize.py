"""-m gpu: L2D_OP_FRAME_RESIZE (csrc/resize.hip) against `resize.resize_ref` -- Pillow's `Image.resize`, pinned in
tests/test_resize_cpu.py -- on every byte, from both source forms, behind guard bytes; and `set_output_size` on the wrapper with
small native components against a twin wrapper's unresized output; and the launches the wrapper's output route makes under every
combination of matte, colour lock and output size."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (1,16,16)->(17,16)    smaller than any tile; one axis skipped, the other grows by one pixel
# (1,16,16)->(128,128)  the 8x limit, every filter phase
# (3,40,72)->(100,99)   a batch; non-integer ratios; rows of 297 bytes, unaligned; no axis a whole number of tiles
# (1,24,136)->(12,68)   the 1/2 limit; 12-13 taps
# (2,64,96)->(33,95)    one axis down, one nearly unchanged
GEOMETRIES = [((1, 16, 16), (17, 16)), ((1, 16, 16), (128, 128)), ((3, 40, 72), (100, 99)), ((1, 24, 136), (12, 68)),
              ((2, 64, 96), (33, 95))]
FILTERS = ["lanczos", "bicubic", "bilinear"]
GUARD = 64


@functools.lru_cache(maxsize=None)
def data16(B, H, W):
    """frames N(0, 0.7) with planted -1, +1, 0, values beyond +-1 and fp16 subnormals (tests/test_gpu_matte.py `data`)"""
    g = torch.Generator().manual_seed(100 * H + W)
    x = (torch.randn(B, 3, H, W, generator=g) * 0.7).half()
    plant = torch.tensor([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8, -6e-8, 3e-5, 0.99951171875, -0.0], dtype=torch.float16)
    for b in range(B):
        for c in range(3):
            x[b, c].view(-1)[3 + c:3 + c + len(plant)] = plant
            x[b, c].view(-1)[-len(plant):] = plant.flip(0)
    return x


@functools.lru_cache(maxsize=None)
def data8(B, H, W):
    """noise, with a block of alternating 0 / 255 columns (one and two pixels wide) in the upper half and of alternating rows in the
    lower half: Lanczos and bicubic overshoot on both sides"""
    rng = np.random.default_rng(1000 * H + W)
    a = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    h2, w2 = H // 2, W // 2
    cols = np.where(np.arange(w2) % 2 == 0, 0, 255).astype(np.uint8)
    wide = np.where((np.arange(W - w2) // 2) % 2 == 0, 0, 255).astype(np.uint8)
    a[:, 1:h2, :w2] = cols[None, None, :, None]
    a[:, 1:h2, w2:] = wide[None, None, :, None]
    rows = np.where(np.arange(H - h2 - 1) % 2 == 0, 255, 0).astype(np.uint8)
    wrows = np.where((np.arange(H - h2 - 1) // 2) % 2 == 0, 255, 0).astype(np.uint8)
    a[:, h2:H - 1, :w2] = rows[None, :, None, None]
    a[:, h2:H - 1, w2:] = wrows[None, :, None, None]
    return a


@functools.lru_cache(maxsize=None)
def source_bytes(form, B, H, W):
    from live2diff_amd.frame_io import egress_ref
    return egress_ref(data16(B, H, W)).numpy() if form == "fp16" else data8(B, H, W)


@functools.lru_cache(maxsize=None)
def reference(form, src, out, resample):
    """(resize_ref of the source's bytes, smallest and largest unclipped value of either pass): computed once per case"""
    from live2diff_amd import resize as R
    (B, H, W), (Ho, Wo) = src, out
    a = source_bytes(form, B, H, W)
    lo, hi = 0, 255
    if Wo != W:
        s = R.pass_sums(a, 2, R.coefficients(W, Wo, resample)) >> R.PRECISION_BITS
        lo, hi = min(lo, int(s.min())), max(hi, int(s.max()))
        a = np.clip(s, 0, 255).astype(np.uint8)
    if Ho != H:
        s = R.pass_sums(a, 1, R.coefficients(H, Ho, resample)) >> R.PRECISION_BITS
        lo, hi = min(lo, int(s.min())), max(hi, int(s.max()))
        a = np.clip(s, 0, 255).astype(np.uint8)
    want = R.resize_ref(source_bytes(form, B, H, W), Ho, Wo, resample)
    assert np.array_equal(a, want)
    return want, lo, hi


def launch(src, B, H, W, Ho, Wo, resample, fill=7):
    """the op into a destination with GUARD bytes behind it, all pre-filled: (frame, guard bytes)"""
    from live2diff_amd import ops
    from live2diff_amd.resize import axis_table
    n = B * Ho * Wo * 3
    buf = torch.full((n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    tx = torch.from_numpy(axis_table(W, Wo, resample)).to(DEV)
    ty = torch.from_numpy(axis_table(H, Ho, resample)).to(DEV)
    ops.run(ops.frame_resize(src, buf[:n], tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    return got[:n].reshape(B, Ho, Wo, 3), got[n:]


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} bytes differ" + (f", max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}" if n else ""))
    return n


@pytest.mark.parametrize("form", ["fp16", "uint8"])
@pytest.mark.parametrize("resample", FILTERS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g[0])) + "-" + "x".join(map(str, g[1])))
def test_kernel_equals_resize_ref(geometry, resample, form):
    (B, H, W), (Ho, Wo) = geometry
    want, lo, hi = reference(form, *geometry, resample)
    if form == "uint8" and resample != "bilinear":
        assert lo < 0 and hi > 255, (lo, hi)                 # both clips are exercised
    src = data16(B, H, W).to(DEV) if form == "fp16" else torch.from_numpy(data8(B, H, W)).to(DEV)
    got, guard = launch(src, B, H, W, Ho, Wo, resample)
    assert report(f"{geometry} {resample} {form}", got, want) == 0
    assert np.all(guard == 7)


def test_kernel_repeatable_and_unaligned_destination():
    """two launches into differently filled outputs agree; a destination that starts at an odd address keeps the bytes around it"""
    from live2diff_amd import ops
    from live2diff_amd.resize import axis_table
    (B, H, W), (Ho, Wo) = geometry = GEOMETRIES[2]
    want, _, _ = reference("uint8", *geometry, "lanczos")
    src = torch.from_numpy(data8(B, H, W)).to(DEV)
    a, _ = launch(src, B, H, W, Ho, Wo, "lanczos", fill=0)
    b, _ = launch(src, B, H, W, Ho, Wo, "lanczos", fill=0xFF)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    n = B * Ho * Wo * 3
    tx, ty = (torch.from_numpy(axis_table(i, o, "lanczos")).to(DEV) for i, o in ((W, Wo), (H, Ho)))
    for off in (1, 2, 3):
        buf = torch.full((GUARD + n + GUARD,), 7, dtype=torch.uint8, device=DEV)
        ops.run(ops.frame_resize(src, buf[GUARD + off:GUARD + off + n], tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[GUARD + off:GUARD + off + n].reshape(want.shape), want), off
        assert np.all(got[:GUARD + off] == 7) and np.all(got[GUARD + off + n:] == 7), off


# ----------------------------------------------------------------------------- the wrapper on the device
def test_wrapper_output_size_on_device():
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import jpeg
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.resize import resize_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    Ho, Wo = 80, 112
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(N + 3, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(size=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if size is not None:
            w.set_output_size(*size)
        shown = w.prepare(warm, PROMPT)
        assert tuple(shown.shape[1:3]) == (H, W)                 # the frames `prepare` returns are not resized
        return w

    def same(ot, got, plain, size=(Ho, Wo), resample="lanczos", tag=""):
        want = resize_ref(plain, *size, resample)
        if ot == "u8":
            assert got.dtype == np.uint8 and report(f"{tag} u8", got, want) == 0
        elif ot == "pil":
            assert got.size == size[::-1] and report(f"{tag} pil", np.array(got), want) == 0
        else:
            assert isinstance(got, bytes) and got == jpeg.encode_ref(want, 75), (tag, ot)

    def both(w, twin, f, ot, **kw):
        w.output_type, twin.output_type = ot, "u8"
        got, plain = w(f), twin(f)
        assert plain.shape == (H, W, 3) and len(np.unique(plain)) > 16
        same(ot, got, plain, **kw)
        w.output_type = "u8"

    # __call__: the fp16 frame goes straight into op 46, which replaces the egress launch
    twin, w = wrapper(), wrapper((Ho, Wo))
    for t, ot in enumerate(("u8", "pil", "jpeg", "u8")):
        both(w, twin, frames[t], ot, tag=f"call {t}")
    assert w.jpeg is None and list(w._size_jpeg) == [(Ho, Wo)] and len(w._size_dev._plans) <= w._size_dev.MAX_PLANS
    # a matte and a colour lock: op 46 reads the matte's uint8 buffer
    for x in (w, twin):
        x.set_matte(0.3, 0.7, feather=2)
        x.set_color_lock("ema", 0.8, 0.3)
    for t, ot in enumerate(("u8", "jpeg", "pil")):
        both(w, twin, frames[t], ot, tag=f"matte + lock {t}")
    for x in (w, twin):
        x.clear_matte()
        x.clear_color_lock()
    # another size and filter, from the next output on; then none
    w.set_output_size(48, 96, "bicubic")
    both(w, twin, frames[3], "u8", size=(48, 96), resample="bicubic", tag="48 x 96 bicubic")
    both(w, twin, frames[4], "jpeg", size=(48, 96), resample="bicubic", tag="48 x 96 bicubic")
    assert sorted(w._size_jpeg) == [(48, 96), (Ho, Wo)]          # one encoder per size
    w.clear_output_size()
    assert w.output_size is None and w._size_dev is None and w._size_jpeg is None
    for ot in ("u8", "jpeg"):
        w.output_type = twin.output_type = ot
        got, plain = w(frames[0]), twin(frames[0])
        assert np.array_equal(got, plain) if ot == "u8" else got == plain

    # push / pop with one frame in flight
    wp, tp = wrapper((Ho, Wo), frame_pipelining=True), wrapper(frame_pipelining=True)
    out, plain = [], []
    for x, o in ((wp, out), (tp, plain)):
        x.push(frames[0])
        for i in range(len(frames)):
            if i + 1 < len(frames):
                x.push(frames[i + 1])
            if x is wp:
                x.output_type = ("u8", "jpeg", "pil")[i % 3]
            o.append(x.pop())
    torch.cuda.synchronize()
    for i, (got, p) in enumerate(zip(out, plain)):
        same(("u8", "jpeg", "pil")[i % 3], got, p, tag=f"push / pop {i}")


# the launches of the output route, as the parent of the commit that made the route one chain recorded them on the device: the
# colour lock, then the matte, then the resize; the egress launch only where neither of the two takes its place; "jpeg" ends
# in the encoder's three launches and never has an egress launch in front of them
LOCK, MATTE, RESIZE, EGRESS = ("OP_FRAME_MOMENTS", "OP_COLOR_LOCK"), ("OP_FRAME_MATTE",), ("OP_FRAME_RESIZE",), ("OP_FRAME_EGRESS",)
JPEG = ("OP_JPEG_DCT", "OP_JPEG_HUFF", "OP_JPEG_PACK")
ROUTE_LAUNCHES = {                               # (output type, matte, colour lock, output size): the first and every later call
    ("u8", False, False, False): EGRESS,
    ("u8", False, False, True): RESIZE,
    ("u8", False, True, False): LOCK + EGRESS,
    ("u8", False, True, True): LOCK + RESIZE,
    ("u8", True, False, False): MATTE,
    ("u8", True, False, True): MATTE + RESIZE,
    ("u8", True, True, False): LOCK + MATTE,
    ("u8", True, True, True): LOCK + MATTE + RESIZE,
    ("jpeg", False, False, False): JPEG,
    ("jpeg", False, False, True): RESIZE + JPEG,
    ("jpeg", False, True, False): LOCK + JPEG,
    ("jpeg", False, True, True): LOCK + RESIZE + JPEG,
    ("jpeg", True, False, False): MATTE + JPEG,
    ("jpeg", True, False, True): MATTE + RESIZE + JPEG,
    ("jpeg", True, True, False): LOCK + MATTE + JPEG,
    ("jpeg", True, True, True): LOCK + MATTE + RESIZE + JPEG,
}


def test_output_route_launch_sequences(monkeypatch):
    """The route alone (`_finish`, or `postprocess_image` with nothing set) on frames the stream made, under the eight
    combinations of matte, colour lock and output size, as "u8" and as "jpeg", twice each (the second call meets the objects the
    first one made): the op kinds of every list that runs equal ROUTE_LAUNCHES, and the bytes equal the host composition
    lock_ref -> composite_ref | egress_ref -> resize_ref -> encode_ref of the same frame."""
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import _lib, jpeg
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.color_lock import lock_ref
    from live2diff_amd.config import tiny_config
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.matte import composite_ref
    from live2diff_amd.resize import resize_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    Ho, Wo = 80, 112
    torch.manual_seed(0)
    w = Wrapper.from_components(Parts(ucfg, ccfg, H, W, N).pipe(), output_type="u8", seed=SEED, device=DEV, num_inference_steps=50,
                                t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)
    w.set_matte(0.3, 0.7, feather=2)
    w.prepare(u8_frames(8, 96, 128, seed=1), PROMPT)
    xs = []
    for f in u8_frames(N + 1, 96, 128, seed=2):
        w(f)
        xs.append(w.stream.prev_image_result.clone())
    xs = [xs[-2], w.stream.prev_image_result]                    # the first and the second call of every case
    slot, settings = w._matte_line.last, w.matte
    assert slot is not None and not torch.equal(xs[0], xs[1])

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, run = [], _lib.OpList.run

    def recording(self, *a, **kw):
        ran.extend(kinds[op.kind] for op in self._ops)
        return run(self, *a, **kw)

    monkeypatch.setattr(_lib.OpList, "run", recording)
    bad = []
    for (ot, matte, lock, size), launches in ROUTE_LAUNCHES.items():
        w.clear_matte()
        w.clear_color_lock()
        w.clear_output_size()
        w.output_type = ot
        if matte:
            w.set_matte(**settings)
        if lock:
            w.set_color_lock("ema", 0.8, 0.3)
        if size:
            w.set_output_size(Ho, Wo)
        state = None
        for call, x in enumerate(xs):
            del ran[:]
            got = w._finish(x, slot) if matte or lock or size else w.postprocess_image(x, ot)
            seen = tuple(ran)
            print(f"{ot:4s} matte={matte:d} lock={lock:d} size={size:d} call {call}: {' '.join(seen)}")
            if seen != launches:
                bad.append((ot, matte, lock, size, call, seen))
            want = x
            if lock:
                want, state = lock_ref(x, state, mode="ema", strength=0.8, rate=0.3, init=call == 0)
                want = torch.from_numpy(want)
                assert call == 0 or not torch.equal(want, x.cpu())               # (the lock does something)
            want = composite_ref(want, slot.source[None], slot.depth[None], **settings)[0] if matte else egress_ref(want)[0].numpy()
            if size:
                want = resize_ref(want, Ho, Wo, "lanczos")
            tag = f"{ot} matte={matte:d} lock={lock:d} size={size:d} call {call}"
            if ot == "u8":
                assert got.dtype == np.uint8 and got.shape == want.shape and report(tag, got, want) == 0
            else:
                assert isinstance(got, bytes) and got == jpeg.encode_ref(want, 75), tag
    assert not bad, bad
