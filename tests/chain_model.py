"""One independent model of the stream wrapper's output chain (wrapper.py `_finish` / `_route`, DESIGN.md sections 8.z4 to
8.z11), in plain numpy / torch on the byte-exact host references: `lock_ref`, `steady_ref`, `composite_ref` (with `edge_ref`),
`resize_ref`, `detail_ref`, `composite_up_ref`, `egress_ref`, `encode_ref`.  It is fed the event script the wrapper is fed and
returns, for every output, the expected bytes and the names of the stages that act on it.  Shared by tests/test_chain_cpu.py
(mock components, host route) and tests/test_gpu_chain.py (native components, device route), with the driver that feeds a
script to a wrapper, the model and a twin (`ChainRun`) and the model-only player the scripts' coverage is computed with
(`play_model_only`).

Own bookkeeping.  The model keeps the list of accepted frames, the delay line's start, the lock's and the steady mode's state,
the camera tap's key and the frames in flight itself; it reads nothing of that from the wrapper.  From the run it takes only
(a) the styled tensor the stream returned for the output and (b) the `(source, depth)` pair the pipeline handed to the tap for
every accepted frame (`TapRecorder`), and the source is first compared with the model's own expectation for that frame
(`source_of`): a frame of the wrong index fails there, before any bytes are compared.

The pairing.  With N denoising steps, output k of the accepted sequence belongs to accepted frame k - (N - 1).  Positions in
front of the first frame hold the last warm-up frame after `prepare`; after a mid-stream start of the line they hold nothing.

The rules, in the order the stages run on a frame:

  stage               acts when                                      on what                         no own slot
  ------------------  ---------------------------------------------  ------------------------------  -------------------------
  1 lock              a colour lock is set                           the styled fp16 frame           "source": the oldest entry
                                                                                                     the line has (stateless: no
                                                                                                     later frame inherits); no
                                                                                                     slot at all: passes
  2 steady            steady is set                                  the locked frame                passes; the sequence has
                                                                                                     not started: the first
                                                                                                     output with its own slot is
                                                                                                     the init frame
  3 matte ("stream")  a matte is set and the camera route is not     the steadied frame over the     the oldest entry the line
                      taken; the edge refinement in front of the     slot's source                   has; no slot at all: none
                      feather
  4 resize            an output size is set                          the bytes of 3, or the egress   --
                                                                     bytes of 2
  5 detail            detail and a size are set, device route, the   the resized frame; gains on     no detail
                      slot is the output's own and carries a camera  the bytes the resize read
                      frame of the current (Ho, Wo, resample)
  6 matte ("camera")  "camera", a matte and a size are set, device   the bytes of 4 / 5 over the     the oldest entry's camera
                      route, the slot carries a camera frame of the  camera frame; the matte is      frame, where it has one
                      current key                                    refined at the stream's size
  7 encoder           "jpeg": `encode_ref`; "u8" / "pil": the bytes  the bytes of 2 .. 6             --

State rules.
  * `set_color_lock` and `prepare` restart the lock ("ema": the next frame copies its own moments; an image's moments are
    measured once and stay over `prepare`); `set_steady` and `prepare` restart the steady sequence (the next frame with its own
    slot passes as it is).  `clear_*` drops the state.  No other call touches either.
  * A repeated frame (the near-duplicate filter refused the call) returns the last locked and the last steadied frame with the
    state unmoved; matte, edge, resize and detail are computed again from the slot of the output before: the same bytes.  With
    no locked / steadied frame to repeat (a drop directly behind `set_color_lock` / `set_steady` / `prepare`) the repeated
    frame is treated as a frame of its own, with the slot of the output before; with no output before, as one with no slot.
  * A camera frame exists only for a frame that came in as a uint8 frame or a JPEG file while the tap was wanted -- ("camera"
    and a matte, or detail) and an output size, device route -- with the current (Ho, Wo, resample), without a break since.
  * Served output types: lock and steady every type but "latent"; matte, output size and detail "u8", "pil", "jpeg"; an
    output size under "jpeg" must be whole 16 x 16 blocks.  `set_*` raises ValueError otherwise and changes nothing.  A frame
    that meets a set mode its `output_type` does not serve raises ValueError too; the frame is consumed all the same: the
    pairing advances, and lock and steady have run where their own type check passed.
  * The host route (no device) has no camera route and no detail: `set_matte_source("camera")` and `set_detail` change no byte.
  * push / pop: the output of a frame pushed before the line existed has no slot at all.
"""
import numpy as np
import torch

from live2diff_amd import color_lock as CL
from live2diff_amd import detail as DT
from live2diff_amd import jpeg as JP
from live2diff_amd import matte as MT
from live2diff_amd import resize as RS
from live2diff_amd import steady as SD
from live2diff_amd.frame_io import egress_ref

# the references, bound here: a test that plants a mutant in the wrapper's path by patching a module attribute leaves the model's
lock_ref, steady_ref, composite_ref, composite_up_ref = CL.lock_ref, SD.steady_ref, MT.composite_ref, MT.composite_up_ref
resize_ref, detail_ref, encode_ref, decode_ref, moments_ref = RS.resize_ref, DT.detail_ref, JP.encode_ref, JP.decode_ref, CL.moments_ref

U8_TYPES = ("u8", "pil", "jpeg")
FLOAT_OK = ("pil", "pt", "np", "u8", "jpeg")
MODES = ("lock", "steady", "matte", "edge", "size", "detail", "camera")


def kind_of(x) -> str:
    """how a frame comes in: "jpeg" (a file as bytes), "u8" (a uint8 array / tensor), "pil", or "float" (a [3,H,W] tensor)"""
    if isinstance(x, (bytes, bytearray, memoryview)):
        return "jpeg"
    if hasattr(x, "convert") and hasattr(x, "resize"):
        return "pil"
    dt = getattr(x, "dtype", None)
    return "u8" if dt == torch.uint8 or dt == np.uint8 else "float"


class TapRecorder:
    """(b): clones of what the pipeline hands to the delay line -- `MatteLine.__call__` per accepted frame, `MatteLine.prime`
    per `prepare` -- recorded by a monkeypatch that then calls on"""

    def __init__(self, monkeypatch):
        self.calls, self.primes = [], []
        call, prime = MT.MatteLine.__call__, MT.MatteLine.prime
        rec = self

        def tapped(line, x, dn):
            rec.calls.append((x.detach().clone(), dn.detach().clone()))
            return call(line, x, dn)

        def primed(line, x, dn):
            rec.primes.append((x.detach().clone(), dn.detach().clone()))
            return prime(line, x, dn)

        monkeypatch.setattr(MT.MatteLine, "__call__", tapped)
        monkeypatch.setattr(MT.MatteLine, "prime", primed)

    def take(self):
        out = self.calls[:]
        del self.calls[:]
        return out

    def take_prime(self):
        out = self.primes[:]
        del self.primes[:]
        return out


class Expected:
    """what one output must be: `value` by `output_type` (uint8 array for "u8" and "pil", the file for "jpeg", the tensor /
    array of the float types), `stages` (the stages that launch, in order) and `acts` (the modes that act on it)"""

    def __init__(self, output_type, value, stages, acts, repeated, own):
        self.output_type, self.value, self.stages, self.acts, self.repeated, self.own = output_type, value, tuple(stages), frozenset(acts), repeated, own

    def differs(self, got):
        """None where `got` is the expected output, else a short description"""
        ot, want = self.output_type, self.value
        if ot == "jpeg":
            return None if isinstance(got, bytes) and got == want else f"the JPEG file differs ({len(got) if isinstance(got, bytes) else type(got)} / {len(want)} bytes)"
        if ot == "pil":
            got = np.array(got)
        if torch.is_tensor(want):
            ok = torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)
            return None if ok else f"the {ot} tensor differs"
        got = np.asarray(got)
        if got.dtype != want.dtype or got.shape != want.shape:
            return f"{got.dtype} {got.shape} in place of {want.dtype} {want.shape}"
        n = int(np.count_nonzero(got != want))
        if not n:
            return None
        return f"{n} of {want.size} values differ, by up to {float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()):g}"


class _Entry:
    def __init__(self, source, depth, camera=None, epoch=None):
        self.source, self.depth, self.camera, self.epoch = source, depth, camera, epoch


class _Line:
    def __init__(self):
        self.entries, self.primed, self.taken = [], None, 0
        self.mid = False                       # started mid-stream: no position in front of its first frame


class ChainModel:
    """`source_of(x, kind)`: the model's own expectation of the frame the pipeline keeps for input `x` (float [3,H,W] in
    [-1, 1]); the recorded source must agree with it within `source_tol` (0: bit for bit, in fp16).  `device_route`: the wrapper
    runs its device route (camera route and detail exist)."""

    def __init__(self, n_steps, height, width, source_of, *, source_tol=0.0, device_route=False, output_type="u8", jpeg_quality=75):
        self.n, self.H, self.W = int(n_steps), int(height), int(width)
        self.source_of, self.source_tol, self.device_route = source_of, float(source_tol), bool(device_route)
        self.output_type, self.jpeg_quality = output_type, jpeg_quality
        self.matte = self.edge = self.lock = self.steady = self.size = self.detail = None
        self.matte_source = "stream"
        self.lock_state, self.lock_init, self.lock_last = None, True, None
        self.steady_state, self.steady_init, self.steady_last = None, True, None
        self.line = None
        self.last = None                       # (entry, own) of the output before, or None
        self.pending = []                      # push / pop: per frame in flight, the line it was pushed into (or None)
        self.tap_key, self.epoch = None, 0
        self.accepted = 0
        self.line_starts = 0                   # mid-stream starts of the line (counted for the scripts' conditions)

    # ------------------------------------------------------------------ settings
    def _served(self, served, what):
        if self.output_type not in served:
            raise ValueError(f"model: output_type={self.output_type!r} does not serve {what}")

    def _sync(self):
        need = (self.matte is not None or self.steady is not None or self.detail is not None
                or (self.lock is not None and self.lock["mode"] == "source"))
        if need and self.line is None:
            self.line, self.last = _Line(), None
            self.line.mid = self.accepted > 0
            for i in range(len(self.pending)):                         # frames in flight were pushed before this line existed
                self.pending[i] = None
        elif not need:
            self.line = self.last = None
        want = (((self.matte_source == "camera" and self.matte is not None) or self.detail is not None)
                and self.size is not None and self.device_route)
        key = (self.size["height"], self.size["width"], self.size["resample"]) if want else None
        if key != self.tap_key:
            self.tap_key, self.epoch = key, self.epoch + 1

    def set_matte(self, lo, hi, *, keep="near", feather=0, show=False):
        self._served(U8_TYPES, "a matte")
        self.matte = MT.check_settings(lo, hi, keep=keep, feather=feather, show=show)
        self._sync()

    def clear_matte(self):
        self.matte = None
        self._sync()

    def set_matte_source(self, source):
        if source not in ("stream", "camera"):
            raise ValueError(source)
        self.matte_source = source
        self._sync()

    def set_matte_edge(self, radius=4, eps=10.0):
        self.edge = MT.check_edge(radius, eps)

    def clear_matte_edge(self):
        self.edge = None

    def set_color_lock(self, to="source", strength=1.0, rate=0.1):
        self._served(FLOAT_OK, "a colour lock")
        settings = CL.check_settings(to, strength, rate)
        ref = None
        if settings["mode"] == "image":
            ref = moments_ref(self.source_of(to, kind_of(to)).to(torch.float16))
        self.lock, self.lock_state, self.lock_init, self.lock_last = settings, ref, True, None
        self._sync()

    def clear_color_lock(self):
        self.lock, self.lock_state, self.lock_init, self.lock_last = None, None, True, None
        self._sync()

    def set_steady(self, lo=2.0, hi=10.0, *, strength=0.8, radius=2, show=False):
        self._served(FLOAT_OK, "the steady mode")
        self.steady = SD.check_settings(lo, hi, strength, radius, show)
        self.steady_state, self.steady_init, self.steady_last = None, True, None
        self._sync()

    def clear_steady(self):
        self.steady, self.steady_state, self.steady_init, self.steady_last = None, None, True, None
        self._sync()

    def set_output_size(self, height, width, resample="lanczos"):
        self._served(U8_TYPES, "an output size")
        ho, wo = RS.check_size(self.H, self.W, height, width)
        RS.check_filter(resample)
        if self.output_type == "jpeg":
            RS.check_jpeg_size(ho, wo)
        self.size = dict(height=ho, width=wo, resample=resample)
        self._sync()

    def clear_output_size(self):
        self.size = None
        self._sync()

    def set_detail(self, radius=2, eps=2.0, strength=1.0, limit=64.0, show=False):
        self._served(U8_TYPES, "the detail mode")
        self.detail = DT.check_settings(radius, eps, strength, limit, show)
        self._sync()

    def clear_detail(self):
        self.detail = None
        self._sync()

    def active(self):
        """the modes that are set (not: that act on the next output)"""
        on = dict(lock=self.lock, steady=self.steady, matte=self.matte, edge=self.edge if self.matte is not None else None,
                  size=self.size, detail=self.detail, camera=self.matte if self.matte_source == "camera" else None)
        return {k for k, v in on.items() if v is not None}

    # ------------------------------------------------------------------ the run
    def _entry(self, x, taps, what):
        """the check of (b) against the model's own frame, and the frame's entry (its camera frame computed here)"""
        assert len(taps) == 1, f"{what}: the tap saw {len(taps)} frames, the model expects 1"
        src, dn = taps[0]
        kind = kind_of(x)
        self._check_source(src, x, what)
        depth = (dn[-1, 0] if dn.ndim == 4 else dn[-1]).detach().cpu().to(torch.float16)
        e = _Entry(src[-1].detach().cpu().to(torch.float16), depth)
        if self.tap_key is not None and kind in ("u8", "jpeg"):
            raw = decode_ref(bytes(x)) if kind == "jpeg" else (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
            y0, x0, bh, bw = RS.camera_box(raw.shape[0], raw.shape[1], self.H, self.W)
            e.camera = resize_ref(np.ascontiguousarray(raw[y0:y0 + bh, x0:x0 + bw]), *self.tap_key)
            e.epoch = self.epoch
        return e

    def _check_source(self, src, x, what):
        """the recorded frame against the model's own expectation for input `x`"""
        want = self.source_of(x, kind_of(x))
        got = src[-1].detach().cpu().float()
        assert got.shape == want.shape, f"{what}: the tap's frame is {tuple(got.shape)}, the model's {tuple(want.shape)}"
        if self.source_tol == 0.0:
            assert torch.equal(got.to(torch.float16), want.to(torch.float16)), f"{what}: the tap's frame is not the model's frame"
        else:
            err = float((got - want.float()).abs().max())
            assert err <= self.source_tol, f"{what}: the tap's frame is {err:g} from the model's frame"

    def prepare(self, warm, primes):
        """`warm`: the warm-up frames; `primes`: what `TapRecorder.take_prime()` holds behind the wrapper's `prepare`"""
        self.lock_init, self.lock_last = True, None
        if self.lock is not None and self.lock["mode"] != "image":
            self.lock_state = None
        self.steady_state, self.steady_init, self.steady_last = None, True, None
        self.pending, self.last = [], None
        if self.line is None:
            assert not primes, "prepare: the tap was primed, the model has no line"
            return
        assert len(primes) == 1, f"prepare: the tap was primed {len(primes)} times, the model expects 1"
        self.line = _Line()
        x, dn = primes[0]
        self._check_source(x, warm[-1], "prepare")
        if self.n > 1:
            self.line.primed = _Entry(x[-1].detach().cpu().to(torch.float16), dn[-1, 0].detach().cpu().to(torch.float16))

    def _pair(self, line):
        """the pairing from first principles: output k of the line's accepted sequence belongs to its frame k - (N - 1)"""
        k = line.taken
        line.taken += 1
        own = k - (self.n - 1)
        if own >= 0:
            return line.entries[own], True
        if line.primed is not None:
            return line.primed, True
        return line.entries[0], False          # the oldest entry the line has: another frame's

    def frame(self, x, styled, taps):
        """an accepted `wrapper(x)`; `styled`: (a), the tensor the stream returned; `taps`: (b), `TapRecorder.take()`"""
        self.accepted += 1
        pair = None
        if self.line is not None:
            self.line.entries.append(self._entry(x, taps, f"frame {self.accepted - 1}"))
            self.line_starts += self.line.mid and len(self.line.entries) == 1
            pair = self.last = self._pair(self.line)
        else:
            assert not taps, f"frame {self.accepted - 1}: the tap saw a frame, the model has no line"
        return self._emit(styled, pair, repeated=False, ingest=self._ingest(x))

    def _ingest(self, x):
        """the launch the camera tap adds to the ingest of a uint8 frame or a JPEG file (also of a call the filter then refuses)"""
        return ["camera"] if self.tap_key is not None and kind_of(x) in ("u8", "jpeg") else []

    def drop(self, styled, taps=(), x=None):
        """a call the near-duplicate filter refused: `styled` is the stream's output of the call before"""
        assert not taps, "a dropped call reached the tap"
        return self._emit(styled, self.last if self.line is not None else None, repeated=True, ingest=self._ingest(x))

    def push(self, x, taps):
        self.accepted += 1
        if self.line is not None:
            self.line.entries.append(self._entry(x, taps, f"push {self.accepted - 1}"))
            self.line_starts += self.line.mid and len(self.line.entries) == 1
        else:
            assert not taps, f"push {self.accepted - 1}: the tap saw a frame, the model has no line"
        self.pending.append(self.line)

    def pop(self, styled):
        line = self.pending.pop(0)
        pair = None
        if self.line is not None and line is self.line:
            pair = self.last = self._pair(line)
        return self._emit(styled, pair, repeated=False)

    # ------------------------------------------------------------------ one output
    def _camera_of(self, entry):
        if entry is None or entry.camera is None or self.tap_key is None or entry.epoch != self.epoch:
            return None
        return entry.camera

    def _emit(self, styled, pair, repeated, ingest=()):
        ot = self.output_type
        entry, own = pair if pair is not None else (None, False)
        stages, acts = list(ingest), set()
        x = styled.detach().cpu() if torch.is_tensor(styled) else styled
        if self.lock is not None:
            self._served(FLOAT_OK, "a colour lock")
            if repeated and self.lock_last is not None:
                x = self.lock_last
                acts.add("lock")
            elif self.lock["mode"] == "source" and entry is None:
                pass
            else:
                lock = self.lock
                out, self.lock_state = lock_ref(x[:1], self.lock_state, mode=lock["mode"], strength=lock["strength"], rate=lock["rate"],
                                                   init=self.lock_init, source=entry.source if lock["mode"] == "source" else None)
                x = self.lock_last = torch.from_numpy(out)
                self.lock_init = False
                stages.append("lock")
                acts.add("lock")
        if self.steady is not None:
            self._served(FLOAT_OK, "the steady mode")
            if repeated and self.steady_last is not None:
                x = self.steady_last
                acts.add("steady")
            elif entry is None or not own:
                self.steady_init, self.steady_last = True, None
            else:
                out, self.steady_state = steady_ref(x[:1], entry.source, self.steady_state, init=self.steady_init, **self.steady)
                x = self.steady_last = torch.from_numpy(out)
                self.steady_init = False
                stages.append("steady")
                acts.add("steady")
        if self.size is not None:
            self._served(U8_TYPES, "an output size")
        if self.matte is not None:
            self._served(U8_TYPES, "a matte")
        if self.detail is not None:
            self._served(U8_TYPES, "the detail mode")
        if ot == "latent":
            return Expected(ot, x[0], stages, acts, repeated, own)
        if ot == "pt":
            return Expected(ot, (x / 2 + 0.5).clamp(0, 1)[0], stages, acts, repeated, own)
        if ot == "np":
            return Expected(ot, (x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().numpy()[0], stages, acts, repeated, own)
        assert ot in U8_TYPES, ot
        size, matte = self.size, self.matte
        if size is not None and ot == "jpeg":
            RS.check_jpeg_size(size["height"], size["width"])
        slot = entry if matte is not None else None
        camera = self._camera_of(slot) if self.device_route and self.matte_source == "camera" and size is not None else None
        sharpen = self._camera_of(entry) if self.device_route and self.detail is not None and size is not None and own else None
        x16 = x[:1].to(torch.float16)
        geo = (size["height"], size["width"], size["resample"]) if size is not None else None
        edge_kw = dict(edge=self.edge)
        if camera is not None:
            if sharpen is not None:
                u8 = detail_ref(x16[0].numpy(), entry.source, sharpen, *geo, **self.detail)
                stages += ["resize", "detail"]
                acts.add("detail")
            else:
                u8 = resize_ref(egress_ref(x16)[0].numpy(), *geo)
                stages.append("resize")
            u8 = composite_up_ref(u8, camera, slot.depth[None], **matte, source=slot.source[None] if self.edge is not None else None, **edge_kw)[0]
            stages += ["edge", "matte_up"] if self.edge is not None else ["matte_up"]
            acts |= {"matte", "camera", "size"} | ({"edge"} if self.edge is not None else set())
        else:
            frame = x16[0].numpy()                                    # what the resize reads: the fp16 frame, or the composite's bytes
            if slot is not None:
                frame = u8 = composite_ref(x16, slot.source[None], slot.depth[None], **matte, **edge_kw)[0]
                stages += ["edge", "matte"] if self.edge is not None else ["matte"]
                acts |= {"matte"} | ({"edge"} if self.edge is not None else set())
            else:
                u8 = egress_ref(x16)[0].numpy()
            if size is not None:
                if sharpen is not None:
                    u8 = detail_ref(frame, entry.source, sharpen, *geo, **self.detail)
                    stages += ["resize", "detail"]
                    acts.add("detail")
                else:
                    u8 = resize_ref(u8, *geo)
                    stages.append("resize")
                acts.add("size")
            elif slot is None and ot != "jpeg":
                stages.append("egress")
        if ot == "jpeg":
            stages.append("jpeg")
            return Expected(ot, encode_ref(u8, self.jpeg_quality), stages, acts, repeated, own)
        return Expected(ot, np.ascontiguousarray(u8), stages, acts, repeated, own)


# ----------------------------------------------------------------------------- the driver
class ChainMismatch(AssertionError):
    """an output of the wrapper that is not the model's (or an error only one of the two raised)"""


def same_output(a, b) -> bool:
    """two outputs of a wrapper, of any output type"""
    if isinstance(a, bytes) or isinstance(b, bytes):
        return isinstance(a, bytes) and isinstance(b, bytes) and a == b
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


class ChainRun:
    """Feeds one event script to a wrapper, to the model and (frames only) to a twin wrapper that never gets a mode, and
    compares every output: `ChainMismatch` at the first one that differs.  `filt` / `twin_filt`: the `DropFilter`s installed
    as the two streams' near-duplicate filters; `launches` (a list the device test's recording `OpList.run` appends the
    frame-op kinds to) and `stage_ops` ({stage: op kinds}): the launches of every output must be the model's stages mapped
    through it; `sync`: called before recorded tensors are read (the device test's synchronize)."""

    def __init__(self, w, model, rec, *, filt=None, twin=None, twin_filt=None, prompt="a prompt", launches=None, stage_ops=None, sync=None):
        self.w, self.m, self.rec, self.filt, self.twin, self.twin_filt, self.prompt = w, model, rec, filt, twin, twin_filt, prompt
        self.launches, self.stage_ops, self.sync = launches, stage_ops, sync or (lambda: None)
        self.calls = 0
        self.log = []                          # one `Expected` (or "raised") per output, in order
        self.compare_twin = False
        self.twin_got = None
        self.popped = []
        if getattr(w, "frame_pipelining", False):
            pop = w.stream.pop

            def keeping():
                x = pop()
                self.popped.append(x.clone())
                return x

            w.stream.pop = keeping

    def settings(self, name, *args, **kw):
        """`set_*` / `clear_*` on the wrapper and on the model: both raise ValueError, or neither"""
        errs = []
        for obj in (self.w, self.m):
            try:
                getattr(obj, name)(*args, **kw)
                errs.append(None)
            except ValueError as e:
                errs.append(e)
        if (errs[0] is None) != (errs[1] is None):
            raise ChainMismatch(f"{name}{args}{kw} under {self.m.output_type!r}: the wrapper raised {errs[0]!r}, the model {errs[1]!r}")
        return errs[0] is not None

    def output_type(self, ot):
        self.w.output_type = self.m.output_type = ot
        if self.twin is not None:
            self.twin.output_type = ot

    def prepare(self, warm):
        for obj in (self.w, self.twin):
            if obj is not None:
                torch.manual_seed(0)
                obj.prepare(warm, self.prompt)
        self.sync()
        self.rec.take()
        self.m.prepare(warm, self.rec.take_prime()[:1])        # (the twin has no line: the one record is the wrapper's)

    def _one(self, obj, filt, x, drop):
        if drop:
            filt.drop.add(filt.calls)
            obj.stream.inference_time_ema = 0.0                # (a dropped call waits that long)
        torch.manual_seed(7000 + self.calls)                   # (the host path draws its re-noising from the global generator)
        return obj(x)

    def _judge(self, label, got, werr, expect, ran=None):
        i = len(self.log)
        try:
            exp, merr = expect(), None
        except ValueError as e:
            exp, merr = None, e
        if (werr is None) != (merr is None):
            raise ChainMismatch(f"output {i} ({label}): the wrapper raised {werr!r}, the model {merr!r}")
        if werr is not None:
            self.log.append("raised")
            return None
        self.log.append(exp)
        bad = exp.differs(got)
        if bad is not None:
            raise ChainMismatch(f"output {i} ({label}, {exp.output_type}, stages {' '.join(exp.stages) or '-'}, set {sorted(self.m.active())}): {bad}")
        if ran is not None:
            want = tuple(op for stage in exp.stages for op in self.stage_ops[stage])
            if ran != want:
                raise ChainMismatch(f"output {i} ({label}): launched {' '.join(ran) or '-'}, the model's stages {' '.join(exp.stages) or '-'} are {' '.join(want) or '-'}")
        if self.compare_twin and not same_output(got, self.twin_got):
            raise ChainMismatch(f"output {i} ({label}): differs from the twin that never had a mode")
        return got

    def frame(self, x, drop=False):
        label = f"call {self.calls}{', dropped' if drop else ''}"
        got = werr = None
        if self.launches is not None:
            del self.launches[:]
        try:
            got = self._one(self.w, self.filt, x, drop)
        except ValueError as e:
            werr = e
        self.sync()
        ran = tuple(self.launches) if self.launches is not None else None
        styled, taps = self.w.stream.prev_image_result, self.rec.take()
        if self.twin is not None:
            self.twin_got = self._one(self.twin, self.twin_filt, x, drop)
            self.sync()
            self.rec.take()
        self.calls += 1
        return self._judge(label, got, werr, (lambda: self.m.drop(styled, taps, x)) if drop else (lambda: self.m.frame(x, styled, taps)), ran)

    def push(self, x):
        self.w.push(x)
        self.sync()
        self.m.push(x, self.rec.take())
        self.calls += 1

    def pop(self):
        got = werr = None
        if self.launches is not None:
            del self.launches[:]
        try:
            got = self.w.pop()
        except ValueError as e:
            werr = e
        self.sync()
        ran = tuple(self.launches) if self.launches is not None else None
        styled = self.popped.pop(0)
        assert not self.popped
        return self._judge(f"pop {len(self.log)}", got, werr, lambda: self.m.pop(styled), ran)

    def play(self, script):
        for ev in script:
            kind = ev[0]
            if kind == "set":
                self.settings(ev[1], *ev[2], **(ev[3] if len(ev) > 3 else {}))
            elif kind == "type":
                self.output_type(ev[1])
            elif kind == "prepare":
                self.prepare(ev[1])
            elif kind in ("frame", "drop"):
                self.frame(ev[1], drop=kind == "drop")
            elif kind == "push":
                self.push(ev[1])
            elif kind == "pop":
                self.pop()
            elif kind == "twin":
                self.compare_twin = True
            else:
                raise KeyError(kind)
        return self.log


def play_model_only(model, script, seed=0):
    """The script against the model alone, with synthetic stand-ins for what a run supplies -- (a) a random styled frame, (b) the
    model's own source with a random depth plane: which stages act on which output depends on neither, so the coverage
    conditions of a script can be computed (and its seeds chosen) without a wrapper.  Returns the log as `ChainRun.play` does."""
    g = torch.Generator().manual_seed(seed)
    H, W = model.H, model.W
    styled = lambda: (torch.randn(1, 3, H, W, generator=g) * 0.6).to(torch.float16)
    depth = lambda n=1: (torch.rand(n, 3, H, W, generator=g) * 2 - 1).to(torch.float16)
    taps = lambda x: [(model.source_of(x, kind_of(x))[None].to(torch.float16), depth())] if model.line is not None else []
    log, last, pops = [], None, []

    def out(fn):
        try:
            log.append(fn())
        except ValueError:
            log.append("raised")

    for ev in script:
        kind = ev[0]
        if kind == "set":
            try:
                getattr(model, ev[1])(*ev[2], **(ev[3] if len(ev) > 3 else {}))
            except ValueError:
                pass
        elif kind == "type":
            model.output_type = ev[1]
        elif kind == "prepare":
            warm = ev[1]
            model.prepare(warm, [(model.source_of(warm[-1], kind_of(warm[-1]))[None].to(torch.float16), depth())] if model.line is not None else [])
        elif kind == "frame":
            last = styled()
            out(lambda: model.frame(ev[1], last, taps(ev[1])))
        elif kind == "drop":
            out(lambda: model.drop(last, (), ev[1]))
        elif kind == "push":
            model.push(ev[1], taps(ev[1]))
        elif kind == "pop":
            out(lambda: model.pop(styled()))
        elif kind != "twin":
            raise KeyError(kind)
    return log
