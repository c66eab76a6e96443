"""Device-side uint8 frame I/O (csrc/frame_io.hip): camera-sized uint8 HWC frames in, uint8 HWC frames
out, one launch each way.

What the reference's callers do on the host around `wrapper(image)`:
  in:  torchvision `Resize(min(h, w), antialias=True)` + `CenterCrop((h, w))` on a [0, 1] tensor (test.py:106-112), then
       VaeImageProcessor's `2 x - 1`;
  out: `x / 2 + 0.5 -> clamp(0, 1) -> cpu -> permute -> float -> x 255 -> round -> uint8` (image_utils.py:9-37).
`geometry`, `aa_weights`, `ingest_ref` and `egress_ref` restate that arithmetic on CPU tensors (the tests pin them to torch and to
the reference, and the kernels to them); `HipFrameIO` owns the static buffers and the two one-op plans of one stream;
`FrameProcessor` is what goes into `stream.image_processor` so that the pipeline's `__call__` / `push` take raw uint8 frames.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

MAX_SCALE = 8.0        # frame_io.hip: 17 taps per axis


# ----------------------------------------------------------------------------- geometry and reference arithmetic (CPU)
def geometry(Hs: int, Ws: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(nh, nw, top, left): torchvision's `Resize(min(H, W))` + `CenterCrop((H, W))` on tensors -- the short side of the source
    becomes min(H, W), the long side `int(s * long / short)`, and the crop window sits at `int(round((n - size) / 2))`.  A window
    that does not lie inside the resized image (torchvision would zero-pad) raises ValueError."""
    s = min(H, W)
    if Hs <= Ws:
        nh, nw = s, int(s * Ws / Hs)
    else:
        nh, nw = int(s * Hs / Ws), s
    top, left = int(round((nh - H) / 2.0)), int(round((nw - W) / 2.0))
    if top < 0 or left < 0 or top + H > nh or left + W > nw:
        raise ValueError(f"frame geometry {Hs}x{Ws} -> {H}x{W}: the {H}x{W} crop window does not lie inside the resized image "
                         f"{nh}x{nw} (zero-padding crops are not supported)")
    return nh, nw, top, left


def aa_weights(n_in: int, n_out: int, dtype=torch.float32):
    """(xmin int64 [n_out], weights [n_out, taps]) of torch's antialiased bilinear filter along one axis
    (`F.interpolate(mode="bilinear", align_corners=False, antialias=True)`): scale = n_in / n_out, support = max(scale, 1),
    c = scale (i + 0.5), taps [max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))),
    w_j = max(0, 1 - |(j + xmin - c + 0.5) / support|), normalised to sum 1 (taps beyond a row's own count are 0)."""
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    support = torch.clamp(scale, min=1.0)
    inv = 1.0 / support
    c = scale * (torch.arange(n_out, dtype=dtype) + 0.5)
    xmin = (c - support + 0.5).to(torch.int64).clamp_(min=0)
    xmax = (c + support + 0.5).to(torch.int64).clamp_(max=n_in)
    taps = int((xmax - xmin).max())
    j = torch.arange(taps, dtype=torch.int64)[None]
    w = (1.0 - ((j + xmin[:, None]).to(dtype) - c[:, None] + 0.5).mul(inv).abs()).clamp_(min=0.0)
    w = torch.where(j < (xmax - xmin)[:, None], w, torch.zeros((), dtype=dtype))
    return xmin, w / w.sum(1, keepdim=True)


def _dense(n_in: int, n_out: int, first: int, count: int, dtype) -> torch.Tensor:
    """rows [first, first + count) of the resize as a dense [count, n_in] matrix"""
    xmin, w = aa_weights(n_in, n_out, dtype)
    xmin, w = xmin[first:first + count], w[first:first + count]
    m = torch.zeros(count, n_in + w.shape[1], dtype=dtype)
    m.scatter_(1, xmin[:, None] + torch.arange(w.shape[1])[None], w)
    return m[:, :n_in]


def ingest_ref(frames, H: int, W: int, dtype=torch.float32) -> torch.Tensor:
    """uint8 [B,Hs,Ws,3] (or [Hs,Ws,3]) -> [B,3,H,W] in [-1, 1]: `2 crop(resize(u8)) / 255 - 1`, both axes in `dtype`, no
    intermediate rounding (what the ingest kernel computes before its single rounding to fp16)."""
    x = torch.as_tensor(np.asarray(frames) if not torch.is_tensor(frames) else frames.cpu())
    if x.ndim == 3:
        x = x[None]
    B, Hs, Ws, _ = x.shape
    nh, nw, top, left = geometry(Hs, Ws, H, W)
    my, mx = _dense(Hs, nh, top, H, dtype), _dense(Ws, nw, left, W, dtype)
    out = torch.empty(B, 3, H, W, dtype=dtype)
    for b in range(B):
        img = x[b].permute(2, 0, 1).to(dtype)                       # [3,Hs,Ws]
        out[b] = torch.matmul(my, torch.matmul(img, mx.t()))
    return 2.0 * (out / 255.0) - 1.0


def egress_ref(x: torch.Tensor) -> torch.Tensor:
    """fp16 [B,3,H,W] (or [3,H,W]) -> uint8 [B,H,W,3] exactly as the reference computes it: `(x / 2 + 0.5).clamp(0, 1)` on the fp16
    tensor (a rounding to fp16 after each step, image_utils.py:13), then `(v.float() * 255).round()` -- half to even -- as uint8
    (:30)."""
    x = x.detach().cpu().to(torch.float16)
    if x.ndim == 3:
        x = x[None]
    v = (x * 0.5 + 0.5).clamp(0, 1)                                 # two fp16 tensor ops, each rounds
    return (v.permute(0, 2, 3, 1).float() * 255.0).round().to(torch.uint8).contiguous()


def frame16(x, prefix: str, what: str = "frame") -> np.ndarray:
    """fp16 [3,H,W] of a [3,H,W] or [1,3,H,W] array / tensor, for the oracles of the output chain; `prefix` names the caller in
    the error"""
    if torch.is_tensor(x):
        x = x.detach().cpu().to(torch.float16).numpy()
    x = np.asarray(x, dtype=np.float16)
    if not x.flags.writeable:
        x = x.copy()                       # (torch.from_numpy refuses to share a read-only array quietly)
    if x.ndim == 4 and x.shape[0] == 1:
        x = x[0]
    if x.ndim != 3 or x.shape[0] != 3:
        raise ValueError(f"{prefix}: expected one [3,H,W] {what}, got {x.shape}")
    return x


# ----------------------------------------------------------------------------- the device side
def to_pinned(dev: torch.Tensor, host: torch.Tensor) -> np.ndarray:
    """a static device buffer copied into its pinned twin on the current stream and waited for: the numpy view of the pinned
    buffer, valid until the next copy into it (the end of `HipFrameIO.egress`, `HipMatte.composite` and `HipResize.resize`)"""
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


class _Slot:
    def __init__(self, Hs, Ws, H, W, device):
        self.staging = torch.empty(Hs, Ws, 3, dtype=torch.uint8).pin_memory()
        self.dev_u8 = torch.empty(1, Hs, Ws, 3, dtype=torch.uint8, device=device)
        self.out = torch.empty(1, 3, H, W, dtype=torch.float16, device=device)
        self.uploaded: Optional[torch.cuda.Event] = None    # behind the last H2D copy out of `staging`
        self.released = None                                # the caller's event behind the last reader of `out` (release())
        self.plan = None                                    # dev_u8 -> out


class HipFrameIO:
    """Static buffers and plans for one `(Hs, Ws) -> (H, W)` stream.  Everything runs on `torch.cuda.current_stream()`.

    A single ingested frame lands in one of TWO slots used in turn; the returned fp16 tensor is a view of the slot, valid until
    the ingest after the next.  A consumer on another stream hands the event behind its last read to `release(view, event)`;
    the next ingest into that slot makes the current stream wait for it.  A batch (B > 1) gets fresh tensors."""

    def __init__(self, height: int, width: int, device="cuda:0"):
        if width % 8 or (height * width) % 16:
            raise ValueError(f"HipFrameIO: width {width} must be a multiple of 8 and height * width a multiple of 16")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self._src = None                   # (Hs, Ws) the slots are planned for
        self._geo = None
        self._slots = []
        self._turn = 0
        self._egress = {}                  # B -> (device uint8, pinned uint8)
        self.last_view = None              # what the last single-frame ingest returned (for release())
        self._device_plans = {}            # (source pointer, slot) -> plan: device frames out of static buffers (jpeg_io.HipJpegDecoder)
        self._device_seen = ()             # the last four source pointers of device frames (integers: nothing is kept alive)
        # Optional hook (resize.CameraTap), single frames only: `camera_tap.prepare(Hs, Ws)` in front of everything a frame
        # launches (it may refuse the geometry), `camera_tap(src)` behind the ingest launch on the same stream, with the device
        # uint8 [1,Hs,Ws,3] source that was just ingested.  None: nothing changes.
        self.camera_tap = None

    # ------------------------------------------------------------------ ingest
    def _plan_source(self, Hs: int, Ws: int):
        self._geo = geometry(Hs, Ws, self.height, self.width)
        nh, nw = self._geo[:2]
        if Hs / nh > MAX_SCALE or Ws / nw > MAX_SCALE:
            raise ValueError(f"frame geometry {Hs}x{Ws} -> {self.height}x{self.width}: down-scale above {MAX_SCALE:g}")
        self._src = (Hs, Ws)
        self._slots = [_Slot(Hs, Ws, self.height, self.width, self.device) for _ in range(2)]
        self._turn = 0
        self._device_plans.clear()

    def _ingest_op(self, src, dst, B):
        (Hs, Ws), (nh, nw, top, left) = self._src, self._geo
        pl = _lib.OpList()
        op, keep = ops.frame_ingest(src, dst, B=B, Hs=Hs, Ws=Ws, H=self.height, W=self.width, nh=nh, nw=nw, top=top, left=left)
        pl.append(op, *keep)
        return pl

    def ingest(self, frame) -> torch.Tensor:
        """np.uint8 / torch.uint8 [Hs,Ws,3] or [B,Hs,Ws,3], on the host or already on the device -> fp16 [B,3,H,W] in [-1, 1]"""
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if frame.dtype != torch.uint8 or frame.ndim not in (3, 4) or frame.shape[-1] != 3:
            raise ValueError(f"ingest: expected uint8 [Hs,Ws,3] or [B,Hs,Ws,3], got {frame.dtype} {tuple(frame.shape)}")
        if frame.ndim == 3:
            frame = frame[None]
        if not frame.is_contiguous():
            frame = frame.contiguous()
        B, Hs, Ws, _ = frame.shape
        if self._src != (Hs, Ws):
            self._plan_source(Hs, Ws)
        if B > 1:
            src = frame if frame.is_cuda else frame.to(self.device, non_blocking=True)
            out = torch.empty(B, 3, self.height, self.width, dtype=torch.float16, device=self.device)
            self._ingest_op(src, out, B).run()
            return out
        if self.camera_tap is not None:
            self.camera_tap.prepare(Hs, Ws)
        slot = self._slots[self._turn]
        self._turn ^= 1
        cur = torch.cuda.current_stream()
        if slot.released is not None:
            cur.wait_event(slot.released)
            slot.released = None
        if frame.is_cuda:
            src = frame
        else:
            if slot.uploaded is not None:
                slot.uploaded.synchronize()          # the copy out of this staging buffer two frames ago (long done)
            slot.staging.copy_(frame[0])
            slot.dev_u8[0].copy_(slot.staging, non_blocking=True)
            slot.uploaded = slot.uploaded or torch.cuda.Event()
            slot.uploaded.record(cur)
            src = slot.dev_u8
        if src is slot.dev_u8:
            plan = slot.plan = slot.plan or self._ingest_op(src, slot.out, 1)
        else:
            # a caller's device frame.  A producer with static outputs (the JPEG decoder's two slots) meets its plan again: a source
            # pointer seen before gets its plan kept, at most four (two sources x two ingest slots; a kept plan keeps its source
            # alive, so its pointer cannot become another tensor's).  A pointer seen for the first time fills one record, as before.
            ptr = src.data_ptr()
            key = (ptr, self._turn)
            plan = self._device_plans.get(key)
            if plan is None:
                plan = self._ingest_op(src, slot.out, 1)
                if ptr in self._device_seen:
                    if len(self._device_plans) >= 4:
                        self._device_plans.clear()
                    self._device_plans[key] = plan
                self._device_seen = (self._device_seen + (ptr,))[-4:]
        plan.run()
        if self.camera_tap is not None:
            self.camera_tap(src)
        self.last_view = slot.out
        return slot.out

    def release(self, slot_view: torch.Tensor, event) -> None:
        """`event` was recorded behind the last read of `slot_view` (a tensor `ingest` returned) on another stream"""
        for slot in self._slots:
            if slot.out.data_ptr() == slot_view.data_ptr():
                slot.released = event
                return
        raise ValueError("release: not a view of an ingest slot")

    # ------------------------------------------------------------------ egress
    def egress(self, image: torch.Tensor, to_host: bool = True):
        """fp16 [3,H,W] / [B,3,H,W] in [-1, 1] on the device -> uint8 [H,W,3] / [B,H,W,3]: a numpy view of the pinned buffer (valid
        until the next egress of the same batch size), or with `to_host=False` the static device tensor."""
        if image.dtype != torch.float16 or not image.is_cuda:
            raise ValueError(f"egress: expected a device fp16 tensor, got {image.dtype} on {image.device}")
        single = image.ndim == 3
        if single:
            image = image[None]
        if tuple(image.shape[1:]) != (3, self.height, self.width):
            raise ValueError(f"egress: expected [B,3,{self.height},{self.width}], got {tuple(image.shape)}")
        if not image.is_contiguous():
            image = image.contiguous()
        B = image.shape[0]
        bufs = self._egress.get(B)
        if bufs is None:
            bufs = self._egress[B] = (torch.empty(B, self.height, self.width, 3, dtype=torch.uint8, device=self.device),
                                      torch.empty(B, self.height, self.width, 3, dtype=torch.uint8).pin_memory())
        dev, host = bufs
        op, _ = ops.frame_egress(image, dev, B=B, H=self.height, W=self.width)
        pl = _lib.OpList()
        pl.append(op)
        pl.run()
        if not to_host:
            return dev[0] if single else dev
        arr = to_pinned(dev, host)
        return arr[0] if single else arr


class _PassThrough:
    """`preprocess(x, ...) -> x[None]`: for callers that hand the pipeline an already ingested [3,H,W] frame"""

    @staticmethod
    def preprocess(image, height: int, width: int) -> torch.Tensor:
        return image[None] if image.ndim == 3 else image


class FrameProcessor:
    """What `StreamAnimateDiffusionDepth.image_processor` becomes: uint8 frames go through the ingest kernel, float tensors take
    `_ImageProcessor(assume_unit_range=True)` (the reference's callers feed [0, 1]; no `.min()` sync)."""

    def __init__(self, io: HipFrameIO):
        from .pipeline_stream_animation_depth import _ImageProcessor
        self.io = io
        self._float = _ImageProcessor(assume_unit_range=True)

    def preprocess(self, image, height: int, width: int) -> torch.Tensor:
        dt = image.dtype
        if dt == torch.uint8 or dt == np.uint8:
            assert (height, width) == (self.io.height, self.io.width)
            return self.io.ingest(image)
        return self._float.preprocess(image, height, width)
