"""The matte from the caller (csrc/mask_in.hip): a mask of a person segmenter or a keyer in the
caller's own process, or a hand-drawn region -- uint8, uint16, bool or float32, of any size, on the host or on the device -> the
raw matte plane of the output chain, fp32 [H,W] in [0, 1] at the stream's size, in place of the smoothstep ramp over the frame's
depth or combined with it.  Everything behind the raw matte (edge refit, hold, feather, backdrop, both composites, `show`) reads
the plane as it reads the ramp.  The reference has no counterpart.

`mask_ref` and `front_ref` (numpy) state the arithmetic: every product, sum and quotient rounded to fp32 on its own, no fma.
They are the oracle of L2D_OP_MASK_INGEST, bit for bit, and what the wrapper computes on CPU tensors.  The resampling is
`depth_io`'s -- the same tables, the same tap loop -- so a mask covers the field of view the colour and depth ingests look at.
`HipMaskIngest` owns the tables, the pool of raw-mask buffers and the plane of one stream.

The mask is quantised to byte levels at the stream's size (P = rint(255 r)): a constant mask comes back exactly 0 or 1 whatever
the weights' rounding, the integers the edge refit and the backdrop form of the plane are P itself, and min / max are exact."""
import os
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from . import depth_io
from .depth_io import _taps

COMBINES = ("replace", "and", "or")
DEFAULTS = dict(combine="replace", invert=False)
IMAGE_MODES = ("L", "1", "I;16", "I;16L", "I;16B", "F")


# ----------------------------------------------------------------------------- settings
def check_settings(combine="replace", invert=False) -> dict:
    """{combine, invert} validated; ValueError names the keyword"""
    if not isinstance(combine, str) or combine not in COMBINES:
        raise ValueError(f"mask input: combine={combine!r}: use 'replace' (the mask alone), 'and' (ramp and mask) or 'or'")
    if not isinstance(invert, (bool, np.bool_)):
        raise ValueError(f"mask input: invert={invert!r}: use True or False")
    return dict(combine=combine, invert=bool(invert))


# ----------------------------------------------------------------------------- geometry and containers
def tables(Hm: int, Wm: int, H: int, W: int):
    """`depth_io.tables` of a mask's own size: ((nh, nw, top, left), ymin, wy, xmin, wx); ValueError with the prefix `mask:` for
    a geometry `frame_io.geometry`, MAX_SCALE or the tap limit refuses"""
    try:
        return depth_io.tables(Hm, Wm, H, W)
    except ValueError as e:
        msg = str(e)
        raise ValueError("mask: " + (msg[len("depth: "):] if msg.startswith("depth: ") else msg)) from None


def load(mask, where: str = "mask"):
    """a `mask=` argument as `_as_mask` / `_torch_mask` take it: arrays and tensors pass, a PIL image of mode "L", "1", "I;16" or
    "F" -- or a path to one -- becomes its array"""
    if isinstance(mask, (str, os.PathLike)):
        from PIL import Image
        try:
            with Image.open(mask) as im:
                im.load()
                mask = im.copy()
        except (OSError, SyntaxError, EOFError) as e:
            raise ValueError(f"{where}: {mask!r} cannot be read as an image: {e}") from None
    if hasattr(mask, "mode") and hasattr(mask, "convert"):
        if mask.mode not in IMAGE_MODES:
            raise ValueError(f"{where}: a mask image must have mode 'L', '1', 'I;16' or 'F', got {mask.mode!r}")
        arr = np.array(mask)
        if mask.mode.startswith("I;16"):
            arr = arr.astype(np.uint16)
        return arr
    return mask


def _as_mask(mask) -> np.ndarray:
    """[Hm,Wm], numpy or torch, -> a contiguous uint8, uint16 or float32 array (bool -> 0 / 255, fp16 widened exactly)"""
    if torch.is_tensor(mask):
        mask = mask.detach().cpu()
        # (a torch int16 tensor holds the bits of uint16 samples, as in depth_io: not every torch build copies uint16)
        mask = mask.view(torch.int16).numpy().view(np.uint16) if mask.dtype in (torch.uint16, torch.int16) else mask.numpy()
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8) * np.uint8(255)
    elif m.dtype == np.float16:
        m = m.astype(np.float32)
    if m.dtype not in (np.uint8, np.uint16, np.float32):
        raise ValueError(f"mask: expected uint8, uint16, bool or float32 samples (float16 is widened), got {m.dtype}")
    if m.ndim != 2 or 0 in m.shape:
        raise ValueError(f"mask: expected [Hm,Wm], got {tuple(m.shape)}")
    return np.ascontiguousarray(m)


def _torch_mask(mask) -> torch.Tensor:
    """a mask as a contiguous uint8, int16 (the bits of uint16 samples) or float32 [Hm,Wm] torch tensor; a device tensor stays
    where it is"""
    if torch.is_tensor(mask) and mask.is_cuda:
        m = mask
        if m.dtype == torch.bool:
            m = m.to(torch.uint8) * 255
        elif m.dtype == torch.float16:
            m = m.float()
        elif m.dtype == torch.uint16:
            m = m.view(torch.int16)
        if m.dtype not in (torch.uint8, torch.int16, torch.float32):
            raise ValueError(f"mask: expected uint8, uint16, bool or float32 samples (float16 is widened), got {mask.dtype}")
        if m.ndim != 2 or 0 in m.shape:
            raise ValueError(f"mask: expected [Hm,Wm], got {tuple(m.shape)}")
        return m if m.is_contiguous() else m.contiguous()
    m = _as_mask(mask)
    return torch.from_numpy(m.view(np.int16) if m.dtype == np.uint16 else m)


# ----------------------------------------------------------------------------- the oracle (numpy)
def unit_ref(mask) -> np.ndarray:
    """fp32 v in [0, 1] of the samples: uint8 float(s) / 255, uint16 float(s) / 65535 (one correctly rounded division each),
    floats min(max(x, 0), 1) with NaN -> 0"""
    m = _as_mask(mask)
    if m.dtype == np.uint8:
        return m.astype(np.float32) / np.float32(255.0)
    if m.dtype == np.uint16:
        return m.astype(np.float32) / np.float32(65535.0)
    with np.errstate(invalid="ignore"):
        v = np.minimum(np.maximum(m, np.float32(0.0)), np.float32(1.0))
    return np.where(np.isnan(m), np.float32(0.0), v).astype(np.float32)


def mask_ref(mask, H: int, W: int, invert: bool = False) -> np.ndarray:
    """uint8 [H,W] plane P: the mask resampled over `frame_io.geometry(Hm, Wm, H, W)` with the fp32 weights of
    `frame_io.aa_weights` -- r = sum_y wy (sum_x wx v), the horizontal pass first, taps ascending, every product and sum rounded
    to fp32 --, P = rint(255 min(max(r, 0), 1)), half to even; `invert`: 255 - P"""
    v = unit_ref(mask)
    _, ymin, wy, xmin, wx = tables(v.shape[0], v.shape[1], H, W)
    ymin, wy, xmin, wx = ymin.numpy().astype(np.int64), wy.numpy(), xmin.numpy().astype(np.int64), wx.numpy()
    r = _taps(_taps(v, xmin, wx, 1), ymin, wy, 0)
    assert r.dtype == np.float32
    c = np.minimum(np.maximum(r, np.float32(0.0)), np.float32(1.0))
    P = np.ascontiguousarray(np.rint(np.float32(255.0) * c).astype(np.uint8))      # (`_taps` leaves a transposed layout)
    return (np.uint8(255) - P) if invert else P


def front_ref(P, depth, lo: float, hi: float, keep: str = "near", combine: str = "replace") -> np.ndarray:
    """fp32 [H,W] raw matte m0 of the byte plane P (`mask_ref`): mu = float(P) / 255; "replace": mu; "and": min(m_r, mu); "or":
    max(m_r, mu) with m_r = `matte.matte_ref(depth, lo, hi, 0, keep)`, the ramp and `keep` without a feather.  "replace" reads
    neither `depth` nor the ramp."""
    from .matte import matte_ref
    check_settings(combine)
    P = np.asarray(P)
    if P.dtype != np.uint8 or P.ndim != 2:
        raise ValueError(f"front_ref: expected a uint8 [H,W] plane, got {P.dtype} {P.shape}")
    mu = P.astype(np.float32) / np.float32(255.0)
    if combine == "replace":
        return mu
    mr = matte_ref(depth, lo, hi, 0, keep)
    if mr.shape != (1,) + P.shape:
        raise ValueError(f"front_ref: the mask plane is {P.shape}, the depth plane {mr.shape[1:]}")
    return (np.minimum(mr[0], mu) if combine == "and" else np.maximum(mr[0], mu)).astype(np.float32)


def raw_ref(mask, depth, matte: dict, mask_input: dict, H: int, W: int) -> np.ndarray:
    """fp32 [H,W]: `front_ref(mask_ref(...))` under the matte's and the mask input's settings -- op 58 on the host"""
    return front_ref(mask_ref(mask, H, W, mask_input["invert"]), depth, matte["lo"], matte["hi"], matte["keep"], mask_input["combine"])


# ----------------------------------------------------------------------------- the host side of the delay line
class HostMaskTap:
    """`MatteLine.mask_source` on CPU tensors: `offer` validates a mask against the stream's size and holds its array as
    `pending`; nothing is pooled"""

    def __init__(self, height: int, width: int):
        self.height, self.width = int(height), int(width)
        self.pending = None

    def begin(self) -> None:
        self.pending = None

    def give_back(self, buf) -> None:
        pass

    def offer(self, mask) -> None:
        m = _as_mask(mask).copy()
        tables(m.shape[0], m.shape[1], self.height, self.width)
        self.pending = m


# ----------------------------------------------------------------------------- the device side
class MaskBuffer:
    """one raw mask on the device: a byte buffer out of the pool, its pinned twin for a host mask, and the (Hm, Wm, dtype) of
    what it holds now"""

    def __init__(self, nbytes: int, device):
        self.nbytes = int(nbytes)
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.host = None                    # pinned, made by the first host mask that lands here
        self.uploaded = None                # behind the last H2D copy out of `host`
        self.shape = self.dtype = None
        self.shared = False                 # a sticky mask's buffer: many slots name it, and it never goes back to the pool

    def view(self) -> torch.Tensor:
        Hm, Wm = self.shape
        return self.dev[:Hm * Wm * self.dtype.itemsize].view(self.dtype).view(Hm, Wm)


class HipMaskIngest:
    """Tables, raw-mask buffers and the raw matte plane of one `(H, W)` stream, and `MatteLine.mask_source` on the device.

    `offer(mask)` copies the raw mask into a pooled device buffer on `torch.cuda.current_stream()` -- a plain copy, H2D through
    a pinned twin or D2D: a caller's device mask is never read in place later, because it is needed N - 1 frames on -- and holds
    the buffer as `pending`.  `MatteLine._store` moves `pending` into the frame's slot and gives the slot's previous buffer back
    (`give_back`); `begin` (the wrapper, in front of every frame) takes back a `pending` nobody claimed, e.g. that of a frame the
    near-duplicate filter dropped.  `record(buffer, depth, matte, mask_input)` is the record of L2D_OP_MASK_INGEST that writes
    `plane`; the composites put it at the head of their `OpList`.  The rule that keeps camera buffers safe without events of
    their own covers these too: the copy in `offer` and every launch that reads a buffer run on the caller's stream, so a
    buffer that went back to the pool is overwritten only behind its last reader.  Tables are kept per mask geometry (at most
    `MAX_TABLES`); the pool grows with the delay line's ring and allocates nothing in steady state."""

    MAX_TABLES = 4

    def __init__(self, height: int, width: int, device="cuda:0"):
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.plane = torch.empty(self.height, self.width, dtype=torch.float32, device=self.device)
        self.pending: Optional[MaskBuffer] = None
        self.free = []
        self.allocated = 0
        self._tables = {}                   # (Hm, Wm) -> (geometry, device tables in the record's order)

    def geometry(self, Hm: int, Wm: int):
        hit = self._tables.get((Hm, Wm))
        if hit is None:
            geo, ymin, wy, xmin, wx = tables(Hm, Wm, self.height, self.width)
            if len(self._tables) >= self.MAX_TABLES:
                self._tables.clear()
            hit = self._tables[(Hm, Wm)] = (geo, tuple(t.to(self.device) for t in (xmin, wx, ymin, wy)))
        return hit

    def begin(self) -> None:
        """in front of a frame: a `pending` buffer nobody claimed goes back to the pool"""
        if self.pending is not None:
            self.give_back(self.pending)
            self.pending = None

    def give_back(self, buf) -> None:
        if isinstance(buf, MaskBuffer) and not buf.shared:
            self.free.append(buf)

    def _buffer(self, nbytes: int) -> MaskBuffer:
        for i, b in enumerate(self.free):
            if b.nbytes >= nbytes:
                return self.free.pop(i)
        self.allocated += 1
        return MaskBuffer(nbytes, self.device)

    def stage(self, mask, shared: bool = False) -> MaskBuffer:
        """the raw mask in a device buffer (out of the pool, or with `shared` one of its own), copied on the current stream"""
        m = _torch_mask(mask)
        Hm, Wm = m.shape
        self.geometry(Hm, Wm)                                # (a geometry the ingest refuses raises here, before anything is copied)
        nbytes = Hm * Wm * m.element_size()
        buf = MaskBuffer(nbytes, self.device) if shared else self._buffer(nbytes)
        buf.shared, buf.shape, buf.dtype = shared, (Hm, Wm), m.dtype
        dst = buf.view()
        if m.is_cuda:
            dst.copy_(m, non_blocking=True)
        elif ops.DRY_RUN:
            dst.copy_(m)
        else:
            if buf.host is None:
                buf.host = torch.empty(buf.nbytes, dtype=torch.uint8).pin_memory()
            if buf.uploaded is not None:
                buf.uploaded.synchronize()                   # the copy out of this pinned buffer a ring ago (long done)
            host = buf.host[:nbytes].view(m.dtype).view(Hm, Wm)
            host.copy_(m)
            dst.copy_(host, non_blocking=True)
            buf.uploaded = buf.uploaded or torch.cuda.Event()
            buf.uploaded.record(torch.cuda.current_stream())
        return buf

    def offer(self, mask) -> None:
        self.pending = mask if isinstance(mask, MaskBuffer) else self.stage(mask)

    def record(self, buf: MaskBuffer, depth: Optional[torch.Tensor], matte: dict, mask_input: dict, out: Optional[torch.Tensor] = None):
        """(record, tensors to keep) of L2D_OP_MASK_INGEST: `buf` under the matte's ramp and the mask input's settings -> `plane`"""
        from .matte import matte_params
        s = check_settings(mask_input["combine"], mask_input["invert"])
        Hm, Wm = buf.shape
        (nh, nw, top, left), tabs = self.geometry(Hm, Wm)
        kw = {}
        if s["combine"] != "replace":
            lo32, inv32, hard = matte_params(matte["lo"], matte["hi"])
            kw = dict(lo32=lo32, inv32=inv32, hard=hard, far=matte["keep"] == "far")
        return ops.mask_ingest(buf.view(), self.plane if out is None else out, depth, *tabs, Hm=Hm, Wm=Wm, H=self.height, W=self.width,
                               nh=nh, nw=nw, top=top, left=left, combine=s["combine"], invert=s["invert"], **kw)

    def ingest(self, mask, depth: Optional[torch.Tensor], matte: dict, mask_input: dict, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one mask -> the raw matte plane, in one run on the current stream (tests and tools; the wrapper goes through `offer`,
        the delay line and `record`); the buffer goes back to the pool behind the launch"""
        buf = self.stage(mask)
        pl = _lib.OpList()
        op, keep = self.record(buf, depth, matte, mask_input, out)
        pl.append(op, *keep)
        pl.run()
        self.give_back(buf)
        return self.plane if out is None else out
