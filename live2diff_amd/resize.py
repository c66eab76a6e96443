"""Output size (csrc/resize.hip): the uint8 frame resampled to a size of the caller's choice on the device,
behind the colour lock and the matte and in front of the JPEG encoder or the copy to the host.  The arithmetic is Pillow's
`Image.resize` on 8-bit images: per axis a table of 22-bit fixed-point coefficients built in fp64, a horizontal pass and a
vertical pass in 32-bit integers, each rounded and clipped to a uint8 image of its own.

  * `coefficients`, `resize_pass`, `resize_ref`   the arithmetic of L2D_OP_FRAME_RESIZE in numpy integers -- the kernel's oracle,
                      as `matte.composite_ref` and `jpeg.encode_ref` are; `resize_ref` equals Pillow byte for byte;
  * `check_size`, `check_filter`   the served geometries and the argument checks of `set_output_size`;
  * `HipResize`       the device tables, the static output buffers and the one-op plans of one geometry;
  * `camera_box`, `CameraTap`   the matte at the output size: the window of the camera frame the ingest
                      looks at, and the hook of `HipFrameIO.ingest` that resamples it to the output size as the frame comes in.
"""
import math
from typing import Tuple

import numpy as np
import torch

from . import _lib, ops
from .frame_io import geometry, to_pinned

SERVED_OUTPUT_TYPES = ("u8", "pil", "jpeg")
PRECISION_BITS = 22                      # 32 - 8 - 2: a byte times a coefficient of up to 2 in a signed 32-bit accumulator
MAX_KS = ops.RESIZE_MAX_KS               # taps per output pixel: Lanczos (support 3) at a 2x down-scale, 2 * 6 + 1
MAX_SIZE = ops.RESIZE_MAX_SIZE


# ----------------------------------------------------------------------------- filters
def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"lanczos": (3.0, _lanczos), "bicubic": (2.0, _bicubic), "bilinear": (1.0, _bilinear)}


def check_filter(resample) -> str:
    if resample not in FILTERS:
        raise ValueError(f"output size: resample={resample!r}: use one of " + ", ".join(repr(f) for f in FILTERS))
    return resample


# ----------------------------------------------------------------------------- reference arithmetic (CPU, Python floats and numpy integers)
def coefficients(n_in: int, n_out: int, resample: str = "lanczos") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One axis: (xmin int32 [n_out], count int32 [n_out], k int32 [n_out][KS]).  Output index xx reads input
    xmin[xx] .. xmin[xx] + count[xx] - 1 with the weights k[xx][:count[xx]], normalised in fp64 and rounded half away from zero
    to 22 fractional bits; the taps behind `count` are 0.  Every row is asserted to keep a byte sum inside a signed 32-bit
    accumulator: 255 sum |k| + 2^21 < 2^31."""
    support, f = FILTERS[check_filter(resample)]
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = support * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    k = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        w = [f((x + lo - c + 0.5) * ss) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS)) for v in w]
        assert 255 * sum(abs(v) for v in row) + (1 << (PRECISION_BITS - 1)) < 1 << 31, (n_in, n_out, resample, xx)
        xmin[xx], count[xx] = lo, hi - lo
        k[xx, :hi - lo] = row
    return xmin, count, k


def pass_sums(a: np.ndarray, axis: int, table) -> np.ndarray:
    """the unclipped, unshifted sums 2^21 + sum_x in[lo + x] k[xx][x] of one pass along `axis`, int64 (they fit int32)"""
    xmin, count, k = table
    a = np.moveaxis(np.asarray(a), axis, -1).astype(np.int64)
    out = np.empty(a.shape[:-1] + (len(xmin),), np.int64)
    for xx in range(len(xmin)):
        lo, n = int(xmin[xx]), int(count[xx])
        out[..., xx] = (a[..., lo:lo + n] * k[xx, :n].astype(np.int64)).sum(-1) + (1 << (PRECISION_BITS - 1))
    assert np.abs(out).max(initial=0) < 1 << 31
    return np.moveaxis(out, -1, axis)


def resize_pass(a: np.ndarray, axis: int, table) -> np.ndarray:
    """one pass: clip((2^21 + sum) >> 22, 0, 255) with an arithmetic shift, as a uint8 image"""
    return np.clip(pass_sums(a, axis, table) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_ref(image, out_height: int, out_width: int, resample: str = "lanczos") -> np.ndarray:
    """L2D_OP_FRAME_RESIZE on the host, and Pillow's `Image.resize((out_width, out_height), resample)` byte for byte: uint8
    [H,W,3] or [B,H,W,3] -> uint8 [Ho,Wo,3] or [B,Ho,Wo,3].  The horizontal pass first, then the vertical pass on its uint8
    result; an axis whose size does not change is skipped."""
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"resize_ref: expected uint8 [H,W,3] or [B,H,W,3], got {a.dtype} {a.shape}")
    check_filter(resample)
    H, W = a.shape[-3], a.shape[-2]
    if int(out_width) != W:
        a = resize_pass(a, a.ndim - 2, coefficients(W, out_width, resample))
    if int(out_height) != H:
        a = resize_pass(a, a.ndim - 3, coefficients(H, out_height, resample))
    return np.ascontiguousarray(a)


def check_size(height: int, width: int, out_height, out_width, batch: int = 1) -> Tuple[int, int]:
    """(Ho, Wo) as ints, or ValueError naming the rule: per axis 1 <= n_out <= 4096 and n_in / 2 <= n_out <= 8 n_in (13 taps at
    the most), and B Ho Wo 3 < 2^31"""
    for name, n_in, n_out in (("height", height, out_height), ("width", width, out_width)):
        if isinstance(n_out, bool) or not isinstance(n_out, (int, np.integer)):
            raise ValueError(f"output size: {name}={n_out!r}: use an integer")
        if not 1 <= int(n_out) <= MAX_SIZE:
            raise ValueError(f"output size: {name}={n_out} is outside 1..{MAX_SIZE}")
        if 2 * int(n_out) < int(n_in) or int(n_out) > 8 * int(n_in):
            raise ValueError(f"output size: {name}={n_out} is outside {n_in} / 2 .. 8 * {n_in} (a ratio from 1/2 to 8 is served)")
    if int(batch) * int(out_height) * int(out_width) * 3 >= 1 << 31:
        raise ValueError(f"output size: {batch} x {out_height} x {out_width} x 3 bytes must stay below 2^31")
    return int(out_height), int(out_width)


def camera_box(Hs: int, Ws: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(y0, x0, bh, bw): the integer window of an Hs x Ws camera frame that the ingest's resize + centre crop to H x W looks at.
    From `frame_io.geometry`'s (nh, nw, top, left), per axis in Python floats: b = clamp(floor(size n_src / n_res + 0.5), 1, n_src),
    o = clamp(floor(first n_src / n_res + 0.5), 0, n_src - b).  The window is rounded to whole source pixels, so it can sit up to
    half a source pixel off the frame the stream stylises."""
    nh, nw, top, left = geometry(Hs, Ws, H, W)

    def axis(size, first, n_src, n_res):
        b = min(max(int(math.floor(size * n_src / n_res + 0.5)), 1), n_src)
        o = min(max(int(math.floor(first * n_src / n_res + 0.5)), 0), n_src - b)
        return o, b

    (y0, bh), (x0, bw) = axis(H, top, Hs, nh), axis(W, left, Ws, nw)
    return y0, x0, bh, bw


def check_jpeg_size(out_height: int, out_width: int) -> None:
    """the JPEG encoder's own rules on an output size: multiples of 16, no wider than `ops.JPEG_MAX_W`"""
    if out_height % 16 or out_width % 16:
        raise ValueError(f"output size: {out_height} x {out_width} is not a multiple of 16 (whole MCUs) in both sizes: "
                         "output_type='jpeg' needs that")
    if out_width > ops.JPEG_MAX_W:
        raise ValueError(f"output size: width={out_width} is above {ops.JPEG_MAX_W}, the widest frame output_type='jpeg' encodes")


# ----------------------------------------------------------------------------- the device side
def axis_table(n_in: int, n_out: int, resample: str) -> np.ndarray:
    """the table of one axis as the kernel reads it: int32 xmin [n_out], count [n_out], k [n_out][KS] behind one another.  An
    axis that does not change gets the identity table (one tap of 2^22: (2^21 + 2^22 b) >> 22 == b)."""
    if n_in == n_out:
        xmin, count = np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32)
        k = np.full((n_out, 1), 1 << PRECISION_BITS, np.int32)
    else:
        xmin, count, k = coefficients(n_in, n_out, resample)
    return np.concatenate([xmin, count, k.reshape(-1)]).astype(np.int32)


class HipResize:
    """Device tables, static output buffers and the launch of one `(H, W) -> (Ho, Wo)` geometry: `resize` is
    `HipFrameIO.egress` with an output size.  The source is the stream's fp16 frame or the matte's uint8 frame; both live in
    static buffers, so the one-op plan of every source pointer is kept.  Everything runs on `torch.cuda.current_stream()`."""

    MAX_PLANS = 4                        # (the stream's outputs, the matte's buffer, the colour lock's frame: a handful)

    def __init__(self, height: int, width: int, out_height: int, out_width: int, resample: str = "lanczos", device="cuda:0"):
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.out_height, self.out_width = check_size(height, width, out_height, out_width)
        self.resample = check_filter(resample)
        tx, ty = axis_table(self.width, self.out_width, resample), axis_table(self.height, self.out_height, resample)
        self.ks_x, self.ks_y = (len(t) // n - 2 for t, n in ((tx, self.out_width), (ty, self.out_height)))
        self.tx, self.ty = torch.from_numpy(tx).to(self.device), torch.from_numpy(ty).to(self.device)
        self.dev = torch.empty(1, self.out_height, self.out_width, 3, dtype=torch.uint8, device=self.device)
        self.host = None if ops.DRY_RUN else torch.empty(1, self.out_height, self.out_width, 3, dtype=torch.uint8).pin_memory()
        self._plans = {}                 # (source pointer, dtype) -> plan, of sources met more than once
        self._seen = ()                  # the last MAX_PLANS source pointers (integers: nothing is kept alive)

    def _plan(self, image: torch.Tensor):
        """A producer with static outputs meets its plan again: a source pointer seen before gets its plan kept (a kept plan
        keeps its source alive, so its pointer cannot become another tensor's).  A pointer seen for the first time fills one
        record and keeps nothing, as `HipFrameIO.ingest` does for a caller's device frames."""
        key = (image.data_ptr(), image.dtype)
        pl = self._plans.get(key)
        if pl is None:
            op, keep = ops.frame_resize(image, self.dev, self.tx, self.ty, B=1, H=self.height, W=self.width, Ho=self.out_height,
                                        Wo=self.out_width)
            pl = _lib.OpList()
            pl.append(op, *keep)
            if key in self._seen:
                if len(self._plans) >= self.MAX_PLANS:
                    self._plans.clear()
                self._plans[key] = pl
            self._seen = (self._seen + (key,))[-self.MAX_PLANS:]
        return pl

    def resize(self, image: torch.Tensor, to_host: bool = True):
        """fp16 [3,H,W] in [-1, 1] (the egress op's bytes first) or uint8 [H,W,3] on the device -> uint8 [Ho,Wo,3]: a numpy view of
        the pinned buffer (valid until the next call), or with `to_host=False` the static device tensor"""
        H, W = self.height, self.width
        ok = (image.dtype == torch.float16 and tuple(image.shape) == (3, H, W)) or \
             (image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3))
        if not ok:
            raise ValueError(f"resize: expected fp16 [3,{H},{W}] or uint8 [{H},{W},3], got {image.dtype} {tuple(image.shape)}")
        if not image.is_contiguous():
            image = image.contiguous()
        self._plan(image).run()
        if not to_host:
            return self.dev[0]
        return to_pinned(self.dev, self.host)[0]


class CameraBuffer:
    """one camera frame at an output size: uint8 [Ho,Wo,3] on the device, and the (Ho, Wo, resample) it was resampled for"""

    def __init__(self, data: torch.Tensor, key):
        self.data, self.key = data, key


class CameraTap:
    """The hook of `HipFrameIO.ingest` (`camera_tap`) while the matte is composited at the output size: every single frame that
    is ingested also leaves its own pixels -- `camera_box` of the uint8 frame on the device -- resampled to the output size
    (`resize_ref` of the window, one launch of L2D_OP_FRAME_RESIZE with the frame's row pitch) in a buffer out of a pool, as
    `pending`.  `MatteLine._store` moves `pending` into the frame's slot and gives the slot's previous buffer back
    (`give_back`); `begin` (the wrapper, in front of every frame) takes back a `pending` nobody claimed, e.g. that of a frame
    the near-duplicate filter dropped.

    For one `(Hs, Ws)` it holds the box, the two `axis_table`s and one kept plan per (source, buffer) pair, by the rule of
    `HipResize._plan`; a frame of another size rebuilds them (the pool's buffers are at the output size and stay).  `prepare(Hs, Ws)` runs in front of the ingest
    launch and raises `check_size`'s ValueError for a window the resize does not serve.  The pool grows with the delay line's
    ring and allocates nothing in steady state.  Launches on `torch.cuda.current_stream()` only, from inside `ingest`."""

    MAX_PLANS = 16

    def __init__(self, height: int, width: int, out_height: int, out_width: int, resample: str = "lanczos", device="cuda:0"):
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.out_height, self.out_width, self.resample = int(out_height), int(out_width), check_filter(resample)
        self.key = (self.out_height, self.out_width, self.resample)
        self.pending = None
        self.free = []
        self.allocated = 0
        self._src = self.box = None

    def prepare(self, Hs: int, Ws: int) -> None:
        if self._src == (Hs, Ws):
            return
        y0, x0, bh, bw = box = camera_box(Hs, Ws, self.height, self.width)
        check_size(bh, bw, self.out_height, self.out_width)
        tx, ty = axis_table(bw, self.out_width, self.resample), axis_table(bh, self.out_height, self.resample)
        self.tx, self.ty = torch.from_numpy(tx).to(self.device), torch.from_numpy(ty).to(self.device)
        self._src, self.box = (Hs, Ws), box
        self._plans, self._seen = {}, ()

    def begin(self) -> None:
        """in front of a frame: a `pending` buffer nobody claimed goes back to the pool"""
        if self.pending is not None:
            self.free.append(self.pending)
            self.pending = None

    def give_back(self, buf) -> None:
        if buf is not None and buf.key == self.key:
            self.free.append(buf)

    def _buffer(self) -> CameraBuffer:
        if self.free:
            return self.free.pop()
        self.allocated += 1
        return CameraBuffer(torch.empty(self.out_height, self.out_width, 3, dtype=torch.uint8, device=self.device), self.key)

    def __call__(self, src: torch.Tensor) -> None:
        """`src`: the device uint8 [1,Hs,Ws,3] frame the ingest launch just read, on the stream it ran on"""
        Hs, Ws = src.shape[-3], src.shape[-2]
        self.prepare(Hs, Ws)
        self.begin()
        buf = self._buffer()
        y0, x0, bh, bw = self.box
        key = (src.data_ptr(), buf.data.data_ptr())
        pl = self._plans.get(key)
        if pl is None:
            window = src.reshape(-1)[(y0 * Ws + x0) * 3:]
            op, keep = ops.frame_resize(window, buf.data, self.tx, self.ty, B=1, H=bh, W=bw, Ho=self.out_height, Wo=self.out_width,
                                        src_pitch=Ws)
            pl = _lib.OpList()
            pl.append(op, *keep)
            if key in self._seen:
                if len(self._plans) >= self.MAX_PLANS:
                    self._plans.clear()
                self._plans[key] = pl
            self._seen = (self._seen + (key,))[-self.MAX_PLANS:]
        pl.run()
        self.pending = buf
