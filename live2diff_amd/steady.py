"""Steady (csrc/steady.hip): hold still what the camera holds still.  The temporal attention keeps the
stream's structure coherent and the colour lock holds its global colour statistics; nothing holds a pixel, so a wall that does
not move in the camera still shimmers in the styled output.  Steady measures, in exact integers on the BYTES a viewer would
see, where the frame's source moved since the source of the output before; where it did not, the previous output pixel is held
(a per-pixel EMA), where it did, the new styled pixel passes untouched -- a hard cut moves everything and passes by itself.
One small launch in front of the outlets (egress, matte, resize, JPEG encoder), behind the colour lock.

  * `steady_params`, `source_bytes`, `weight_ref`, `steady_ref`   the arithmetic of L2D_OP_FRAME_STEADY in numpy -- the kernel's
                      oracle, as `matte.composite_ref` and `color_lock.lock_ref` are.  The motion is exact integers; every
                      floating-point step is one fp32 operation with one rounding and no fused multiply-add, so the kernel is
                      held to equality;
  * `check_settings`  the argument checks of `StreamAnimateDiffusionDepthWrapper.set_steady`;
  * `follow_candidates`, `motion_ref`, `warp_ref`, `follow_ref`, `check_follow`   follow (csrc/steady_follow.hip, DESIGN.md section
                      8.z14): steady along the source's motion.  One vector per 8 x 8 block, found by exhaustive matching of the
                      bytes in exact integers (L2D_OP_FRAME_MOTION), then `steady_ref` on the previous record fetched along the
                      vectors (L2D_OP_FRAME_STEADY_FOLLOW) -- under a pan or a hand-held camera, where plain steady holds nothing;
  * `HipSteady`       the static buffers and the launches of one stream: op 48, or with `follow=` ops 55 and 56.

A state is `(prev_out, prev_bytes)`: the previous steady output, fp16 [3,H,W], and the bytes of ITS source frame, planar uint8
[3,H,W].  `lo` and `hi` are in byte levels (0..255) of the locally averaged motion: at or below `lo` a pixel counts as still, at
or above `hi` as moving, a smoothstep in between."""
from typing import Tuple

import numpy as np
import torch

from . import _lib, ops
from .frame_io import egress_ref, frame16

MAX_RADIUS = ops.STEADY_MAX_R
FOLLOW_BLOCK, FOLLOW_APRON = ops.FOLLOW_BLOCK, ops.FOLLOW_APRON       # one vector per 8 x 8 block; the matching window is 16 x 16
FOLLOW_MAX_SEARCH, FOLLOW_MAX_BIAS = ops.FOLLOW_MAX_SEARCH, ops.FOLLOW_MAX_BIAS
SERVED_OUTPUT_TYPES = ("pil", "pt", "np", "u8", "jpeg")


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy)
def steady_params(lo: float, hi: float) -> Tuple[np.float32, np.float32, bool]:
    """(lo32, inv32, hard) of a ramp from `lo` to `hi`, both byte levels in [0, 255]: lo32 = float32(lo), inv32 =
    float32(1 / (hi - lo)) computed in Python doubles; hi <= lo, or an inverse that is not finite, is a step (`hard`, inv32 = 0)"""
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= 255.0 and 0.0 <= hi <= 255.0):
        raise ValueError(f"steady: lo={lo!r}, hi={hi!r} must lie in [0, 255]")
    if lo > hi:
        raise ValueError(f"steady: lo={lo!r} is above hi={hi!r}")
    hard = hi <= lo
    with np.errstate(over="ignore"):
        inv = np.float32(0.0) if hard else np.float32(1.0 / (hi - lo))
    if not np.isfinite(inv):
        hard, inv = True, np.float32(0.0)
    return np.float32(lo), inv, bool(hard)


def source_bytes(source) -> np.ndarray:
    """planar uint8 [3,H,W]: the bytes `egress_ref` makes of the finite fp16 frame `source` -- the fp16 chain
    clamp(fp16(fp16(x / 2) + 0.5), 0, 1), then rint(255 v), half to even: what a viewer would see of it"""
    x = np.ascontiguousarray(frame16(source, "steady", "source frame"))
    return np.ascontiguousarray(egress_ref(torch.from_numpy(x))[0].numpy().transpose(2, 0, 1))


def window_sum(d: np.ndarray, radius: int) -> np.ndarray:
    """int64 [H,W]: the sum of the integers `d` over the (2 radius + 1)^2 window, coordinates clamped to the image"""
    d = np.asarray(d).astype(np.int64)
    r = int(radius)
    if r == 0:
        return d
    H, W = d.shape
    p = np.pad(d, r, mode="edge")
    rows = sum(p[:, k:k + W] for k in range(2 * r + 1))
    return sum(rows[k:k + H] for k in range(2 * r + 1))


def weight_ref(now_bytes, prev_bytes, *, lo: float, hi: float, radius: int = 0) -> np.ndarray:
    """float32 [H,W], 1 = moving, 0 = still, from two planar uint8 [3,H,W] byte frames: d = max_c |b_c - bp_c|, D = its window
    sum, dbar = float32(D) / float32((2r+1)^2) (one correctly rounded division; D <= 255 * 289 converts exactly),
    t = clamp((dbar - lo32) inv32, 0, 1) (hard: dbar >= lo32), w = (t t) (3 - 2 t)"""
    lo32, inv32, hard = steady_params(lo, hi)
    r = int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"steady: radius={radius!r}: use an integer from 0 to {MAX_RADIUS}")
    b, bp = np.asarray(now_bytes), np.asarray(prev_bytes)
    if b.dtype != np.uint8 or bp.dtype != np.uint8 or b.ndim != 3 or b.shape[0] != 3 or b.shape != bp.shape:
        raise ValueError(f"steady: expected two planar uint8 [3,H,W] byte frames, got {b.dtype} {b.shape} and {bp.dtype} {bp.shape}")
    d = np.abs(b.astype(np.int64) - bp.astype(np.int64)).max(axis=0)
    D = window_sum(d, r)
    dbar = D.astype(np.float32) / np.float32((2 * r + 1) ** 2)
    one, zero = np.float32(1.0), np.float32(0.0)
    if hard:
        t = np.where(dbar >= lo32, one, zero).astype(np.float32)
    else:
        t = np.minimum(np.maximum((dbar - lo32) * inv32, zero), one)
    w = (t * t) * (np.float32(3.0) - np.float32(2.0) * t)
    assert w.dtype == np.float32
    return w


def steady_ref(styled, source, state, *, lo: float, hi: float, strength: float, radius: int, show: bool = False, init: bool = False):
    """L2D_OP_FRAME_STEADY on the host: the finite fp16 [3,H,W] (or [1,3,H,W]) frames `styled` and `source` in the decoder's
    [-1, 1] convention and the state `(prev_out fp16 [3,H,W], prev_bytes uint8 [3,H,W])` (ignored with `init`, where it may be
    None) -> (fp16 [1,3,H,W], new state).  a = 1 - s32 (1 - w) and o = fp16(P + a (S - P)) in three fp32 operations each, one
    rounding per operation; where a == 1 the output is S's own bits.  o lies between S and P (rounding is monotone; asserted),
    nothing is clamped.  `show` returns fp16(2 w - 1) in all three channels instead; the new state is (o, b) either way.  With
    `init` the output and the state's frame are `styled` itself."""
    S16 = np.ascontiguousarray(frame16(styled, "steady", "styled frame"))
    b = source_bytes(source)
    if b.shape != S16.shape:
        raise ValueError(f"steady: the styled frame is {S16.shape}, its source {b.shape}")
    s = float(strength)
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"steady: strength={strength!r}: use a number in [0, 1]")
    if init:
        steady_params(lo, hi)
        return S16[None].copy(), (S16.copy(), b)
    P16, bp = state
    P16 = frame16(P16, "steady", "previous frame")
    if P16.shape != S16.shape:
        raise ValueError(f"steady: the styled frame is {S16.shape}, the previous output {P16.shape}")
    w = weight_ref(b, bp, lo=lo, hi=hi, radius=radius)
    one = np.float32(1.0)
    a = (one - np.float32(s) * (one - w))[None]
    S, P = S16.astype(np.float32), P16.astype(np.float32)
    o32 = P + a * (S - P)                                  # numpy: three separate fp32 operations
    assert o32.dtype == np.float32 and a.dtype == np.float32
    o = np.where(a == one, S16, o32.astype(np.float16))
    assert o.dtype == np.float16 and np.all(o >= np.minimum(S16, P16)) and np.all(o <= np.maximum(S16, P16))
    new = (np.ascontiguousarray(o), b)
    if show:
        pic = (np.float32(2.0) * w - one).astype(np.float16)
        return np.ascontiguousarray(np.broadcast_to(pic, S16.shape))[None], new
    return o[None].copy(), new


def check_settings(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False) -> dict:
    """the settings as a dict, or ValueError: lo > hi, values outside [0, 255], `strength` outside [0, 1], `radius` no integer
    in 0..8"""
    for name, v in (("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 255.0:
            raise ValueError(f"steady: {name}={v!r}: use a number in [0, 255]")
    if float(lo) > float(hi):
        raise ValueError(f"steady: lo={lo!r} is above hi={hi!r}")
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"steady: strength={strength!r}: use a number in [0, 1]")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"steady: radius={radius!r}: use an integer from 0 to {MAX_RADIUS}")
    return dict(lo=float(lo), hi=float(hi), strength=float(strength), radius=int(radius), show=bool(show))


# ----------------------------------------------------------------------------- follow: reference arithmetic (CPU, numpy)
def follow_candidates(search: int):
    """the vectors (dy, dx) of [-search, search]^2 sorted by (|dy| + |dx|, dy, dx): the position in the list is the `rank`"""
    R = int(search)
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))


def _check_search(search, bias):
    if isinstance(search, bool) or not isinstance(search, (int, np.integer)) or not 1 <= int(search) <= FOLLOW_MAX_SEARCH:
        raise ValueError(f"steady follow: search={search!r}: use an integer from 1 to {FOLLOW_MAX_SEARCH}")
    if isinstance(bias, bool) or not isinstance(bias, (int, np.integer)) or not 0 <= int(bias) <= FOLLOW_MAX_BIAS:
        raise ValueError(f"steady follow: bias={bias!r}: use an integer from 0 to {FOLLOW_MAX_BIAS}")
    return int(search), int(bias)


def motion_ref(now_bytes, prev_bytes, search: int, bias: int) -> np.ndarray:
    """L2D_OP_FRAME_MOTION on the host: two planar uint8 [3,H,W] byte frames -> int8 [ceil(H/8), ceil(W/8), 2], per 8 x 8 block the
    vector (dy, dx) of the smallest key = (cost + bias (|dy| + |dx|)) 512 + rank, cost the sum over the block's 16 x 16 window
    (rows 8i-4 .. 8i+11, columns 8j-4 .. 8j+11) and the channels of |now[c, cl(y), cl(x)] - prev[c, cl(y+dy), cl(x+dx)]|, every
    coordinate clamped to the image on its own.  Exact integers: ties go to the shortest vector, then the smaller dy, then the
    smaller dx; the zero vector wins any tie."""
    R, bias = _check_search(search, bias)
    b, bp = np.asarray(now_bytes), np.asarray(prev_bytes)
    if b.dtype != np.uint8 or bp.dtype != np.uint8 or b.ndim != 3 or b.shape[0] != 3 or b.shape != bp.shape:
        raise ValueError(f"steady follow: expected two planar uint8 [3,H,W] byte frames, got {b.dtype} {b.shape} and {bp.dtype} {bp.shape}")
    _, H, W = b.shape
    B, A = FOLLOW_BLOCK, FOLLOW_APRON
    Hb, Wb = -(-H // B), -(-W // B)
    ys, xs = np.arange(-A, B * Hb + A), np.arange(-A, B * Wb + A)      # the rows and columns the windows cover, unclamped
    now = b.astype(np.int64)[:, np.clip(ys, 0, H - 1)][:, :, np.clip(xs, 0, W - 1)]
    prev = bp.astype(np.int64)
    best = np.full((Hb, Wb), np.iinfo(np.int64).max, dtype=np.int64)
    cands = follow_candidates(R)
    assert len(cands) <= 512
    for rank, (dy, dx) in enumerate(cands):
        moved = prev[:, np.clip(ys + dy, 0, H - 1)][:, :, np.clip(xs + dx, 0, W - 1)]
        # cells of 4 x 4 pixels (the apron's size); the window of block (i, j) is the 4 x 4 cells from cell (2i, 2j) on
        c4 = np.abs(now - moved).sum(axis=0).reshape(2 * Hb + 2, A, 2 * Wb + 2, A).sum(axis=(1, 3))
        rows = c4[0:-3] + c4[1:-2] + c4[2:-1] + c4[3:]
        win = rows[:, 0:-3] + rows[:, 1:-2] + rows[:, 2:-1] + rows[:, 3:]
        cost = win[0::2, 0::2]
        assert cost.shape == (Hb, Wb) and int(cost.max()) <= 768 * 255
        best = np.minimum(best, (cost + bias * (abs(dy) + abs(dx))) * 512 + rank)
    assert int(best.max()) < 1 << 27
    field = np.array(cands, dtype=np.int8)[best % 512]
    return np.ascontiguousarray(field)


def warp_ref(planes, field) -> np.ndarray:
    """out[c, y, x] = planes[c, cl(y + dy), cl(x + dx)], (dy, dx) the vector of block (y // 8, x // 8) of the int8 `field`"""
    p, f = np.asarray(planes), np.asarray(field)
    _, H, W = p.shape
    if f.dtype != np.int8 or f.shape != (-(-H // FOLLOW_BLOCK), -(-W // FOLLOW_BLOCK), 2):
        raise ValueError(f"steady follow: a [{H},{W}] frame takes an int8 field of {(-(-H // FOLLOW_BLOCK), -(-W // FOLLOW_BLOCK), 2)}, got {f.dtype} {f.shape}")
    y, x = np.mgrid[0:H, 0:W]
    v = f[y // FOLLOW_BLOCK, x // FOLLOW_BLOCK].astype(np.int64)
    return np.ascontiguousarray(p[:, np.clip(y + v[..., 0], 0, H - 1), np.clip(x + v[..., 1], 0, W - 1)])


def follow_ref(styled, source, state, *, search: int, bias: int, lo: float, hi: float, strength: float, radius: int, show: bool = False,
               init: bool = False):
    """L2D_OP_FRAME_MOTION and L2D_OP_FRAME_STEADY_FOLLOW on the host -> (fp16 [1,3,H,W], new state, int8 field): the field of
    `motion_ref` between the source's bytes and the state's, then `steady_ref` on the state warped along it -- d, its window sum
    (each pixel with its own block's vector), w, a, the blend, "S's own bits where a == 1", `show` and the new state (o, b) are
    `steady_ref`'s.  With `init` there is no search: the field is zero and `steady_ref`'s init path applies."""
    R, bias = _check_search(search, bias)
    kw = dict(lo=lo, hi=hi, strength=strength, radius=radius, show=show)
    if init:
        frame, new = steady_ref(styled, source, None, init=True, **kw)
        _, H, W = new[1].shape
        return frame, new, np.zeros((-(-H // FOLLOW_BLOCK), -(-W // FOLLOW_BLOCK), 2), dtype=np.int8)
    P16, bp = state
    P16 = frame16(P16, "steady", "previous frame")
    field = motion_ref(source_bytes(source), bp, R, bias)
    frame, new = steady_ref(styled, source, (warp_ref(P16, field), warp_ref(bp, field)), **kw)
    return frame, new, field


def check_follow(search=4, bias=256) -> dict:
    """the follow settings as a dict, or ValueError: `search` no integer in 1..8, `bias` no integer in 0..4096"""
    search, bias = _check_search(search, bias)
    return dict(search=search, bias=bias)


# ----------------------------------------------------------------------------- the device side
class HipSteady:
    """Static buffers and the launch of one `(H, W)` stream: two `(out, bytes)` records the launches ping-pong between (a tile's
    halo reads its neighbours' previous bytes, so no block may read what another writes) and the picture `show` returns.
    Nothing is ever zeroed: the first launch carries `init` and reads neither record.  Everything runs on
    `torch.cuda.current_stream()`; nothing is read back."""

    def __init__(self, height: int, width: int, device="cuda:0", records=None, field=None):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipSteady: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        H, W = self.height, self.width
        # `records`: two (fp16 [1,3,H,W], uint8 [3,H,W]) pairs of the caller's (tests place them inside guarded buffers)
        self.records = records if records is not None else [
            (torch.empty(1, 3, H, W, dtype=torch.float16, device=self.device), torch.empty(3, H, W, dtype=torch.uint8, device=self.device))
            for _ in range(2)]
        # `field`: the int8 [ceil(H/8), W/8, 2] vectors of the last followed frame (made by the first one, or the caller's, as
        # `records`); every block of it is written by every followed frame, so tests and tools may read it behind one
        self.field = field
        self.picture = None                 # fp16 [1,3,H,W], made by the first `show` frame
        self._cur = 0                       # the record that holds the current state

    @property
    def state(self):
        """the current `(out, bytes)` record (device tensors; reading them synchronises)"""
        return self.records[self._cur]

    def steady(self, image: torch.Tensor, source: torch.Tensor, settings: dict, init: bool = False, follow=None) -> torch.Tensor:
        """fp16 [3,H,W] (or [1,3,H,W]) on the device + the fp16 [3,H,W] source frame -> the static fp16 [1,3,H,W] record (with
        `show` the picture buffer), valid until the next call.  One `OpList` run, no synchronisation, no read-back.  `follow`:
        `check_follow`'s dict, or None; with it, and not `init`, the frame runs ops 55 and 56 (the vectors, then steady along
        them) in place of op 48."""
        H, W = self.height, self.width
        for name, t in (("image", image), ("source", source)):
            if t.dtype != torch.float16 or tuple(t.shape[-3:]) != (3, H, W) or t.numel() != 3 * H * W:
                raise ValueError(f"steady: expected an fp16 [3,{H},{W}] {name}, got {t.dtype} {tuple(t.shape)}")
        image = image if image.is_contiguous() else image.contiguous()
        source = source if source.is_contiguous() else source.contiguous()
        lo32, inv32, hard = steady_params(settings["lo"], settings["hi"])
        show = bool(settings["show"])
        if show and self.picture is None:
            self.picture = torch.empty(1, 3, H, W, dtype=torch.float16, device=self.device)
        (prev_out, prev_bytes), (out, next_bytes) = self.records[self._cur], self.records[1 - self._cur]
        pl = _lib.OpList()
        common = dict(H=H, W=W, lo32=lo32, inv32=inv32, s32=np.float32(settings["strength"]), r=settings["radius"], hard=hard,
                      show=show, picture=self.picture if show else None)
        if follow is not None and not init:
            if self.field is None:
                self.field = torch.empty((H + FOLLOW_BLOCK - 1) // FOLLOW_BLOCK, W // FOLLOW_BLOCK, 2, dtype=torch.int8, device=self.device)
            op, keep = ops.frame_motion(source, prev_bytes, self.field, H=H, W=W, search=follow["search"], bias=follow["bias"])
            pl.append(op, *keep)
            op, keep = ops.frame_steady_follow(image, source, prev_out, prev_bytes, out, next_bytes, self.field, **common)
        else:
            op, keep = ops.frame_steady(image, source, prev_out, prev_bytes, out, next_bytes, init=init, **common)
        pl.append(op, *keep)
        pl.run()
        self._cur = 1 - self._cur
        return self.picture if show else out
