"""Colour lock (csrc/colorlock.hip): hold the output's colour statistics on the device.  The temporal
attention keeps the stream's structure stable; nothing constrains the global brightness and colour cast of the decoded frame,
which wander from frame to frame and away from the room's lighting.  The lock measures the per-channel mean and variance of the
BYTES a frame leaves as, and moves them to a target -- the frame's own source, a running average, or a reference image -- with
one gain and one offset per channel, in two small launches in front of the outlets (egress, matte, JPEG encoder).

  * `sums_ref`, `moments_ref`, `coefficients_ref`, `lock_ref`   the arithmetic of L2D_OP_FRAME_MOMENTS and L2D_OP_COLOR_LOCK in
                      numpy -- the kernels' oracle, as `matte.composite_ref` and `frame_io.egress_ref` are.  The statistics are
                      exact integers; every floating-point step is one fp64 or fp32 operation with one rounding and no fused
                      multiply-add, so the kernels are held to equality;
  * `check_settings`  the argument checks of `StreamAnimateDiffusionDepthWrapper.set_color_lock`;
  * `HipColorLock`    the static buffers and the two-op launch of one stream.

A state is a float64 [3,2] array: (mean, variance) of the bytes of channel 0, 1, 2.  Modes: "source" (the target is the frame's
own source frame), "ema" (the target follows the unlocked styled frame: t <- t + rate (c - t)), "image" (a frozen reference)."""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .frame_io import egress_ref, frame16

MODES = ("source", "ema", "image")
SERVED_OUTPUT_TYPES = ("pil", "pt", "np", "u8", "jpeg")
MAX_PIXELS = ops.COLOR_LOCK_MAX_PIXELS
GAIN_MIN, GAIN_MAX = 0.25, 4.0


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy)
def _frame16(x) -> np.ndarray:
    """fp16 [3,H,W] of a [3,H,W] or [1,3,H,W] array / tensor of at most MAX_PIXELS pixels"""
    x = frame16(x, "colour lock")
    if x.shape[1] * x.shape[2] > MAX_PIXELS:
        raise ValueError(f"colour lock: {x.shape[1]} x {x.shape[2]} is more than {MAX_PIXELS} pixels (n S2 - S1^2 must stay inside int64)")
    return x


def sums_ref(x) -> Tuple[np.ndarray, np.ndarray, int]:
    """(S1, S2, n): per channel the sum and the sum of squares (int64 [3]) of the bytes `egress_ref` makes of the finite fp16 frame
    `x` -- the fp16 chain clamp(fp16(fp16(x / 2) + 0.5), 0, 1), then rint(255 v), half to even: what the viewer sees -- and
    n = H W.  Refuses more than 2^22 pixels with ValueError."""
    x = _frame16(x)
    b = egress_ref(torch.from_numpy(x))[0].numpy().astype(np.int64).reshape(-1, 3)
    return b.sum(0), (b * b).sum(0), x.shape[1] * x.shape[2]


def moments_from_sums(S1, S2, n: int) -> np.ndarray:
    """float64 [3,2]: mean = double(S1) / double(n), var = double(n S2 - S1^2) / double(n n); the integers are exact in int64 for
    n <= 2^22, the conversions round to nearest even (exact below 2^53) and each division is one correctly rounded fp64 division"""
    S1, S2, n = np.asarray(S1, dtype=np.int64), np.asarray(S2, dtype=np.int64), int(n)
    D = n * S2 - S1 * S1
    return np.stack([S1.astype(np.float64) / np.float64(n), D.astype(np.float64) / np.float64(n * n)], axis=1)


def moments_ref(x) -> np.ndarray:
    """float64 [3,2], (mean, variance) per channel of the bytes a finite fp16 [3,H,W] frame leaves as (`sums_ref`)"""
    return moments_from_sums(*sums_ref(x))


def coefficients_ref(own, target, strength: float = 1.0) -> np.ndarray:
    """float32 [3,3], (g32, s32, t32) per channel, from the frame's own moments and the target's (float64 [3,2] each), in fp64 with
    one rounding per step: g = sqrt(var_t / var_s), 1 where either variance is 0; g = min(max(g, 1/4), 4); g = 1 + a (g - 1);
    m = mean_s + a (mean_t - mean_s); s32 = float32(2 mean_s / 255 - 1), t32 = float32(2 m / 255 - 1), g32 = float32(g)"""
    own, target = np.asarray(own, dtype=np.float64), np.asarray(target, dtype=np.float64)
    a, one = np.float64(strength), np.float64(1.0)
    out = np.empty((3, 3), dtype=np.float32)
    for c in range(3):
        (mean_s, var_s), (mean_t, var_t) = own[c], target[c]
        g = one if var_s == 0.0 or var_t == 0.0 else np.sqrt(var_t / var_s)
        g = min(max(g, np.float64(GAIN_MIN)), np.float64(GAIN_MAX))
        g = one + a * (g - one)
        m = mean_s + a * (mean_t - mean_s)
        s = np.float64(2.0) * mean_s / np.float64(255.0) - one
        t = np.float64(2.0) * m / np.float64(255.0) - one
        out[c] = np.float32(g), np.float32(s), np.float32(t)
    return out


def state_ref(own, state, *, mode: str, rate: float = 0.1, init: bool = False, source=None) -> np.ndarray:
    """the target state of this output frame: "source" the moments of `source`; "image" `state` as it is; "ema" the frame's own
    moments `own` when `init`, else t + rate (c - t) in three fp64 operations per value"""
    if mode == "source":
        return moments_ref(source)
    if mode == "image":
        return np.array(state, dtype=np.float64).reshape(3, 2)
    if mode != "ema":
        raise ValueError(f"colour lock: mode={mode!r}: use one of {MODES}")
    own = np.asarray(own, dtype=np.float64)
    if init:
        return own.copy()
    t = np.asarray(state, dtype=np.float64).reshape(3, 2)
    return t + np.float64(rate) * (own - t)


def apply_ref(x, coef) -> np.ndarray:
    """fp16 [3,H,W]: per pixel d = float32(x) - s32, p = d g32, o = p + t32, fp16(clamp(o, -1, 1)) rounded to nearest even"""
    x = _frame16(x).astype(np.float32)
    coef = np.asarray(coef, dtype=np.float32)
    g, s, t = (coef[:, k].reshape(3, 1, 1) for k in range(3))
    o = (x - s) * g + t                                  # numpy: three separate fp32 operations
    assert o.dtype == np.float32
    return np.clip(o, np.float32(-1.0), np.float32(1.0)).astype(np.float16)


def lock_ref(styled, state=None, *, mode: str = "ema", strength: float = 1.0, rate: float = 0.1, init: bool = False, source=None,
             with_coefficients: bool = False):
    """L2D_OP_FRAME_MOMENTS + L2D_OP_COLOR_LOCK on the host: the finite fp16 [3,H,W] (or [1,3,H,W]) frame `styled` in the decoder's
    [-1, 1] convention and the float64 [3,2] `state` (ignored by "source", and by "ema" with `init`) -> (locked fp16 [1,3,H,W],
    new state) -- and the float32 [3,3] coefficient record with `with_coefficients`.  `source`: the fp16 frame "source" takes its
    target from.  Inputs are finite: NaN or infinity in a frame has no defined result."""
    own = moments_ref(styled)
    new = state_ref(own, state, mode=mode, rate=rate, init=init, source=source)
    coef = coefficients_ref(own, new, strength)
    locked = apply_ref(styled, coef)[None]
    return (locked, new, coef) if with_coefficients else (locked, new)


def check_settings(to="source", strength=1.0, rate=0.1) -> dict:
    """{mode, strength, rate}, or ValueError: `to` is "source", "ema" or a reference image (anything that is no string: mode
    "image"), `strength` a number in [0, 1], `rate` a number in (0, 1]"""
    if isinstance(to, str):
        if to not in ("source", "ema"):
            raise ValueError(f"color lock: to={to!r}: use 'source', 'ema' or a reference image")
        mode = to
    elif to is None or isinstance(to, (bool, int, float)):
        raise ValueError(f"color lock: to={to!r}: use 'source', 'ema' or a reference image")
    else:
        mode = "image"
    for name, v, lo_open in (("strength", strength, False), ("rate", rate, True)):
        ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and 0.0 <= float(v) <= 1.0
        if not ok or (lo_open and float(v) == 0.0):
            raise ValueError(f"color lock: {name}={v!r}: use a number in {'(0, 1]' if lo_open else '[0, 1]'}")
    return dict(mode=mode, strength=float(strength), rate=float(rate))


# ----------------------------------------------------------------------------- the device side
class HipColorLock:
    """Static buffers and the two launches of one `(H, W)` stream: the partial sums, two state records the launches ping-pong
    between (no block reads what block 0 writes), the coefficient record and the fp16 output frame.  Everything runs on
    `torch.cuda.current_stream()`; nothing is read back."""

    def __init__(self, height: int, width: int, device="cuda:0"):
        if width % 8 or (height * width) % 16:
            raise ValueError(f"HipColorLock: width {width} must be a multiple of 8 and height * width a multiple of 16")
        if height * width > MAX_PIXELS:
            raise ValueError(f"HipColorLock: {height} x {width} is more than {MAX_PIXELS} pixels")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.nblk = ops.color_lock_blocks(height, width)
        self.partials = torch.zeros(2, self.nblk, 6, dtype=torch.int32, device=self.device)
        self.states = [torch.zeros(3, 2, dtype=torch.float64, device=self.device) for _ in range(2)]
        self.coef = torch.zeros(3, 3, dtype=torch.float32, device=self.device)
        self.out = torch.empty(1, 3, self.height, self.width, dtype=torch.float16, device=self.device)
        self._cur = 0                       # the record that holds the current state

    @property
    def state(self) -> torch.Tensor:
        """the current state record (a device tensor; reading it synchronises)"""
        return self.states[self._cur]

    def load_state(self, state) -> None:
        """set the state from the host (a reference image's moments, computed once)"""
        self.states[self._cur].copy_(torch.as_tensor(np.asarray(state, dtype=np.float64).reshape(3, 2)), non_blocking=False)

    def lock(self, image: torch.Tensor, source: Optional[torch.Tensor], settings: dict, init: bool = False) -> torch.Tensor:
        """fp16 [3,H,W] (or [1,3,H,W]) on the device (+ the fp16 [3,H,W] source frame in "source" mode) -> the static fp16
        [1,3,H,W] output frame, valid until the next call.  No synchronisation, no read-back."""
        H, W = self.height, self.width
        if image.dtype != torch.float16 or tuple(image.shape[-3:]) != (3, H, W) or image.numel() != 3 * H * W:
            raise ValueError(f"lock: expected fp16 [3,{H},{W}], got {image.dtype} {tuple(image.shape)}")
        if not image.is_contiguous():
            image = image.contiguous()
        mode = settings["mode"]
        if (mode == "source") != (source is not None):
            raise ValueError("lock: a source frame goes with mode 'source', and with no other")
        if source is not None and not source.is_contiguous():
            source = source.contiguous()
        nxt = 1 - self._cur
        pl = _lib.OpList()
        op, keep = ops.frame_moments(image, source, self.partials, H=H, W=W)
        pl.append(op, *keep)
        op, keep = ops.color_lock(image, self.out, self.partials, self.states[self._cur], self.states[nxt], self.coef, H=H, W=W,
                                  strength=settings["strength"], rate=settings["rate"], init=init and mode == "ema",
                                  source=mode == "source", freeze=mode == "image")
        pl.append(op, *keep)
        pl.run()
        self._cur = nxt
        return self.out
