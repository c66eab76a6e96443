"""Detail mode (csrc/detail.hip): the camera's fine detail in the upscaled frame.  The output size
resamples 512 lines of styled frame to 1080 lines and sharpens nothing; the camera frame at the output size
(`resize.CameraTap`, carried by `matte.MatteLine`) holds what the stream-size bottleneck lost.  The regression-based detail
injection of pan-sharpening puts it back: the styled frame is the low-resolution colour image, the camera's luma at the output
size the high-resolution band, and the injection gain the local regression slope of each styled channel on the source frame's
luma -- stage 1 of the guided filter of `matte.edge_coefficients`.  Where the style follows the camera's structure the
camera's sub-pixel edges and texture come back in the style's own colours and polarity; where the style is flat the gain is 0
and nothing is added.

  * `gains_ref`, `inject_ref`, `detail_ref`   the arithmetic of L2D_OP_FRAME_DETAIL_GAIN and L2D_OP_FRAME_DETAIL in numpy -- the
                      kernels' oracle, as `matte.edge_ref` and `matte.composite_up_ref` are.  Exact integers and one correctly
                      rounded operation per step, no fused multiply-add, so the kernels are held to equality;
  * `check_settings`  the argument checks of `StreamAnimateDiffusionDepthWrapper.set_detail`;
  * `HipDetail`       the static buffers, the tables and the three-op plans of one `(H, W) -> (Ho, Wo)` geometry.

  P[c]  the bytes L2D_OP_FRAME_RESIZE is about to resample: the egress bytes of the fp16 frame, or the matte's uint8 frame
  Y     matte.guide_ref(source): the stream-sized source frame's luma
  A[c]  = matte.edge_coefficients(P[c], Y, r, eps)[0] = rint(4096 a), |A| <= 261120
  G[c]  = steady.window_sum(A[c], r): n 4096 times the mean gain, int32
  S, C, L   uint8 [Ho,Wo,3]: S = resize_ref(P), C the camera's pixels, L = resize_ref(egress bytes of the source), the same filter
  d     = luma(C) - luma(L) with luma(x) = (77 R + 150 G + 29 B + 128) >> 8: what the stream-size bottleneck lost
  g[c]  = matte.matte_up_ref(float32(G))[c];  k = float32(strength / (n 4096))
  t = g[c] float32(d);  u = t k;  u = min(max(u, -limit), limit);  o = min(max(float32(S[c]) + u, 0), 255);  byte = rint(o)
  show: byte = rint(min(max(128 + u, 0), 255)) per channel -- the injected term, for tuning eps

`L` goes through the output size's own filter, so luma(C) - luma(L) is exactly the high-pass that `S` lacks; a bilinear `L`
would sharpen twice.  C == L, strength == 0 and G == 0 each give S back byte for byte, and |byte - S| <= ceil(limit)."""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .frame_io import to_pinned
from .matte import EDGE_SHIFT, MAX_EDGE_RADIUS, edge_E, edge_coefficients, guide_ref, luma, matte_up_ref, table_words
from .resize import axis_table, check_filter, check_size, resize_ref
from .steady import source_bytes, window_sum

SERVED_OUTPUT_TYPES = ("u8", "pil", "jpeg")
MAX_RADIUS = MAX_EDGE_RADIUS
MAX_GAIN = ops.DETAIL_MAX_GAIN               # |A| <= 4096 * 127.5 / 2: the bound matte_edge.hip and detail.hip state
MAX_STRENGTH = 4.0


# ----------------------------------------------------------------------------- settings
def check_settings(radius=2, eps=2.0, strength=1.0, limit=64.0, show=False) -> dict:
    """the settings as {radius, eps, strength, limit, show}, or ValueError: `radius` no integer in 1..8, `eps` no finite number
    >= 1 (byte levels, as `matte.check_edge`), `strength` outside [0, 4], `limit` outside [0, 255]"""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(float(v))

    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"detail: radius={radius!r}: use an integer from 1 to {MAX_RADIUS}")
    if not number(eps) or not 1.0 <= float(eps) <= 1.0e100:
        raise ValueError(f"detail: eps={eps!r}: use a finite number of byte levels, at least 1")
    if not number(strength) or not 0.0 <= float(strength) <= MAX_STRENGTH:
        raise ValueError(f"detail: strength={strength!r}: use a number in [0, {MAX_STRENGTH:g}]")
    if not number(limit) or not 0.0 <= float(limit) <= 255.0:
        raise ValueError(f"detail: limit={limit!r}: use a number of byte levels in [0, 255]")
    return dict(radius=int(radius), eps=float(eps), strength=float(strength), limit=float(limit), show=bool(show))


def gain_scale(radius: int, strength: float) -> np.float32:
    """k = float32(strength / (n 4096)), formed in Python floats, then one cast: what turns g d into byte levels"""
    n = (2 * int(radius) + 1) ** 2
    return np.float32(float(strength) / (n * float(EDGE_SHIFT)))


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy)
def _u8_hwc(x, what: str) -> np.ndarray:
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if x.ndim == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[-1] != 3:
        raise ValueError(f"detail: expected one uint8 [H,W,3] {what}, got {x.dtype} {x.shape}")
    return x


def frame_bytes(frame_or_u8) -> np.ndarray:
    """uint8 [H,W,3]: the bytes the resize reads of a frame -- a uint8 [H,W,3] frame (the matte's) as it is, an fp16 [3,H,W]
    frame through the egress expression (`steady.source_bytes`)"""
    dt = getattr(frame_or_u8, "dtype", None)
    if dt == torch.uint8 or dt == np.uint8:
        return _u8_hwc(frame_or_u8, "frame")
    return np.ascontiguousarray(source_bytes(frame_or_u8).transpose(1, 2, 0))


def gains_ref(frame_or_u8, source, radius: int, eps: float) -> np.ndarray:
    """L2D_OP_FRAME_DETAIL_GAIN on the host: the frame the resize reads (fp16 [3,H,W], or uint8 [H,W,3]) and the fp16 [3,H,W]
    `source` frame -> int32 [3,H,W]: G[c] = window_sum(A[c]) with A[c] = rint(4096 a) the regression slope of the frame's bytes
    of channel c on the source frame's luma in every (2r+1)^2 window.  |G| <= 261120 n (asserted)."""
    s = check_settings(radius, eps)
    r = s["radius"]
    n = (2 * r + 1) ** 2
    P = frame_bytes(frame_or_u8).astype(np.int64)
    Y = guide_ref(source)
    if Y.shape != P.shape[:2]:
        raise ValueError(f"gains_ref: the frame is {P.shape[:2]}, the source frame {Y.shape}")
    G = np.stack([window_sum(edge_coefficients(P[..., c], Y, r, s["eps"])[0], r) for c in range(3)])
    assert int(np.abs(G).max()) <= MAX_GAIN * n < 1 << 31
    return G.astype(np.int32)


def inject_ref(S, C, L, G, H: int, W: int, radius: int, strength: float, limit: float, show: bool = False) -> np.ndarray:
    """L2D_OP_FRAME_DETAIL on the host: uint8 [Ho,Wo,3] `S`, `C`, `L` and the int32 [3,H,W] gains `G` -> uint8 [Ho,Wo,3].  Every
    floating-point step is one fp32 operation with one rounding."""
    S, C, L = _u8_hwc(S, "styled frame"), _u8_hwc(C, "camera frame"), _u8_hwc(L, "source frame at the output size")
    if not (S.shape == C.shape == L.shape):
        raise ValueError(f"inject_ref: the styled frame is {S.shape}, the camera frame {C.shape}, the source frame {L.shape}")
    G = np.asarray(G)
    if G.shape != (3, int(H), int(W)) or not np.issubdtype(G.dtype, np.integer):
        raise ValueError(f"inject_ref: expected integer gains [3,{H},{W}], got {G.dtype} {G.shape}")
    s = check_settings(radius, 1.0, strength, limit, show)
    Ho, Wo = S.shape[:2]
    d = (luma(C) - luma(L)).astype(np.float32)                              # |d| <= 255: exact
    g = matte_up_ref(G.astype(np.int32).astype(np.float32), Ho, Wo)         # [3,Ho,Wo]; the cast rounds to nearest even
    k, lim = gain_scale(s["radius"], s["strength"]), np.float32(s["limit"])
    t = g * d[None]
    u = t * k
    u = np.minimum(np.maximum(u, -lim), lim)
    base = np.float32(128.0) if s["show"] else S.astype(np.float32).transpose(2, 0, 1)
    o = base + u
    o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(255.0))
    assert t.dtype == u.dtype == o.dtype == np.float32
    return np.ascontiguousarray(np.rint(o).astype(np.uint8).transpose(1, 2, 0))


def detail_ref(frame_or_u8, source, camera, out_height: int, out_width: int, resample: str = "lanczos", *, radius=2, eps=2.0,
               strength=1.0, limit=64.0, show=False) -> np.ndarray:
    """the two joined from the frames: the frame the resize reads (fp16 [3,H,W] or uint8 [H,W,3]), its fp16 [3,H,W] `source`
    frame and the uint8 [Ho,Wo,3] `camera` frame -> the uint8 [Ho,Wo,3] frame the mode leaves"""
    s = check_settings(radius, eps, strength, limit, show)
    P = frame_bytes(frame_or_u8)
    H, W = P.shape[:2]
    S = resize_ref(P, out_height, out_width, resample)
    L = resize_ref(frame_bytes(source), out_height, out_width, resample)
    G = gains_ref(P, source, s["radius"], s["eps"])
    return inject_ref(S, camera, L, G, H, W, s["radius"], s["strength"], s["limit"], s["show"])


# ----------------------------------------------------------------------------- the device side
class HipDetail:
    """The static buffers, the tables and the launches of one `(H, W) -> (Ho, Wo)` geometry: the int32 gain planes, the source
    frame at the output size (`low`: one more launch of L2D_OP_FRAME_RESIZE on the slot's source frame with the `axis_table`s
    of the styled frame's resize, into a buffer of its own -- `HipResize.dev` holds S and is not touched), the output frame
    and its pinned twin, and the two `table_words` tables the gains are sampled with.  A frame is three launches in one plan;
    plans are kept by `HipResize._plan`'s rule.  Everything runs on `torch.cuda.current_stream()`: the plan reads a camera
    buffer (`MatteLine`'s rule)."""

    MAX_PLANS = 16                       # (ring slots x camera buffers x the stream's outputs: as CameraTap's)

    def __init__(self, height: int, width: int, out_height: int, out_width: int, resample: str = "lanczos", device="cuda:0"):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipDetail: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.out_height, self.out_width = check_size(height, width, out_height, out_width)
        self.resample = check_filter(resample)
        H, W, Ho, Wo = self.height, self.width, self.out_height, self.out_width
        self.tx, self.ty = (torch.from_numpy(table_words(n_in, n_out)).to(self.device) for n_in, n_out in ((W, Wo), (H, Ho)))
        self.rx, self.ry = (torch.from_numpy(axis_table(n_in, n_out, resample)).to(self.device) for n_in, n_out in ((W, Wo), (H, Ho)))
        self.gains = torch.empty(3, H, W, dtype=torch.int32, device=self.device)
        self.low = torch.empty(1, Ho, Wo, 3, dtype=torch.uint8, device=self.device)
        self.dev = torch.empty(1, Ho, Wo, 3, dtype=torch.uint8, device=self.device)
        self.host = None if ops.DRY_RUN else torch.empty(1, Ho, Wo, 3, dtype=torch.uint8).pin_memory()
        self._plans = {}                 # key -> plan, of operand sets met more than once
        self._seen = ()

    def plan(self, S_dev: torch.Tensor, frame: torch.Tensor, source: torch.Tensor, camera: torch.Tensor, settings: dict):
        """the three records -- gains, source resize, inject -- of one set of operands under `settings`"""
        H, W, Ho, Wo = self.height, self.width, self.out_height, self.out_width
        s = check_settings(**settings)
        pl = _lib.OpList()
        op, keep = ops.frame_detail_gain(frame, source, self.gains, H=H, W=W, r=s["radius"], E=edge_E(s["radius"], s["eps"]))
        pl.append(op, *keep)
        op, keep = ops.frame_resize(source, self.low, self.rx, self.ry, B=1, H=H, W=W, Ho=Ho, Wo=Wo)
        pl.append(op, *keep)
        op, keep = ops.frame_detail(S_dev, camera, self.low[0], self.gains, self.tx, self.ty, self.dev[0], H=H, W=W, Ho=Ho, Wo=Wo,
                                    k=gain_scale(s["radius"], s["strength"]), limit=np.float32(s["limit"]), show=s["show"])
        pl.append(op, *keep)
        return pl

    def _plan(self, S_dev, frame, source, camera, settings):
        key = (S_dev.data_ptr(), frame.data_ptr(), frame.dtype, source.data_ptr(), camera.data_ptr(), tuple(sorted(settings.items())))
        pl = self._plans.get(key)
        if pl is None:
            pl = self.plan(S_dev, frame, source, camera, settings)
            if key in self._seen:
                if len(self._plans) >= self.MAX_PLANS:
                    self._plans.clear()
                self._plans[key] = pl
            self._seen = (self._seen + (key,))[-self.MAX_PLANS:]
        return pl

    def apply(self, S_dev: torch.Tensor, frame: torch.Tensor, slot, settings: dict, to_host: bool = True):
        """`S_dev`: the uint8 [Ho,Wo,3] device frame L2D_OP_FRAME_RESIZE made of `frame` (fp16 [3,H,W] or uint8 [H,W,3], on the
        device) + the `MatteLine` slot of the frame, which carries its source frame and its camera buffer -> uint8 [Ho,Wo,3]: a
        numpy view of the pinned buffer (valid until the next call), or with `to_host=False` the static device tensor"""
        H, W, Ho, Wo = self.height, self.width, self.out_height, self.out_width
        camera = slot.camera.data
        for name, t in (("styled", S_dev), ("camera", camera)):
            if t.dtype != torch.uint8 or tuple(t.shape) != (Ho, Wo, 3) or not t.is_contiguous():
                raise ValueError(f"detail: expected a contiguous uint8 [{Ho},{Wo},3] {name} frame, got {t.dtype} {tuple(t.shape)}")
        ok = (frame.dtype == torch.float16 and tuple(frame.shape) == (3, H, W)) or \
             (frame.dtype == torch.uint8 and tuple(frame.shape) == (H, W, 3))
        if not ok:
            raise ValueError(f"detail: expected fp16 [3,{H},{W}] or uint8 [{H},{W},3], got {frame.dtype} {tuple(frame.shape)}")
        if not frame.is_contiguous():
            frame = frame.contiguous()
        self._plan(S_dev, frame, slot.source, camera, settings).run()
        if not to_host:
            return self.dev[0]
        return to_pinned(self.dev, self.host)[0]
