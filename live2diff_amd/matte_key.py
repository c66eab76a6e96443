"""The matte key (csrc/matte_key.hip): cut the frame by a colour or by a clean plate.  Every pixel of the
frame's source is compared, on the bytes a viewer would see, against a key colour (a green or blue screen) or against a plate --
a picture of the empty room taken by a camera that does not move.  Where the pixel differs from the key is the subject.  The
result is the raw matte plane of the output chain, fp32 [H,W] in [0, 1] at the stream's size, in place of the smoothstep ramp
over the frame's depth or combined with it, exactly as `mask_io` hands in a caller's mask: everything behind the raw matte (edge
refit, hold, feather, backdrop, both composites, `show`) reads the plane as it reads the ramp.  A key needs no model and no
depth.  The reference has no counterpart.

`key_ref` (numpy) states the arithmetic: exact integers up to the window sum, then a few fp32 steps, each rounded on its own, no
fma.  With `mask_io.front_ref` it is the oracle of L2D_OP_MATTE_KEY, bit for bit, and what the wrapper computes on CPU tensors.
`HipMatteKey` owns the plane and the plate of one stream; L2D_OP_FRAME_PLANAR_BYTES captures a plate from a frame's source.

`lo` and `hi` are in byte levels of the colour distance: at or below `lo` a pixel counts as the key (matte 0), at or above `hi`
as the subject (matte 1), a smoothstep over the squared distance in between.  `luma` in [0, 1] weighs the brightness difference
in: 0 ignores it, so a shadow on the screen stays screen.  `DEFAULTS` are a guess made on a synthetic green-screen frame; they
are NOT tuned on camera footage (as the matte hold's are not)."""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .mask_io import COMBINES, front_ref
from .steady import source_bytes, window_sum

MAX_RADIUS = ops.MATTE_KEY_MAX_R
MAX_LEVEL = 1024
# untuned on camera footage: a colour key ignores brightness (a shadow on the screen stays screen); a plate weighs it in, because a
# grey subject in front of a grey wall differs in little else
DEFAULTS = dict(lo=40.0, hi=90.0, luma=0.0, radius=1, combine="replace", invert=False)
PLATE_DEFAULTS = dict(DEFAULTS, luma=0.25)
MAX_D = 2 * 510 * 510 + 255 * 255                 # |cb|, |cr| <= 510, (L dy^2 + 128) >> 8 <= 255^2 with L <= 256: 585,225 < 2^20


# ----------------------------------------------------------------------------- settings
def _number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(float(v))


def is_color(to) -> bool:
    return (isinstance(to, (tuple, list)) and len(to) == 3
            and all(not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) for v in to))


def check_settings(lo=None, hi=None, luma=None, radius=1, combine="replace", invert=False, plate: bool = False) -> dict:
    """{lo, hi, luma, radius, combine, invert} validated, None -> the default of a colour key or (`plate`) of a plate key;
    ValueError names the keyword"""
    d = PLATE_DEFAULTS if plate else DEFAULTS
    lo, hi, luma = (d["lo"] if lo is None else lo), (d["hi"] if hi is None else hi), (d["luma"] if luma is None else luma)
    for name, v in (("lo", lo), ("hi", hi)):
        if not _number(v) or not 0.0 <= float(v) <= MAX_LEVEL:
            raise ValueError(f"matte key: {name}={v!r}: use a number in [0, {MAX_LEVEL}] (byte levels of the colour distance)")
    if float(lo) > float(hi):
        raise ValueError(f"matte key: lo={lo!r} is above hi={hi!r}")
    if not _number(luma) or not 0.0 <= float(luma) <= 1.0:
        raise ValueError(f"matte key: luma={luma!r}: use a number in [0, 1]")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"matte key: radius={radius!r}: use an integer from 0 to {MAX_RADIUS}")
    if not isinstance(combine, str) or combine not in COMBINES:
        raise ValueError(f"matte key: combine={combine!r}: use 'replace' (the key alone), 'and' (ramp and key) or 'or'")
    if not isinstance(invert, (bool, np.bool_)):
        raise ValueError(f"matte key: invert={invert!r}: use True or False")
    return dict(lo=float(lo), hi=float(hi), luma=float(luma), radius=int(radius), combine=combine, invert=bool(invert))


def check_color(to) -> Tuple[int, int, int]:
    if not is_color(to) or not all(0 <= int(v) <= 255 for v in to):
        raise ValueError(f"matte key: to={to!r}: a colour is an (r, g, b) triple of integers in 0..255")
    return tuple(int(v) for v in to)


def key_params(lo: float, hi: float) -> Tuple[np.float32, np.float32, bool]:
    """(lo2, inv, hard) of the key's ramp over the mean squared distance, computed in Python doubles as `matte.matte_params`
    computes its own: lo2 = float32(lo^2), inv = float32(1 / (hi^2 - lo^2)); hi <= lo, or an inverse that is not finite, is a
    step (`hard`, inv = 0)"""
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= MAX_LEVEL and 0.0 <= hi <= MAX_LEVEL):
        raise ValueError(f"matte key: lo={lo!r}, hi={hi!r} must lie in [0, {MAX_LEVEL}]")
    if lo > hi:
        raise ValueError(f"matte key: lo={lo!r} is above hi={hi!r}")
    den = hi * hi - lo * lo
    hard = hi <= lo or den <= 0.0
    with np.errstate(over="ignore"):
        inv = np.float32(0.0) if hard else np.float32(1.0 / den)
    if not np.isfinite(inv) or inv == 0.0:
        hard, inv = True, np.float32(0.0)
    return np.float32(lo * lo), inv, bool(hard)


def luma_weight(luma: float) -> int:
    """L = rint(256 luma) in 0..256"""
    luma = float(luma)
    if not 0.0 <= luma <= 1.0:
        raise ValueError(f"matte key: luma={luma!r}: use a number in [0, 1]")
    return int(np.rint(256.0 * luma))


# ----------------------------------------------------------------------------- the oracle (numpy)
def _key_planes(key, shape) -> np.ndarray:
    k = np.asarray(key.detach().cpu().numpy() if torch.is_tensor(key) else key)
    if k.shape == (3,):
        if k.dtype.kind not in "iu" or k.min() < 0 or k.max() > 255:
            raise ValueError(f"matte key: a colour is three bytes, got {key!r}")
        return np.broadcast_to(k.astype(np.int64)[:, None, None], shape)
    if k.dtype != np.uint8 or k.shape != tuple(shape):
        raise ValueError(f"matte key: a plate is a planar uint8 {list(shape)} array, got {k.dtype} {k.shape}")
    return k.astype(np.int64)


def distance_ref(b, key, luma: float = 0.0) -> np.ndarray:
    """int64 [H,W] D of the planar uint8 [3,H,W] bytes `b` against the key: dR, dG, dB = b - k; dy = (77 dR + 150 dG + 29 dB +
    128) >> 8 (arithmetic: towards minus infinity); cb = dB - dy, cr = dR - dy; D = cb^2 + cr^2 + ((L dy^2 + 128) >> 8)"""
    b = np.asarray(b)
    if b.dtype != np.uint8 or b.ndim != 3 or b.shape[0] != 3:
        raise ValueError(f"matte key: expected planar uint8 [3,H,W] bytes, got {b.dtype} {b.shape}")
    L = luma_weight(luma)
    d = b.astype(np.int64) - _key_planes(key, b.shape)
    dR, dG, dB = d[0], d[1], d[2]
    dy = (77 * dR + 150 * dG + 29 * dB + 128) >> 8
    cb, cr = dB - dy, dR - dy
    D = cb * cb + cr * cr + ((L * dy * dy + 128) >> 8)
    assert D.min() >= 0 and D.max() <= MAX_D < 1 << 20
    return D


def plane_of(D, *, lo: float, hi: float, radius: int = 1, invert: bool = False) -> np.ndarray:
    """uint8 [H,W] P of the distances `D`: S = `steady.window_sum(D, radius)`; mean = float32(S) / float32((2r+1)^2); t =
    clamp((mean - lo2) inv, 0, 1) (hard: mean >= lo2); m = (t t)(3 - 2 t); P = rint(255 m), half to even; `invert`: 255 - P"""
    r = int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"matte key: radius={radius!r}: use an integer from 0 to {MAX_RADIUS}")
    lo2, inv, hard = key_params(lo, hi)
    S = window_sum(D, r)
    assert S.min() >= 0 and S.max() < 1 << 31
    mean = S.astype(np.float32) / np.float32((2 * r + 1) ** 2)
    one, zero = np.float32(1.0), np.float32(0.0)
    if hard:
        t = np.where(mean >= lo2, one, zero).astype(np.float32)
    else:
        t = np.minimum(np.maximum((mean - lo2) * inv, zero), one)
    m = (t * t) * (np.float32(3.0) - np.float32(2.0) * t)
    assert m.dtype == np.float32
    P = np.ascontiguousarray(np.rint(np.float32(255.0) * m).astype(np.uint8))
    return (np.uint8(255) - P) if invert else P


def key_ref(source, key, *, lo: float, hi: float, luma: float = 0.0, radius: int = 1, invert: bool = False) -> np.ndarray:
    """uint8 [H,W] plane P of the finite fp16 [3,H,W] frame `source` against `key` (three bytes, or a plate as planar uint8
    [3,H,W]): `plane_of(distance_ref(steady.source_bytes(source), key, luma), ...)`.  255: differs from the key -- the subject,
    which the matte formula source + m (styled - source) stylises."""
    return plane_of(distance_ref(source_bytes(source), key, luma), lo=lo, hi=hi, radius=radius, invert=invert)


def raw_ref(source, key, depth, matte: dict, key_settings: dict) -> np.ndarray:
    """fp32 [H,W]: `mask_io.front_ref(key_ref(...))` under the matte's and the key's settings -- op 59 on the host"""
    s = key_settings
    P = key_ref(source, key, lo=s["lo"], hi=s["hi"], luma=s["luma"], radius=s["radius"], invert=s["invert"])
    return front_ref(P, depth, matte["lo"], matte["hi"], matte["keep"], s["combine"])


def plate_ref(image, H: int, W: int, resample: str = "lanczos") -> np.ndarray:
    """planar uint8 [3,H,W]: `backdrop.image_ref` (the largest centred window of the stream's aspect ratio, resampled to the
    stream's size) transposed -- a plate from an array, a PIL image or a path"""
    from .backdrop import image_ref
    return np.ascontiguousarray(image_ref(image, H, W, resample).transpose(2, 0, 1))


# ----------------------------------------------------------------------------- the device side
class HipMatteKey:
    """The raw matte plane and the plate of one `(H, W)` stream.  `record(slot, matte, settings)` gives the records that write
    `plane` from a `MatteLine` slot's source: L2D_OP_MATTE_KEY against `settings["to"]` (a colour) or the plate, with `capture`
    L2D_OP_FRAME_PLANAR_BYTES of the same source in front of it, which makes that frame the plate.  The composites put the
    records at the head of their `OpList`; nothing is zeroed: every launch writes the whole plane (and a capture the whole
    plate).  `plane` and `plate` may be the caller's: tests place them inside guarded buffers."""

    def __init__(self, height: int, width: int, device="cuda:0", plane=None, plate=None):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipMatteKey: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.plane = plane if plane is not None else torch.empty(self.height, self.width, dtype=torch.float32, device=self.device)
        self.plate = plate                   # planar uint8 [3,H,W], made by the first `set_plate` or capture
        self.has_plate = False

    def _plate(self) -> torch.Tensor:
        if self.plate is None:
            self.plate = torch.empty(3, self.height, self.width, dtype=torch.uint8, device=self.device)
        return self.plate

    def set_plate(self, planar) -> None:
        """a planar uint8 [3,H,W] array or tensor becomes the plate (a copy on the current stream)"""
        t = planar if torch.is_tensor(planar) else torch.from_numpy(np.array(planar, order="C"))       # (a copy: the caller's may be read-only)
        if t.dtype != torch.uint8 or tuple(t.shape) != (3, self.height, self.width):
            raise ValueError(f"HipMatteKey: a plate is planar uint8 [3,{self.height},{self.width}], got {t.dtype} {tuple(t.shape)}")
        self._plate().copy_(t, non_blocking=t.is_cuda)
        self.has_plate = True

    def record(self, slot, matte: dict, settings: dict, capture: bool = False, out: Optional[torch.Tensor] = None):
        """(records, keep, plane): `slot.source` (and with "and" / "or" `slot.depth` under the matte's ramp) under the key's
        `settings` ({to: a colour or "plate", lo, hi, luma, radius, combine, invert}) -> `plane`; `records` is a list of L2D
        records, `keep` the tensors they name"""
        from .matte import matte_params
        H, W = self.height, self.width
        s = check_settings(settings["lo"], settings["hi"], settings["luma"], settings["radius"], settings["combine"], settings["invert"])
        records, keep = [], []
        to = settings["to"]
        if capture:
            op, k = ops.frame_planar_bytes(slot.source, self._plate(), H=H, W=W)
            records.append(op)
            keep.extend(k)
            self.has_plate = True
            to = "plate"
        if isinstance(to, str):
            if to != "plate" or not self.has_plate:
                raise ValueError(f"HipMatteKey: to={to!r}: no plate is set (set_plate, or a capture)")
            key = self.plate
        else:
            key = check_color(to)
        lo2, inv, hard = key_params(s["lo"], s["hi"])
        kw = {}
        if s["combine"] != "replace":
            lo32, inv32, ramp_hard = matte_params(matte["lo"], matte["hi"])
            kw = dict(lo32=lo32, inv32=inv32, ramp_hard=ramp_hard, far=matte["keep"] == "far")
        plane = self.plane if out is None else out
        op, k = ops.matte_key(slot.source, plane, slot.depth, key, H=H, W=W, r=s["radius"], L=luma_weight(s["luma"]), lo2=lo2, inv=inv,
                              hard=hard, combine=s["combine"], invert=s["invert"], **kw)
        records.append(op)
        keep.extend(k)
        return records, tuple(keep), plane

    def key(self, source: torch.Tensor, depth: Optional[torch.Tensor], matte: dict, settings: dict, capture: bool = False,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one fp16 [3,H,W] source frame (and its fp16 [H,W] depth plane) -> the raw matte plane, in one run on the current
        stream (tests and tools; the wrapper goes through the delay line and `record`)"""
        import types
        records, keep, plane = self.record(types.SimpleNamespace(source=source, depth=depth), matte, settings, capture, out)
        pl = _lib.OpList()
        for j, op in enumerate(records):
            pl.append(op, *(keep if j == 0 else ()))
        pl.run()
        return plane
