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
are NOT tuned on camera footage (as the matte hold's are not).

The adaptive plate: a plate is a frozen record, and a cloud, a lamp warming up or a camera's exposure
settling moves every background pixel off it.  With adaptation the plate is a state, uint16 [3,H,W] in 8.8 fixed point, that
moves after each keyed frame a little towards the frame's source where the key says "background" (`rate`) and not, or much more
slowly, where it says "subject" (`absorb`).  `key_adapt_ref` restates L2D_OP_MATTE_KEY_ADAPT in exact integers; with both rates 0
it is `key_ref` against the plate on every frame.  `ADAPT_DEFAULTS` are a guess too, untuned on camera footage.

The plate gain: a camera's auto-exposure or auto-white-balance moves every background pixel at once,
and the adaptive plate follows only at `rate`.  With the gain every keyed frame first measures one gain per channel between the
plate and the frame's source -- the lower median of the per-pixel ratios b / k in units of 1 / 128 (`gain_hist_ref`, `gain_of`)
-- and is then keyed against the plate times that gain (`gain_plate`).  A gain of 128 is unity and gives the plate's own bytes,
so `key_ref` and `key_adapt_ref` with `gain=(128, 128, 128)` are what they are without.  The median holds while the subject
covers less than half of the valid samples; past that it measures the subject (see `gain_of`).  `GAIN_DEFAULTS` are a guess."""
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
ADAPT_DEFAULTS = dict(rate=1.0 / 32.0, absorb=0.0)        # untuned on camera footage
MAX_RATE = 0.5                                    # the state moves at most half way per frame
MAX_STATE = 255 * 256                             # a plate byte in 8.8 fixed point
GAIN_DEFAULTS = dict(limit=2.0, min_share=1.0 / 16.0)      # untuned on camera footage
GAIN_UNITY = ops.MATTE_KEY_GAIN_UNITY             # a gain is an integer in units of 1 / 128
GAIN_BINS = ops.MATTE_KEY_GAIN_BINS               # the ratios 0 .. 511; 511 holds everything above
MAX_GAIN_LIMIT = 3.99                             # lim = rint(128 limit) <= 511
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


def check_adapt(rate=ADAPT_DEFAULTS["rate"], absorb=ADAPT_DEFAULTS["absorb"]) -> dict:
    """{rate, absorb} validated; ValueError names the keyword"""
    for name, v in (("rate", rate), ("absorb", absorb)):
        if not _number(v) or not 0.0 <= float(v) <= MAX_RATE:
            raise ValueError(f"matte key adapt: {name}={v!r}: use a number in [0, {MAX_RATE}] (the part of the way the plate moves per frame)")
    return dict(rate=float(rate), absorb=float(absorb))


def adapt_params(rate: float, absorb: float = 0.0) -> Tuple[int, int]:
    """(a_bg, a_fg) = (rint(65536 rate), rint(65536 absorb)), both in 0..32768"""
    s = check_adapt(rate, absorb)
    a_bg, a_fg = int(np.rint(65536.0 * s["rate"])), int(np.rint(65536.0 * s["absorb"]))
    assert 0 <= a_bg <= ops.MATTE_KEY_MAX_RATE and 0 <= a_fg <= ops.MATTE_KEY_MAX_RATE
    return a_bg, a_fg


def check_gain(limit=GAIN_DEFAULTS["limit"], min_share=GAIN_DEFAULTS["min_share"]) -> dict:
    """{limit, min_share} validated; ValueError names the keyword"""
    if not _number(limit) or not 1.0 <= float(limit) <= MAX_GAIN_LIMIT:
        raise ValueError(f"matte key gain: limit={limit!r}: use a number in [1, {MAX_GAIN_LIMIT}] (the largest gain, and 1 / the smallest)")
    if not _number(min_share) or not 0.0 <= float(min_share) <= 1.0:
        raise ValueError(f"matte key gain: min_share={min_share!r}: use a number in [0, 1] (the part of the frame's pixels a channel "
                         "needs as valid samples)")
    return dict(limit=float(limit), min_share=float(min_share))


def gain_params(limit: float, min_share: float, H: int, W: int) -> Tuple[int, int]:
    """(lim, min_count) = (rint(128 limit), ceil(min_share H W)): 128 <= lim <= 511, 0 <= min_count <= H W"""
    s = check_gain(limit, min_share)
    lim, min_count = int(np.rint(128.0 * s["limit"])), int(np.ceil(s["min_share"] * H * W))
    assert GAIN_UNITY <= lim < GAIN_BINS and 0 <= min_count <= H * W
    return lim, min_count


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


def key_ref(source, key, *, lo: float, hi: float, luma: float = 0.0, radius: int = 1, invert: bool = False, gain=None) -> np.ndarray:
    """uint8 [H,W] plane P of the finite fp16 [3,H,W] frame `source` against `key` (three bytes, or a plate as planar uint8
    [3,H,W]): `plane_of(distance_ref(steady.source_bytes(source), key, luma), ...)`.  255: differs from the key -- the subject,
    which the matte formula source + m (styled - source) stylises.  `gain` (three integers, 128: unity; a plate only): against
    `gain_plate(key, gain)`."""
    if gain is not None:
        key = gain_plate(key.detach().cpu().numpy() if torch.is_tensor(key) else key, gain)
    return plane_of(distance_ref(source_bytes(source), key, luma), lo=lo, hi=hi, radius=radius, invert=invert)


def raw_ref(source, key, depth, matte: dict, key_settings: dict, gain=None) -> np.ndarray:
    """fp32 [H,W]: `mask_io.front_ref(key_ref(...))` under the matte's and the key's settings -- op 59 on the host (`gain`: under
    L2D_MATTE_KEY_GAIN with that record)"""
    s = key_settings
    P = key_ref(source, key, lo=s["lo"], hi=s["hi"], luma=s["luma"], radius=s["radius"], invert=s["invert"], gain=gain)
    return front_ref(P, depth, matte["lo"], matte["hi"], matte["keep"], s["combine"])


# ----------------------------------------------------------------------------- the adaptive plate's oracle (numpy)
def _state(state) -> np.ndarray:
    s = np.asarray(state.detach().cpu().numpy() if torch.is_tensor(state) else state)
    if s.dtype == np.int16:                       # (the bits of uint16 words)
        s = s.view(np.uint16)
    if s.dtype != np.uint16 or s.ndim != 3 or s.shape[0] != 3 or (s.size and int(s.max()) > MAX_STATE):
        raise ValueError(f"matte key adapt: a state is planar uint16 [3,H,W] with values up to {MAX_STATE}, got {s.dtype} {s.shape}")
    return s


def state_of(plate) -> np.ndarray:
    """uint16 [3,H,W]: s = 256 k of a plate that arrives as planar uint8 bytes; `plate_bytes(state_of(k)) == k`"""
    k = np.asarray(plate)
    if k.dtype != np.uint8 or k.ndim != 3 or k.shape[0] != 3:
        raise ValueError(f"matte key adapt: a plate is a planar uint8 [3,H,W] array, got {k.dtype} {k.shape}")
    return (k.astype(np.uint16) << 8).astype(np.uint16)


def plate_bytes(state) -> np.ndarray:
    """uint8 [3,H,W]: k = (s + 128) >> 8, the plate byte the key compares against"""
    return ((_state(state).astype(np.int64) + 128) >> 8).astype(np.uint8)


def adapt_ref(state, source_bytes_, P0, a_bg: int, a_fg: int) -> np.ndarray:
    """uint16 [3,H,W] s': a = (a_bg (255 - P0) + a_fg P0 + 127) // 255 per pixel, with P0 the uint8 [H,W] plane in front of
    `invert`; per channel e = 256 b - s, s' = s + ((a e + 32768) >> 16), the shift arithmetic (towards minus infinity)"""
    s = _state(state).astype(np.int64)
    b = np.asarray(source_bytes_)
    P0 = np.asarray(P0)
    if b.dtype != np.uint8 or b.shape != s.shape or P0.dtype != np.uint8 or P0.shape != s.shape[1:]:
        raise ValueError(f"matte key adapt: expected uint8 {s.shape} bytes and a uint8 {s.shape[1:]} plane, got {b.dtype} {b.shape}, "
                         f"{P0.dtype} {P0.shape}")
    for name, v in (("a_bg", a_bg), ("a_fg", a_fg)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= ops.MATTE_KEY_MAX_RATE:
            raise ValueError(f"matte key adapt: {name}={v!r}: use an integer from 0 to {ops.MATTE_KEY_MAX_RATE}")
    p = P0.astype(np.int64)
    a = (int(a_bg) * (255 - p) + int(a_fg) * p + 127) // 255
    e = 256 * b.astype(np.int64) - s
    t = a[None] * e + 32768
    assert np.abs(e).max(initial=0) <= MAX_STATE and a.max(initial=0) <= ops.MATTE_KEY_MAX_RATE
    assert np.abs(a[None] * e).max(initial=0) + 32768 <= ops.MATTE_KEY_MAX_RATE * MAX_STATE + 32768 == 2139127808 < 1 << 31
    n = s + (t >> 16)
    assert n.min(initial=0) >= 0 and n.max(initial=0) <= MAX_STATE
    return n.astype(np.uint16)


def key_adapt_ref(source, state, *, lo: float, hi: float, luma: float = 0.0, radius: int = 1, invert: bool = False,
                  rate: float = ADAPT_DEFAULTS["rate"], absorb: float = ADAPT_DEFAULTS["absorb"], gain=None) -> Tuple[np.ndarray, np.ndarray]:
    """(P, s'): the plane `key_ref` gives against `plate_bytes(state)`, and the state moved towards the source's bytes under
    that plane in front of `invert` -- L2D_OP_MATTE_KEY_ADAPT without the depth ramp.  `gain`: the key is formed against
    `gain_plate(plate_bytes(state), gain)`; the update is unchanged, e = 256 b - s, towards the frame's own bytes."""
    a_bg, a_fg = adapt_params(rate, absorb)
    b = source_bytes(source)
    k = plate_bytes(state) if gain is None else gain_plate(plate_bytes(state), gain)
    P0 = plane_of(distance_ref(b, k, luma), lo=lo, hi=hi, radius=radius)
    return ((np.uint8(255) - P0) if invert else P0), adapt_ref(state, b, P0, a_bg, a_fg)


def raw_adapt_ref(source, state, depth, matte: dict, key_settings: dict, adapt: dict, gain=None) -> Tuple[np.ndarray, np.ndarray]:
    """(fp32 [H,W], s'): `mask_io.front_ref` of `key_adapt_ref`'s plane under the matte's and the key's settings, and the next
    state -- op 61 on the host"""
    s = key_settings
    P, nxt = key_adapt_ref(source, state, lo=s["lo"], hi=s["hi"], luma=s["luma"], radius=s["radius"], invert=s["invert"],
                           rate=adapt["rate"], absorb=adapt["absorb"], gain=gain)
    return front_ref(P, depth, matte["lo"], matte["hi"], matte["keep"], s["combine"]), nxt


# ----------------------------------------------------------------------------- the plate gain's oracle (numpy)
def _bytes3(name, a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"matte key gain: {name}: expected planar uint8 [3,H,W] bytes, got {a.dtype} {a.shape}")
    return a


def gain_hist_ref(b, k) -> np.ndarray:
    """int64 [3,512] hist of the source's planar uint8 [3,H,W] bytes `b` against the plate's bytes `k`: per pixel and channel
    the sample is valid when 16 <= k <= 239 and 4 <= b <= 251 (a clipped or near-black value says nothing about a ratio); q =
    min(511, (128 b + (k >> 1)) // k), the ratio b / k in units of 1 / 128 rounded to nearest (b == k: exactly 128); hist[c][q]
    counts the valid samples -- L2D_OP_MATTE_KEY_GAIN_HIST summed over its blocks"""
    b, k = _bytes3("b", b).astype(np.int64), _bytes3("k", k).astype(np.int64)
    if b.shape != k.shape:
        raise ValueError(f"matte key gain: the bytes {b.shape} and the plate {k.shape} differ in shape")
    assert 3 * b[0].size < 1 << 31                # every count is at most H W
    valid = (k >= 16) & (k <= 239) & (b >= 4) & (b <= 251)
    q = np.minimum(GAIN_BINS - 1, (128 * b + (k >> 1)) // np.maximum(k, 1))
    hist = np.zeros((3, GAIN_BINS), np.int64)
    for c in range(3):
        hist[c] = np.bincount(q[c][valid[c]], minlength=GAIN_BINS)
    return hist


def gain_of(hist, lim: int, min_count: int) -> Tuple[np.ndarray, np.ndarray]:
    """(g, n), int64 [3] each, of a [3,512] histogram: n_c = the samples of channel c; g_c = 128 if n_c < min_count, else the
    smallest q with 2 cum_c(q) >= n_c (the lower median), clamped to [ceil(16384 / lim), lim] -- L2D_OP_MATTE_KEY_GAIN.

    The median is the subject's guard: it is the background's ratio while the subject (whose ratios lie anywhere) covers less
    than half of the valid samples.  Past that it is not: with a subject over 60 % of the frame the measured gains are the
    subject's against the wall behind it, and the key is wrong everywhere.  Nothing here detects that; `limit` only bounds it."""
    h = np.asarray(hist)
    if h.shape != (3, GAIN_BINS) or h.dtype.kind not in "iu" or (h.size and int(h.min()) < 0):
        raise ValueError(f"matte key gain: a histogram is [3,{GAIN_BINS}] counts, got {h.dtype} {h.shape}")
    for name, v, lo, hi in (("lim", lim, GAIN_UNITY, GAIN_BINS - 1), ("min_count", min_count, 0, (1 << 31) - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"matte key gain: {name}={v!r}: use an integer from {lo} to {hi}")
    h = h.astype(np.int64)
    cum = np.cumsum(h, axis=1)
    n = cum[:, -1]
    assert 3 * int(n.max(initial=0)) < 1 << 31    # 2 cum fits 32 bits
    lim = int(lim)
    lo = -(-GAIN_UNITY * GAIN_UNITY // lim)       # ceil(16384 / lim)
    g = np.empty(3, np.int64)
    for c in range(3):
        g[c] = GAIN_UNITY if n[c] < int(min_count) else min(max(int(np.argmax(2 * cum[c] >= n[c])), lo), lim)
    return g, n


def _gain3(gain) -> np.ndarray:
    g = np.asarray(gain)
    if g.shape != (3,) or g.dtype.kind not in "iu" or int(g.min()) < 0 or int(g.max()) >= GAIN_BINS:
        raise ValueError(f"matte key gain: a gain is three integers in 0..{GAIN_BINS - 1} (128: unity), got {gain!r}")
    return g.astype(np.int64)


def gain_plate(k, g) -> np.ndarray:
    """uint8 [3,H,W] k' = min(255, (g_c k + 64) >> 7): the plate's bytes under the gains `g` (g = 128: k itself)"""
    t = _gain3(g)[:, None, None] * _bytes3("k", k).astype(np.int64) + 64
    assert t.max(initial=0) <= (GAIN_BINS - 1) * 255 + 64 < 1 << 17
    return np.minimum(255, t >> 7).astype(np.uint8)


def measure_gain(b, k, lim: int, min_count: int) -> Tuple[np.ndarray, np.ndarray]:
    """(g, n) = `gain_of(gain_hist_ref(b, k), lim, min_count)`"""
    return gain_of(gain_hist_ref(b, k), lim, min_count)



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
    plate).  `plane` and `plate` may be the caller's: tests place them inside guarded buffers.

    With `adapt` ({rate, absorb}) `record` gives L2D_OP_MATTE_KEY_ADAPT in place of L2D_OP_MATTE_KEY: the plate lives in two
    uint16 records that ping-pong (`states`, the caller's or made on first use; `cur` is the one the next launch reads), and
    starts from the plate's bytes on the first frame behind `set_plate`, a capture or `restart`.  `repeated` runs the launch
    with both rates 0, so that the plate is not fed the same frame twice.

    With `gain` ({limit, min_share}) `record` puts L2D_OP_MATTE_KEY_GAIN_HIST and L2D_OP_MATTE_KEY_GAIN in front of the key's
    launch and sets L2D_MATTE_KEY_GAIN on it: the frame is keyed against the plate (or the state read) times the gains just
    measured.  `partials` and `gain_record` are the caller's or made on first use; nothing is accumulated from frame to frame."""

    def __init__(self, height: int, width: int, device="cuda:0", plane=None, plate=None, states=None, partials=None, gain_record=None):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipMatteKey: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.plane = plane if plane is not None else torch.empty(self.height, self.width, dtype=torch.float32, device=self.device)
        self.plate = plate                   # planar uint8 [3,H,W], made by the first `set_plate` or capture
        self.has_plate = False
        self.states = list(states) if states is not None else [None, None]       # planar uint16 [3,H,W] each, 8.8 fixed point
        self.cur = 0                         # the record the next adaptive launch reads
        self.from_plate = True               # the next adaptive frame starts from the plate's bytes
        self.partials = partials             # uint32 [nblk,3,512] (as int32 bits): every block's histogram of the ratios
        self.gain_record = gain_record       # int32 [8]: {g_r, g_g, g_b, n_r, n_g, n_b, 0, 0}
        self.has_gain = False                # a record with `gain=` has been built: the record holds (or will hold) a measurement

    def _gain_buffers(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.partials is None:
            self.partials = torch.empty(ops.matte_key_gain_blocks(self.height, self.width), 3, GAIN_BINS, dtype=torch.int32, device=self.device)
        if self.gain_record is None:
            self.gain_record = torch.empty(8, dtype=torch.int32, device=self.device)
        return self.partials, self.gain_record

    def current_gain(self) -> Tuple[np.ndarray, np.ndarray]:
        """(g, n), int64 [3] each: the gains (128: unity) and the valid samples of the last keyed frame, copied to the host (a
        copy that waits for the device)"""
        if not self.has_gain:
            raise ValueError("HipMatteKey: no gain has been measured (record with gain=)")
        r = self.gain_record.cpu().numpy().astype(np.int64)
        return r[:3].copy(), r[3:6].copy()

    def _state(self, j: int) -> torch.Tensor:
        if self.states[j] is None:
            self.states[j] = torch.empty(3, self.height, self.width, dtype=torch.uint16, device=self.device)
        return self.states[j]

    def restart(self) -> None:
        """the next adaptive frame starts from the plate's bytes again"""
        self.from_plate = True

    def current_plate(self) -> np.ndarray:
        """the plate of this moment on the host, uint8 [H,W,3]: `plate_bytes` of the state while one runs, else the plate's own
        bytes (a copy that waits for the device)"""
        if not self.has_plate:
            raise ValueError("HipMatteKey: no plate is set (set_plate, or a capture)")
        k = self.plate.cpu().numpy() if self.from_plate else plate_bytes(self._state(self.cur).cpu().numpy())
        return np.ascontiguousarray(k.transpose(1, 2, 0))

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
        self.from_plate = True

    def record(self, slot, matte: dict, settings: dict, capture: bool = False, out: Optional[torch.Tensor] = None,
               adapt: Optional[dict] = None, repeated: bool = False, gain: Optional[dict] = None):
        """(records, keep, plane): `slot.source` (and with "and" / "or" `slot.depth` under the matte's ramp) under the key's
        `settings` ({to: a colour or "plate", lo, hi, luma, radius, combine, invert}) -> `plane`; `records` is a list of L2D
        records, `keep` the tensors they name.  `adapt` ({rate, absorb}): the plate follows the source (op 61 in place of op 59;
        the records are good for one run each: the state advances with every call); `repeated`: with both rates 0.  `gain`
        ({limit, min_share}): ops 62 and 63 in front of the key's launch, which reads their record under L2D_MATTE_KEY_GAIN"""
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
            self.from_plate = True
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
        if gain is not None:
            if not isinstance(to, str):
                raise ValueError(f"HipMatteKey: to={to!r}: a gain needs a plate, not a colour")
            lim, min_count = gain_params(gain["limit"], gain["min_share"], H, W)
            partials, rec = self._gain_buffers()
            against = self._state(self.cur) if adapt is not None and not self.from_plate else self.plate
            for op, k in (ops.matte_key_gain_hist(slot.source, against, partials, H=H, W=W),
                          ops.matte_key_gain(partials, rec, H=H, W=W, lim=lim, min_count=min_count)):
                records.append(op)
                keep.extend(k)
            kw["gain"] = rec
            self.has_gain = True
        if adapt is not None:
            if not isinstance(to, str):
                raise ValueError(f"HipMatteKey: to={to!r}: adaptation needs a plate, not a colour")
            a_bg, a_fg = (0, 0) if repeated else adapt_params(adapt["rate"], adapt["absorb"])
            init = self.from_plate
            nxt = self.cur if init else 1 - self.cur
            op, k = ops.matte_key_adapt(slot.source, plane, slot.depth, self.plate if init else None, None if init else self._state(self.cur),
                                        self._state(nxt), H=H, W=W, r=s["radius"], L=luma_weight(s["luma"]), lo2=lo2, inv=inv, hard=hard,
                                        a_bg=a_bg, a_fg=a_fg, combine=s["combine"], invert=s["invert"], **kw)
            self.cur, self.from_plate = nxt, False
            records.append(op)
            keep.extend(k)
            return records, tuple(keep), plane
        op, k = ops.matte_key(slot.source, plane, slot.depth, key, H=H, W=W, r=s["radius"], L=luma_weight(s["luma"]), lo2=lo2, inv=inv,
                              hard=hard, combine=s["combine"], invert=s["invert"], **kw)
        records.append(op)
        keep.extend(k)
        return records, tuple(keep), plane

    def key(self, source: torch.Tensor, depth: Optional[torch.Tensor], matte: dict, settings: dict, capture: bool = False,
            out: Optional[torch.Tensor] = None, adapt: Optional[dict] = None, repeated: bool = False,
            gain: Optional[dict] = None) -> torch.Tensor:
        """one fp16 [3,H,W] source frame (and its fp16 [H,W] depth plane) -> the raw matte plane, in one run on the current
        stream (tests and tools; the wrapper goes through the delay line and `record`)"""
        import types
        records, keep, plane = self.record(types.SimpleNamespace(source=source, depth=depth), matte, settings, capture, out, adapt, repeated, gain)
        pl = _lib.OpList()
        for j, op in enumerate(records):
            pl.append(op, *(keep if j == 0 else ()))
        pl.run()
        return plane
