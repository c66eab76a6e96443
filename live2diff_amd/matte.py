"""Depth matte (csrc/matte.hip): stylise the near or the far part of the frame only.  Every frame pays
for a depth map that `encode_depth` turns into the UNet's conditioning and drops; here it also becomes a matte that composites
the stream's output over the stream's own source frame, on the device, in the launch that writes the uint8 frame.

  * `matte_params`, `matte_ref`, `composite_ref`   the arithmetic of L2D_OP_FRAME_MATTE in numpy float32 -- the kernel's oracle,
                      as `frame_io.egress_ref` and `style_bank.blend_ref` are.  Every step is one fp32 operation with one rounding
                      and no fused multiply-add, so the kernel is held to equality;
  * `check_settings`  the argument checks of `StreamAnimateDiffusionDepthWrapper.set_matte`;
  * `MatteLine`       the delay line: with N denoising steps the frame that leaves the stream at call t entered it at call
                      t - (N - 1), the ingested frame lives in a two-slot buffer, and in push / pop mode the depth path runs on
                      a side stream -- so source frames and depth planes are kept, delayed and consumed on the device;
  * `HipMatte`        the static output buffers and the one-op launch of one stream;
  * `up_table`, `matte_up_ref`, `composite_up_ref`, `HipMatteUp`   the matte at the output size: the
                      arithmetic of L2D_OP_FRAME_MATTE_UP -- the matte sampled bilinearly at the output size, the styled bytes
                      over the camera's own -- and its launch;
  * `check_edge`, `guide_ref`, `edge_ref`, `HipMatteEdge`   the edge-aware matte: the matte re-fitted
                      locally as a linear function of the source frame's luma (a guided filter), in exact integers and a few
                      individually rounded fp64 steps -- the arithmetic of L2D_OP_FRAME_MATTE_EDGE -- and its launch;
  * `check_hold`, `hold_ref`, `HipMatteHold`   the matte hold: the matte in front of the feather blended
                      with the previous held one where the source's bytes did not move (steady's weight, optionally along the
                      source's motion) -- the arithmetic of L2D_OP_FRAME_MATTE_HOLD -- and its records and launches.
"""
import collections
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .frame_io import to_pinned

MAX_FEATHER = ops.MATTE_MAX_R
MAX_EDGE_RADIUS = ops.MATTE_EDGE_MAX_R
SERVED_OUTPUT_TYPES = ("u8", "pil", "jpeg")


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy fp32)
def matte_params(lo: float, hi: float) -> Tuple[np.float32, np.float32, bool]:
    """(lo32, inv32, hard) of a ramp from `lo` to `hi`, both in [0, 1] in units of normalised inverse depth (0 = the farthest point
    of the frame, 1 = the nearest).  They are mapped to the depth tensor's [-1, 1] scale in Python doubles: lo_d = 2 lo - 1,
    hi_d = 2 hi - 1, lo32 = float32(lo_d), inv32 = float32(1 / (hi_d - lo_d)); hi_d <= lo_d is a step (`hard`, inv32 = 0)."""
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= 1.0 and 0.0 <= hi <= 1.0):
        raise ValueError(f"matte: lo={lo!r}, hi={hi!r} must lie in [0, 1]")
    if lo > hi:
        raise ValueError(f"matte: lo={lo!r} is above hi={hi!r}")
    lo_d, hi_d = 2.0 * lo - 1.0, 2.0 * hi - 1.0
    hard = hi_d <= lo_d
    inv = np.float32(0.0) if hard else np.float32(1.0 / (hi_d - lo_d))
    if not np.isfinite(inv):
        hard, inv = True, np.float32(0.0)
    return np.float32(lo_d), inv, bool(hard)


def _np16(x) -> np.ndarray:
    if torch.is_tensor(x):
        x = x.detach().cpu().to(torch.float16).numpy()
    return np.asarray(x, dtype=np.float16)


def _box_pass(m: np.ndarray, r: int, axis: int) -> np.ndarray:
    """one pass of the (2r+1) box along `axis`: edge replication, the taps added in increasing coordinate order, one division"""
    pad = [(0, 0)] * m.ndim
    pad[axis] = (r, r)
    p = np.pad(m, pad, mode="edge")
    n = m.shape[axis]
    acc = np.take(p, np.arange(0, n), axis=axis)
    for k in range(1, 2 * r + 1):
        acc = acc + np.take(p, np.arange(k, k + n), axis=axis)
    return acc / np.float32(2 * r + 1)


def matte_ref(depth, lo: float, hi: float, feather: int = 0, keep: str = "near", *, edge: Optional[dict] = None, source=None,
              plane=None) -> np.ndarray:
    """fp16 [B,H,W] depth planes (channel 0 of `encode_depth`'s `dn`: min-max normalised, in [-1, 1], at frame size) -> fp32
    [B,H,W] matte in [0, 1]: t = clamp((d - lo32) inv32, 0, 1) (hard: d >= lo32), m = (t t) (3 - 2 t), `keep="far"`: 1 - m, then
    the (2r+1) x (2r+1) box filter as a horizontal and a vertical pass.  `edge` ({radius, eps}, with the fp16 [B,3,H,W] `source`
    frames as the guide): `edge_ref` refines m in front of the box filter.  `plane` (fp32 [B,H,W]): a ready matte in front of
    the box filter, in place of the ramp and `edge` -- the host twin of L2D_MATTE_PLANE; `depth` is then not read."""
    check_settings(lo, hi, keep=keep, feather=feather)
    if plane is not None:
        m = np.asarray(plane.detach().cpu().numpy() if torch.is_tensor(plane) else plane)
        if m.dtype != np.float32 or m.ndim not in (2, 3):
            raise ValueError(f"matte_ref: plane: expected float32 [B,H,W], got {m.dtype} {m.shape}")
        m = m[None] if m.ndim == 2 else m
        if feather:
            m = _box_pass(_box_pass(m, feather, 2), feather, 1)
        assert m.dtype == np.float32
        return m
    lo32, inv32, hard = matte_params(lo, hi)
    d = _np16(depth).astype(np.float32)
    if d.ndim == 2:
        d = d[None]
    one, zero = np.float32(1.0), np.float32(0.0)
    if hard:
        t = np.where(d >= lo32, one, zero).astype(np.float32)
    else:
        t = np.minimum(np.maximum((d - lo32) * inv32, zero), one)
    m = (t * t) * (np.float32(3.0) - np.float32(2.0) * t)
    if keep == "far":
        m = one - m
    if edge is not None:
        if source is None:
            raise ValueError("matte_ref: an edge-aware matte needs the source frames as its guide")
        src = _np16(source)
        src = src[None] if src.ndim == 3 else src
        if src.shape[0] != m.shape[0]:
            raise ValueError(f"matte_ref: {m.shape[0]} depth planes, {src.shape[0]} source frames")
        m = np.stack([edge_ref(m[b], src[b], edge["radius"], edge["eps"]) for b in range(m.shape[0])])
    if feather:
        m = _box_pass(_box_pass(m, feather, 2), feather, 1)
    assert m.dtype == np.float32
    return m


# ----------------------------------------------------------------------------- edge-aware matte
EDGE_SHIFT = 4096              # the fixed point of the coefficients A and B: 12 fractional bits


def check_edge(radius=4, eps=10.0) -> dict:
    """the edge setting as {radius, eps}, or ValueError: `radius` no integer in 1..8, `eps` no finite number >= 1 (byte levels:
    the contrast of the guide below which a window counts as flat; from 1 on the coefficients fit 32 bits)"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_EDGE_RADIUS:
        raise ValueError(f"matte edge: radius={radius!r}: use an integer from 1 to {MAX_EDGE_RADIUS}")
    if (isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not np.isfinite(float(eps))
            or not 1.0 <= float(eps) <= 1.0e100):
        raise ValueError(f"matte edge: eps={eps!r}: use a finite number of byte levels, at least 1")
    return dict(radius=int(radius), eps=float(eps))


def edge_E(radius: int, eps: float) -> float:
    """E = double(n n) eps eps with n = (2 radius + 1)^2, in Python doubles: what the op carries in place of eps"""
    n = (2 * int(radius) + 1) ** 2
    return float(n * n) * float(eps) * float(eps)


def luma(x: np.ndarray) -> np.ndarray:
    """int64 [...]: (77 R + 150 G + 29 B + 128) >> 8 of uint8 [..., 3]"""
    b = np.asarray(x).astype(np.int64)
    return (77 * b[..., 0] + 150 * b[..., 1] + 29 * b[..., 2] + 128) >> 8


def guide_ref(source) -> np.ndarray:
    """int64 [H,W] in 0..255: the guide Y, the luma of the egress bytes of the fp16 [3,H,W] frame"""
    from .steady import source_bytes
    return luma(source_bytes(source).transpose(1, 2, 0))


def edge_coefficients(P: np.ndarray, Y: np.ndarray, radius: int, eps: float) -> Tuple[np.ndarray, np.ndarray]:
    """(A, B) int64 [H,W], both inside int32 (asserted): stage 1 of `edge_ref` on the integer planes P and Y in 0..255"""
    from .steady import window_sum
    r = int(radius)
    n = (2 * r + 1) ** 2
    P, Y = np.asarray(P).astype(np.int64), np.asarray(Y).astype(np.int64)
    S_I, S_P, S_II, S_IP = (window_sum(v, r) for v in (Y, P, Y * Y, Y * P))
    cov, var = n * S_IP - S_I * S_P, n * S_II - S_I * S_I
    assert int(np.abs(cov).max()) < 1 << 33 and 0 <= int(var.min()) and int(var.max()) < 1 << 33
    a = cov.astype(np.float64) / (var.astype(np.float64) + np.float64(edge_E(r, eps)))
    A = np.rint(a * np.float64(EDGE_SHIFT))
    prod = a * S_I.astype(np.float64)                       # (numpy: one multiplication, one subtraction, one division)
    bc = (S_P.astype(np.float64) - prod) / np.float64(n)
    B = np.rint(bc * np.float64(EDGE_SHIFT))
    assert float(np.abs(A).max()) < 2.0 ** 31 and float(np.abs(B).max()) < 2.0 ** 31
    return A.astype(np.int64), B.astype(np.int64)


def edge_ref(m0, source, radius: int, eps: float) -> np.ndarray:
    """L2D_OP_FRAME_MATTE_EDGE on the host: the fp32 [H,W] matte `m0` (`matte_ref` with feather 0: ramp and `keep` applied) and
    the fp16 [3,H,W] `source` frame -> fp32 [H,W], the matte re-fitted by the frame (a guided filter with the frame's luma as
    the guide).  P = rint(255 m0), Y = `guide_ref(source)`, n = (2r+1)^2; per pixel over the window (coordinates clamped)
    cov = n S_IP - S_I S_P and var = n S_II - S_I S_I in exact integers, a = double(cov) / (double(var) + E), A = rint(4096 a),
    bc = (double(S_P) - a double(S_I)) / double(n), B = rint(4096 bc); then Q = window_sum(A) Y + window_sum(B) in exact integers,
    q = double(Q) / double(n 4096 255), m' = float32(min(max(q, 0), 1)).  A constant m0 comes back as float32(P / 255): an
    all-near or all-far matte stays exactly 1 or 0."""
    from .steady import window_sum
    e = check_edge(radius, eps)
    r = e["radius"]
    n = (2 * r + 1) ** 2
    m0 = np.asarray(m0, dtype=np.float32)
    if m0.ndim != 2:
        raise ValueError(f"edge_ref: expected one [H,W] matte, got {m0.shape}")
    P = np.rint(m0 * np.float32(255.0)).astype(np.int64)
    Y = guide_ref(source)
    if Y.shape != P.shape:
        raise ValueError(f"edge_ref: the matte is {P.shape}, the source frame {Y.shape}")
    assert 0 <= int(P.min()) and int(P.max()) <= 255
    A, B = edge_coefficients(P, Y, r, e["eps"])
    Q = window_sum(A, r) * Y + window_sum(B, r)
    q = Q.astype(np.float64) / np.float64(n * EDGE_SHIFT * 255)
    return np.minimum(np.maximum(q, 0.0), 1.0).astype(np.float32)


def _unit(x) -> np.ndarray:
    """the egress op's fp16 chain, `(x * 0.5 + 0.5).clamp(0, 1)` with its two fp16 roundings, widened to fp32: [B,H,W,3]"""
    x = torch.from_numpy(_np16(x))
    if x.ndim == 3:
        x = x[None]
    return (x * 0.5 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().numpy()


def composite_ref(styled, source, depth, lo: float, hi: float, feather: int = 0, keep: str = "near", show: bool = False, *,
                  edge: Optional[dict] = None, backdrop=None, plane=None) -> np.ndarray:
    """L2D_OP_FRAME_MATTE on the host: fp16 [B,3,H,W] `styled` and `source` in [-1, 1] + fp16 [B,H,W] `depth` -> uint8 [B,H,W,3].
    o = v_c + m (v_s - v_c) in three fp32 operations, byte = round_half_even(255 o); `show` writes round_half_even(255 m) to all
    three channels.  Both v are multiples of 2^-24 in [0, 1], so v_s - v_c is exact: m == 1 gives the bytes of
    `egress_ref(styled)` and m == 0 those of `egress_ref(source)`, whatever the feather radius.  `edge` ({radius, eps}): the matte
    refined by `source` first (`edge_ref`).  `backdrop` (fp16 [B,3,H,W], backdrop.py): v_c is taken from it in place of
    `source`; the guide of `edge` stays the real `source`.  `plane` (fp32 [B,H,W]): a ready matte in front of the feather, in
    place of the ramp and `edge` (`matte_ref`), as `hold_ref` returns one."""
    if plane is not None:
        m = matte_ref(depth, lo, hi, feather, keep, plane=plane)[..., None]
    else:
        m = matte_ref(depth, lo, hi, feather, keep, edge=edge, source=source if edge is not None else None)[..., None]
    scale = np.float32(255.0)
    if show:
        return np.rint(np.repeat(m, 3, axis=-1) * scale).astype(np.uint8)
    vs, vc = _unit(styled), _unit(source if backdrop is None else backdrop)
    if vs.shape != vc.shape:
        raise ValueError(f"composite_ref: the styled frame is {vs.shape}, the kept part {vc.shape}")
    o = vc + m * (vs - vc)
    assert o.dtype == np.float32
    return np.rint(o * scale).astype(np.uint8)


def up_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(i0 int32 [n_out], i1 int32 [n_out], f float32 [n_out]): half-pixel bilinear sampling of one axis.  In Python floats
    s = (o + 0.5) n_in / n_out - 0.5, k = floor(s), f = float32(s - k), i0 = clamp(k, 0, n_in - 1), i1 = clamp(k + 1, 0, n_in - 1)."""
    import math
    n_in, n_out = int(n_in), int(n_out)
    i0, i1, f = np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.empty(n_out, np.float32)
    for o in range(n_out):
        s = (o + 0.5) * n_in / n_out - 0.5
        k = math.floor(s)
        f[o] = np.float32(s - k)
        i0[o], i1[o] = min(max(k, 0), n_in - 1), min(max(k + 1, 0), n_in - 1)
    return i0, i1, f


def table_words(n_in: int, n_out: int) -> np.ndarray:
    """`up_table` as the kernel reads it: int32 [3, n_out] -- i0, i1 and the bits of f"""
    i0, i1, f = up_table(n_in, n_out)
    return np.ascontiguousarray(np.stack([i0, i1, f.view(np.int32)]))


def matte_up_ref(m: np.ndarray, out_height: int, out_width: int) -> np.ndarray:
    """fp32 [B,H,W] matte of `matte_ref` (the feather already applied) -> fp32 [B,Ho,Wo]: per row a = m[x0] + fx (m[x1] - m[x0])
    on rows y0 and y1, then M = top + fy (bot - top); each subtraction, multiplication and addition rounds once.  M is exactly 1
    or 0 where its four taps are, and `m` itself bit for bit where the size does not change."""
    m = np.asarray(m, dtype=np.float32)
    if m.ndim == 2:
        m = m[None]
    x0, x1, fx = up_table(m.shape[2], out_width)
    y0, y1, fy = up_table(m.shape[1], out_height)
    fy = fy[None, :, None]

    def rows(y):
        a = m[:, y]
        left = a[:, :, x0]
        return left + fx * (a[:, :, x1] - left)

    top, bot = rows(y0), rows(y1)
    out = top + fy * (bot - top)
    assert out.dtype == np.float32
    return out


def composite_up_ref(styled_u8, camera_u8, depth, lo: float, hi: float, feather: int = 0, keep: str = "near",
                     show: bool = False, *, edge: Optional[dict] = None, source=None, backdrop=None, plane=None) -> np.ndarray:
    """L2D_OP_FRAME_MATTE_UP on the host: uint8 [B,Ho,Wo,3] `styled_u8` (the styled frame at the output size) and `camera_u8` (the
    camera's own pixels at that size) + fp16 [B,H,W] `depth` -> uint8 [B,Ho,Wo,3].  M = matte_up_ref(matte_ref(depth, ...)),
    o = C + M (S - C) on the bytes as fp32 -- S - C is exact, then one multiplication and one addition --, byte =
    round_half_even(o); `show` writes round_half_even(255 M) to all three channels.  Rounding is monotone and 0 <= M <= 1, so o
    lies between C and S and nothing is clamped (asserted); M == 1 gives S and M == 0 gives C exactly.  `edge` ({radius, eps},
    with the stream-sized fp16 [B,3,H,W] `source` frames): the matte is refined at the stream's size (`edge_ref`) and sampled
    as before.  `backdrop` (uint8 [B,Ho,Wo,3], backdrop.py): C is taken from it in place of `camera_u8`, which may then be None.
    `plane` (fp32 [B,H,W], stream-sized): a ready matte in front of the feather, in place of the ramp and `edge` (`matte_ref`),
    sampled as before."""
    def u8(x):
        x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
            raise ValueError(f"composite_up_ref: expected uint8 [B,Ho,Wo,3], got {x.dtype} {x.shape}")
        return x[None] if x.ndim == 3 else x

    S, C = u8(styled_u8), u8(camera_u8 if backdrop is None else backdrop)
    if S.shape != C.shape:
        raise ValueError(f"composite_up_ref: the styled frame is {S.shape}, the camera frame {C.shape}")
    m = (matte_ref(depth, lo, hi, feather, keep, plane=plane) if plane is not None
         else matte_ref(depth, lo, hi, feather, keep, edge=edge, source=source))
    M = matte_up_ref(m, S.shape[1], S.shape[2])[..., None]
    assert M.shape[0] == S.shape[0] and float(M.min()) >= 0.0 and float(M.max()) <= 1.0
    if show:
        return np.rint(np.repeat(M, 3, axis=-1) * np.float32(255.0)).astype(np.uint8)
    S, C = S.astype(np.float32), C.astype(np.float32)
    o = C + M * (S - C)
    assert o.dtype == np.float32 and np.all(o >= np.minimum(S, C)) and np.all(o <= np.maximum(S, C))
    return np.rint(o).astype(np.uint8)


def check_settings(lo, hi, *, keep="near", feather=0, show=False) -> dict:
    """the settings as a dict, or ValueError: lo > hi, values outside [0, 1], `feather` no integer in 0..8, `keep` not near / far"""
    for name, v in (("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"matte: {name}={v!r}: use a number in [0, 1]")
    if float(lo) > float(hi):
        raise ValueError(f"matte: lo={lo!r} is above hi={hi!r}")
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)) or not 0 <= int(feather) <= MAX_FEATHER:
        raise ValueError(f"matte: feather={feather!r}: use an integer from 0 to {MAX_FEATHER}")
    if keep not in ("near", "far"):
        raise ValueError(f"matte: keep={keep!r}: use 'near' or 'far'")
    return dict(lo=float(lo), hi=float(hi), keep=keep, feather=int(feather), show=bool(show))


# ----------------------------------------------------------------------------- matte hold
def check_hold(lo=2.0, hi=10.0, strength=0.8, radius=2, search=0, bias=256) -> dict:
    """the hold's settings as {lo, hi, strength, radius, search, bias}, or ValueError.  `lo`, `hi`, `strength` and `radius` mean
    what they mean in `steady.check_settings` (byte levels of the locally averaged source motion, a number in [0, 1], an integer
    in 0..8); `search` is an integer in 0..8 -- 0 compares the same coordinates, 1..8 follows the source's motion with
    `steady.motion_ref(search, bias)` --, `bias` an integer in 0..4096.  The defaults are steady's; nobody has tuned them on
    camera footage."""
    from . import steady
    try:
        st = steady.check_settings(lo, hi, strength, radius)
    except ValueError as e:
        raise ValueError(f"matte hold: {e}") from None
    if isinstance(search, bool) or not isinstance(search, (int, np.integer)) or not 0 <= int(search) <= steady.FOLLOW_MAX_SEARCH:
        raise ValueError(f"matte hold: search={search!r}: use an integer from 0 to {steady.FOLLOW_MAX_SEARCH} (0: the same coordinates)")
    if isinstance(bias, bool) or not isinstance(bias, (int, np.integer)) or not 0 <= int(bias) <= steady.FOLLOW_MAX_BIAS:
        raise ValueError(f"matte hold: bias={bias!r}: use an integer from 0 to {steady.FOLLOW_MAX_BIAS}")
    return dict(lo=st["lo"], hi=st["hi"], strength=st["strength"], radius=st["radius"], search=int(search), bias=int(bias))


def hold_ref(m0, source, state, *, lo: float = 2.0, hi: float = 10.0, strength: float = 0.8, radius: int = 2, search: int = 0,
             bias: int = 256, init: bool = False):
    """L2D_OP_FRAME_MATTE_HOLD (behind L2D_OP_FRAME_MOTION where `search > 0`) on the host: the fp32 [H,W] matte `m0` in front of
    the feather (`matte_ref` with feather 0, or `edge_ref`'s plane), the fp16 [3,H,W] `source` frame and the state `(prev_plane
    fp32 [H,W], prev_bytes uint8 [3,H,W])` (ignored with `init`, where it may be None) -> (h fp32 [H,W], new state, int8 field).
    b = `steady.source_bytes(source)`; with `search > 0` the field is `steady.motion_ref(b, prev_bytes, search, bias)` and P, bp
    are the state fetched along it (`steady.warp_ref`), else the state as it is and a zero field; w =
    `steady.weight_ref(b, bp, lo, hi, radius)`, a = 1 - s32 (1 - w), h = P + a (m0 - P) in three fp32 operations, then
    h = min(max(h, min(m0, P)), max(m0, P)) -- the fp32 blend may leave the interval by an ulp; with the clamp h stays in [0, 1]
    and exactly 0 or 1 where m0 and P both are --, and m0's own bits where a == 1.  The new state is (h, b), b where it is.
    With `init` h is m0 with its bits and nothing is read from a state."""
    from .steady import FOLLOW_BLOCK, motion_ref, source_bytes, warp_ref, weight_ref
    st = check_hold(lo, hi, strength, radius, search, bias)
    m0 = np.ascontiguousarray(m0.detach().cpu().numpy() if torch.is_tensor(m0) else m0)
    if m0.dtype != np.float32 or m0.ndim != 2:
        raise ValueError(f"hold_ref: expected one float32 [H,W] matte, got {m0.dtype} {m0.shape}")
    b = source_bytes(source)
    H, W = m0.shape
    if b.shape != (3, H, W):
        raise ValueError(f"hold_ref: the matte is {m0.shape}, the source frame {b.shape}")
    field = np.zeros((-(-H // FOLLOW_BLOCK), -(-W // FOLLOW_BLOCK), 2), dtype=np.int8)
    if init:
        return m0.copy(), (m0.copy(), b), field
    P, bp = state
    P, bp = np.asarray(P), np.asarray(bp)
    if P.dtype != np.float32 or P.shape != m0.shape:
        raise ValueError(f"hold_ref: the matte is {m0.shape}, the previous plane {P.dtype} {P.shape}")
    if st["search"] > 0:
        field = motion_ref(b, bp, st["search"], st["bias"])
        P, bp = warp_ref(P[None], field)[0], warp_ref(bp, field)
    w = weight_ref(b, bp, lo=st["lo"], hi=st["hi"], radius=st["radius"])
    one = np.float32(1.0)
    a = one - np.float32(st["strength"]) * (one - w)
    h = P + a * (m0 - P)                                   # numpy: three separate fp32 operations
    h = np.minimum(np.maximum(h, np.minimum(m0, P)), np.maximum(m0, P))
    h = np.ascontiguousarray(np.where(a == one, m0, h))
    assert h.dtype == np.float32 and a.dtype == np.float32
    return h, (h.copy(), b), field


# ----------------------------------------------------------------------------- the delay line
class _Slot:
    def __init__(self, height, width, device):
        self.source = torch.empty(3, height, width, dtype=torch.float16, device=device)
        self.depth = torch.empty(height, width, dtype=torch.float16, device=device)
        self.camera = None                     # the frame's own pixels at the output size (resize.CameraBuffer), or None
        self.mask = None                       # the frame's own raw mask (mask_io.MaskBuffer; a numpy array on CPU tensors), or None


class MatteLine:
    """A ring of static slots, each one source frame (fp16 [3,H,W]) and its depth plane (fp16 [H,W]), that delays them by the
    stream batch: the output of the k-th accepted frame is the frame that entered N - 1 accepted frames earlier, so `take()` for
    it returns the slot of frame k - (N - 1).

    The line is the tap of `StreamAnimateDiffusionDepth.matte_tap`: the pipeline calls it with the preprocessed frame and `dn`
    for every frame the near-duplicate filter lets through (`__call__`) and for every pushed frame (`push`, on the side stream
    and in front of the event `push` records, so `pop`'s `wait_event` covers the copies).  The copies are needed: the frame is a
    view of an ingest slot that is overwritten two frames later, `dn` a static buffer of the depth glue.  A dropped frame never
    reaches the tap and does not advance the line; the repeated output is composited with `last`, the slot of the output before.

    `prime` (called by `prepare`) clears the line and fills the N - 1 positions behind the first frame with the last warm-up
    frame and its depth.  That is a definition, not parity: the reference's first N - 1 outputs come from zeroed latent rows and
    correspond to no frame at all.  A line that starts mid-stream has no such positions: `take` then returns the oldest entry
    it has, and `last_own` is False -- the slot is another frame's, which the detail mode (detail.py) does not sharpen with.

    Slots in use: the N - 1 frames behind the newest taken one, the one taken last, and the tapped-but-not-taken frames of
    push / pop mode.  The ring grows when a caller pushes deeper than before; in steady state nothing is allocated.

    The camera frame.  While `camera_source` is set (a `resize.CameraTap`, or anything with `pending`
    and `give_back`), a slot also takes the buffer the source holds as `pending` -- the frame's own pixels at the output size,
    resampled inside `HipFrameIO.ingest` -- as `slot.camera`, and gives the slot's previous buffer back to the source's pool.
    That is a move of a reference, not a copy: the tap may run on the side stream of `push` and launches nothing there for the
    camera frame.  The rule that makes the buffers safe without events of their own: EVERY launch that writes or reads a camera
    buffer runs on the caller's stream -- the resample inside `ingest`, the composite inside the wrapper's `_finish` -- so a
    buffer that went back to the pool is overwritten only behind its last reader.  A frame that was not ingested on the device
    (a float tensor, a batch) leaves `slot.camera` None; `last` keeps its buffer as it keeps its slot.

    The mask.  While `mask_source` is set (a `mask_io.HipMaskIngest`, or anything with `pending` and
    `give_back`), a slot takes the raw mask the source holds as `pending` as `slot.mask`, exactly as it takes a camera buffer: a
    move of a reference with no launch on the side stream, the slot's previous buffer back to the pool, and the same rule --
    the copy that fills a buffer and L2D_OP_MASK_INGEST, its only reader, both run on the caller's stream.  A frame that
    brought no mask leaves `slot.mask` None and is cut by the ramp alone."""

    def __init__(self, n_steps: int, height: int, width: int, device="cpu"):
        self.n, self.height, self.width, self.device = int(n_steps), int(height), int(width), torch.device(device)
        self.slots = []
        self.camera_source = None
        self.mask_source = None
        self.clear()

    def clear(self) -> None:
        self._hist = collections.deque()       # slot ids of frames first .. first + len - 1, oldest first
        self._first = 0                        # the accepted-frame number of _hist[0] (negative: warm-up positions)
        self.tapped = 0                        # accepted frames copied in
        self.taken = 0                         # outputs composited
        self.last: Optional[_Slot] = None
        self.last_own = False                  # `last` is the slot of the output's own frame, not the oldest entry in its place
        self._last_id = None

    def _free_slot(self) -> int:
        used = set(self._hist)
        used.add(self._last_id)
        for i in range(len(self.slots)):
            if i not in used:
                return i
        self.slots.append(_Slot(self.height, self.width, self.device))
        return len(self.slots) - 1

    def _store(self, x: torch.Tensor, dn: torch.Tensor) -> int:
        i = self._free_slot()
        s = self.slots[i]
        s.source.copy_(x[-1], non_blocking=True)
        s.depth.copy_(dn[-1, 0] if dn.ndim == 4 else dn[-1], non_blocking=True)
        src, camera = self.camera_source, None
        if src is not None and src.pending is not None:
            camera, src.pending = src.pending, None
        old, s.camera = s.camera, camera
        if old is not None and src is not None:
            src.give_back(old)
        src, mask = self.mask_source, None
        if src is not None and src.pending is not None:
            mask, src.pending = src.pending, None
        old, s.mask = s.mask, mask
        if old is not None and src is not None:
            src.give_back(old)
        return i

    def drop_cameras(self) -> None:
        """forget every camera buffer (the output size or the filter changed, or the feature was turned off)"""
        for s in self.slots:
            s.camera = None

    def drop_masks(self) -> None:
        """forget every mask (the matte was turned off)"""
        for s in self.slots:
            s.mask = None

    def prime(self, x: torch.Tensor, dn: torch.Tensor) -> None:
        """`x` [F,3,H,W], `dn` [F,3,H,W]: the warm-up frames of `prepare` and their normalised depth; the last one is kept"""
        self.clear()
        if self.n > 1:
            i = self._store(x, dn)
            self._hist.extend([i] * (self.n - 1))
            self._first = -(self.n - 1)

    def __call__(self, x: torch.Tensor, dn: torch.Tensor) -> None:
        """the tap: `x` [1,3,H,W] in [-1, 1], `dn` [1,3,H,W] (or [1,H,W]) in [-1, 1]; runs on the current stream"""
        if not self._hist:
            self._first = self.tapped
        self._hist.append(self._store(x, dn))
        self.tapped += 1

    def take(self) -> _Slot:
        """the slot that belongs to the output of accepted frame number `taken`"""
        if self.taken >= self.tapped:
            raise RuntimeError("MatteLine.take: no tapped frame is waiting for its output")
        k = self.taken
        self.taken += 1
        idx = max(k - (self.n - 1), self._first) - self._first
        self.last_own = k - (self.n - 1) >= self._first
        self._last_id = self._hist[idx]
        self.last = self.slots[self._last_id]
        keep_from = self.taken - (self.n - 1)               # what the next take may still ask for
        while self._first < keep_from and len(self._hist) > 1:
            self._hist.popleft()
            self._first += 1
        return self.last


# ----------------------------------------------------------------------------- the device side
class HipMatteEdge:
    """The static fp32 plane and the launch of the edge-aware matte of one `(H, W)` stream: `op` is the record of
    L2D_OP_FRAME_MATTE_EDGE for a `MatteLine` slot, which the composites put in front of their own launch with the plane in place
    of the depth plane.  Nothing is zeroed: every launch writes the whole plane."""

    def __init__(self, height: int, width: int, device="cuda:0"):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipMatteEdge: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.plane = torch.empty(self.height, self.width, dtype=torch.float32, device=self.device)

    def op(self, slot: "_Slot", settings: dict, edge: dict, plane: Optional[torch.Tensor] = None):
        """(record, tensors to keep): `slot.source` and `slot.depth` under the matte `settings` and the `edge` setting -> `plane`;
        with `plane` (op 58's raw matte) that plane in place of the depth plane and the ramp"""
        e = check_edge(edge["radius"], edge["eps"])
        if plane is not None:
            return ops.frame_matte_edge(slot.source, None, self.plane, H=self.height, W=self.width, r=e["radius"],
                                        E=edge_E(e["radius"], e["eps"]), plane=plane)
        lo32, inv32, hard = matte_params(settings["lo"], settings["hi"])
        return ops.frame_matte_edge(slot.source, slot.depth, self.plane, H=self.height, W=self.width, r=e["radius"],
                                    E=edge_E(e["radius"], e["eps"]), lo32=lo32, inv32=inv32, hard=hard, far=settings["keep"] == "far")


class HipMatteHold:
    """The two `(plane, bytes)` records and the field of the matte hold of one `(H, W)` stream, and its launches.  The records
    ping-pong (a tile's halo and a displaced fetch read what a neighbour would write); nothing is ever zeroed: the first frame
    carries `init` and reads neither record.  `append` puts the frame's ops into the `OpList` that carries the composite -- op 55
    when `search > 0` and the frame is no init frame, then op 57 -- so a frame stays one run, with no synchronisation and no
    read-back.  `records` (two (fp32 [H,W], uint8 [3,H,W]) pairs) and `field` (int8 [ceil(H/8), W/8, 2]) may be the caller's:
    tests place them inside guarded buffers."""

    def __init__(self, height: int, width: int, device="cuda:0", records=None, field=None):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipMatteHold: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        H, W = self.height, self.width
        self.records = records if records is not None else [
            (torch.empty(H, W, dtype=torch.float32, device=self.device), torch.empty(3, H, W, dtype=torch.uint8, device=self.device))
            for _ in range(2)]
        self.field = field                  # made by the first followed frame, or the caller's
        self._cur = 0                       # the record that holds the current state

    @property
    def state(self):
        """the current `(plane, bytes)` record (device tensors; reading them synchronises)"""
        return self.records[self._cur]

    @property
    def plane(self) -> torch.Tensor:
        """the held plane of the last frame: what the composite reads under L2D_MATTE_PLANE"""
        return self.records[self._cur][0]

    def append(self, pl, slot: "_Slot", matte_settings: dict, settings: dict, plane: Optional[torch.Tensor] = None,
               init: bool = False) -> torch.Tensor:
        """append the frame's ops to `pl` and return the plane they write.  The matte input is `plane` (op 49's fp32 plane) or,
        without one, `slot.depth` under the ramp of `matte_settings`; `settings` is `check_hold`'s dict."""
        from .steady import FOLLOW_BLOCK, steady_params
        H, W = self.height, self.width
        (prev_plane, prev_bytes), (out_plane, next_bytes) = self.records[self._cur], self.records[1 - self._cur]
        lo32, inv32, hard = steady_params(settings["lo"], settings["hi"])
        kw = dict(H=H, W=W, lo32=lo32, inv32=inv32, s32=np.float32(settings["strength"]), r=settings["radius"], hard=hard, init=init)
        if plane is None:
            ramp_lo32, ramp_inv32, ramp_hard = matte_params(matte_settings["lo"], matte_settings["hi"])
            kw.update(ramp_lo32=ramp_lo32, ramp_inv32=ramp_inv32, ramp_hard=ramp_hard, far=matte_settings["keep"] == "far")
        field = None
        if settings["search"] > 0 and not init:
            if self.field is None:
                self.field = torch.empty((H + FOLLOW_BLOCK - 1) // FOLLOW_BLOCK, W // FOLLOW_BLOCK, 2, dtype=torch.int8, device=self.device)
            field = self.field
            op, keep = ops.frame_motion(slot.source, prev_bytes, field, H=H, W=W, search=settings["search"], bias=settings["bias"])
            pl.append(op, *keep)
        op, keep = ops.frame_matte_hold(slot.source, slot.depth if plane is None else None, prev_plane, prev_bytes, out_plane, next_bytes,
                                        plane=plane, field=field, **kw)
        pl.append(op, *keep)
        self._cur = 1 - self._cur
        return out_plane


class HoldStep(collections.namedtuple("HoldStep", "dev settings init repeat")):
    """the `hold=` of a composite: `dev` the stream's `HipMatteHold`, `settings` `check_hold`'s dict, `init` the frame starts the
    sequence, `repeat` the frame is a repeated output -- it is composited with the last held plane and moves nothing"""


def _front(owner, pl, slot: "_Slot", settings: dict, edge: Optional[dict], hold: Optional[HoldStep],
           raw: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """append what stands in front of a composite's own op -- the edge op, then the hold's -- and return the fp32 plane the
    composite reads in place of the depth plane, or None.  `raw` (the plane L2D_OP_MASK_INGEST wrote at the head of the list):
    the raw matte in place of the ramp -- the edge op and the hold read it, and without either the composite does."""
    if hold is not None and hold.repeat:
        return hold.dev.plane
    plane = raw
    if edge is not None:
        if owner.edge is None:
            owner.edge = HipMatteEdge(owner.height, owner.width, device=owner.device)
        op, keep = owner.edge.op(slot, settings, edge, plane=raw)
        pl.append(op, *keep)
        plane = owner.edge.plane
    if hold is not None:
        plane = hold.dev.append(pl, slot, settings, hold.settings, plane, init=hold.init)
    return plane


def _mask_head(pl, mask) -> Optional[torch.Tensor]:
    """a composite's `mask=`: None, or `(record, keep, plane)` of L2D_OP_MASK_INGEST -- appended first, in front of the
    backdrop's records, which read its plane too.  A matte key (`matte_key.HipMatteKey.record`) hands in a list of records in
    the same form: L2D_OP_MATTE_KEY (L2D_OP_MATTE_KEY_ADAPT with an adaptive plate), with a capture L2D_OP_FRAME_PLANAR_BYTES in
    front of it, and with a plate gain L2D_OP_MATTE_KEY_GAIN_HIST and L2D_OP_MATTE_KEY_GAIN between the two."""
    if mask is None:
        return None
    op, keep, plane = mask
    if isinstance(op, (list, tuple)):
        for j, one in enumerate(op):
            pl.append(one, *(keep if j == 0 else ()))
    else:
        pl.append(op, *keep)
    return plane


def _backdrop_parts(backdrop, default):
    """(tensor, records) of a composite's `backdrop=`: None (the `default` tensor), a tensor, or (tensor, [(op, keep), ...])"""
    if backdrop is None:
        return default, ()
    if torch.is_tensor(backdrop):
        return backdrop, ()
    tensor, records = backdrop
    return tensor, tuple(records)


class HipMatte:
    """Static output buffers and the launch of one `(H, W)` stream: `composite` is `HipFrameIO.egress` with a source frame and a
    depth plane beside the image.  Everything runs on `torch.cuda.current_stream()`."""

    def __init__(self, height: int, width: int, device="cuda:0"):
        if width % 8 or (height * width) % 16:
            raise ValueError(f"HipMatte: width {width} must be a multiple of 8 and height * width a multiple of 16")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.dev = torch.empty(1, self.height, self.width, 3, dtype=torch.uint8, device=self.device)
        self.host = None if ops.DRY_RUN else torch.empty(1, self.height, self.width, 3, dtype=torch.uint8).pin_memory()
        self.edge = None                       # HipMatteEdge, made by the first frame with an edge setting

    def composite(self, image: torch.Tensor, slot: _Slot, settings: dict, to_host: bool = True, edge: Optional[dict] = None,
                  backdrop=None, hold: Optional[HoldStep] = None, mask=None):
        """fp16 [3,H,W] on the device + a `MatteLine` slot -> uint8 [H,W,3]: a numpy view of the pinned buffer (valid until the next
        call), or with `to_host=False` the static device tensor.  `edge` ({radius, eps}): the matte refined by the slot's source
        frame first -- one more launch in front, and the composite reads its plane.  `backdrop` (an fp16 [3,H,W] device tensor,
        or `(tensor, records)` as `backdrop.HipBackdrop.stream` returns it): the tensor goes where `slot.source` goes in the
        composite op, the records in front of it in the same list; the edge op keeps reading the slot's real source.  `hold` (a
        `HoldStep`): the matte hold's ops behind the edge op, in the same list, and the composite reads the held plane.  `mask`
        (`(record, keep, plane)` of L2D_OP_MASK_INGEST): the record at the head of the list, its plane the raw matte."""
        H, W = self.height, self.width
        if image.dtype != torch.float16 or tuple(image.shape) != (3, H, W):
            raise ValueError(f"composite: expected fp16 [3,{H},{W}], got {image.dtype} {tuple(image.shape)}")
        if not image.is_contiguous():
            image = image.contiguous()
        kept, records = _backdrop_parts(backdrop, slot.source)
        if kept.dtype != torch.float16 or tuple(kept.shape) != (3, H, W) or not kept.is_contiguous():
            raise ValueError(f"composite: expected a contiguous fp16 [3,{H},{W}] backdrop, got {kept.dtype} {tuple(kept.shape)}")
        pl = _lib.OpList()
        raw = _mask_head(pl, mask)
        for op, keep in records:
            pl.append(op, *keep)
        plane = _front(self, pl, slot, settings, edge, hold, raw)
        if plane is not None:
            op, keep = ops.frame_matte(image, kept, None, self.dev, B=1, H=H, W=W, show=settings["show"], r=settings["feather"],
                                       plane=plane)
        else:
            lo32, inv32, hard = matte_params(settings["lo"], settings["hi"])
            op, keep = ops.frame_matte(image, kept, slot.depth, self.dev, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard,
                                       far=settings["keep"] == "far", show=settings["show"], r=settings["feather"])
        pl.append(op, *keep)
        pl.run()
        if not to_host:
            return self.dev[0]
        return to_pinned(self.dev, self.host)[0]


class HipMatteUp:
    """Device tables, static output buffers and the launch of one `(H, W) -> (Ho, Wo)` geometry: `composite` is
    `HipMatte.composite` at the output size, on the bytes `HipResize.resize` made of the styled frame and the slot's camera
    buffer.  Everything runs on `torch.cuda.current_stream()`."""

    def __init__(self, height: int, width: int, out_height: int, out_width: int, device="cuda:0"):
        from .resize import check_size
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.out_height, self.out_width = check_size(height, width, out_height, out_width)
        self.tx, self.ty = (torch.from_numpy(table_words(n_in, n_out)).to(self.device)
                            for n_in, n_out in ((self.width, self.out_width), (self.height, self.out_height)))
        self.dev = torch.empty(1, self.out_height, self.out_width, 3, dtype=torch.uint8, device=self.device)
        self.host = None if ops.DRY_RUN else torch.empty(1, self.out_height, self.out_width, 3, dtype=torch.uint8).pin_memory()
        self.edge = None                       # HipMatteEdge, made by the first frame with an edge setting

    def composite(self, styled_u8: torch.Tensor, slot: _Slot, settings: dict, to_host: bool = True, edge: Optional[dict] = None,
                  backdrop=None, hold: Optional[HoldStep] = None, mask=None):
        """uint8 [Ho,Wo,3] on the device + a `MatteLine` slot that carries a camera buffer -> uint8 [Ho,Wo,3]: a numpy view of the
        pinned buffer (valid until the next call), or with `to_host=False` the static device tensor.  `edge` ({radius, eps}): the
        matte refined at the stream's size by the slot's stream-sized source frame first, then sampled as before.  `backdrop` (a
        uint8 [Ho,Wo,3] device tensor, or `(tensor, records)` as `backdrop.HipBackdrop.output` returns it): the tensor goes where
        the slot's camera buffer goes in the composite op -- the slot then needs none --, the records in front of it.  `hold` (a
        `HoldStep`): the matte hold's ops behind the edge op; the held plane is sampled as the edge plane is.  `mask`: as
        `HipMatte.composite`'s."""
        Ho, Wo = self.out_height, self.out_width
        camera, records = _backdrop_parts(backdrop, None)
        if camera is None:
            camera = slot.camera.data
        for name, t in (("styled", styled_u8), ("camera", camera)):
            if t.dtype != torch.uint8 or tuple(t.shape) != (Ho, Wo, 3) or not t.is_contiguous():
                raise ValueError(f"composite: expected a contiguous uint8 [{Ho},{Wo},3] {name} frame, got {t.dtype} {tuple(t.shape)}")
        pl = _lib.OpList()
        raw = _mask_head(pl, mask)
        for op, keep in records:
            pl.append(op, *keep)
        plane = _front(self, pl, slot, settings, edge, hold, raw)
        if plane is not None:
            op, keep = ops.frame_matte_up(styled_u8, camera, None, self.dev, self.tx, self.ty, B=1, H=self.height, W=self.width, Ho=Ho,
                                          Wo=Wo, show=settings["show"], r=settings["feather"], plane=plane)
        else:
            lo32, inv32, hard = matte_params(settings["lo"], settings["hi"])
            op, keep = ops.frame_matte_up(styled_u8, camera, slot.depth, self.dev, self.tx, self.ty, B=1, H=self.height, W=self.width,
                                          Ho=Ho, Wo=Wo, lo32=lo32, inv32=inv32, hard=hard, far=settings["keep"] == "far",
                                          show=settings["show"], r=settings["feather"])
        pl.append(op, *keep)
        pl.run()
        if not to_host:
            return self.dev[0]
        return to_pinned(self.dev, self.host)[0]
