"""Depth from the caller (csrc/depth_in.hip): a depth frame of an RGB-D camera, or of an estimator in the
caller's own process, in place of the built-in detector's -- uint16 or float32, of any size, on the host or on the device ->
the stream's conditioning map `dn`, fp16 [B,3,H,W] in [-1, 1] (larger = nearer), what `encode_depth` normalises the detector's
output to.  The reference has no counterpart.

`depth_ref` (numpy) states the arithmetic: every product, sum and quotient rounded to fp32 on its own, no fma, one rounding to
fp16 at the end.  It is the oracle of the two kernels, bit for bit, and what the pipeline computes on CPU tensors.
`HipDepthIngest` owns the static buffers and the kept plans of one stream.

One rule beyond validity by value: a sample counts only if its `u` is finite and not negative.  For `kind="distance"` that is
`z > 0` (and 1 / z not overflowing); for `kind="inverse"` it excludes negative inverse depths, which mean nothing and would
collide with the negative "no value" mark of the resampled plane.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .frame_io import MAX_SCALE, aa_weights, geometry

KINDS = ("distance", "inverse")
DEFAULTS = dict(kind="distance", invalid=0, range=None)
FLAT = np.float32(2.0 ** -14)        # range=None: a map whose own range mx - mn is at or below FLAT mx is flat, all -1 (normalize_ref)
NO_VALUE = np.float32(-1.0)          # the mark of a pixel without a value in the resampled plane (u >= 0 wherever it is valid)


# ----------------------------------------------------------------------------- settings
def check_settings(kind="distance", invalid=0, range=None) -> dict:
    """{kind, invalid, range} validated; ValueError names the keyword"""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: use 'distance' (metric, larger = farther) or 'inverse' (larger = nearer)")
    if invalid is not None:
        if isinstance(invalid, bool) or not isinstance(invalid, (int, float, np.integer, np.floating)) or not np.isfinite(invalid):
            raise ValueError(f"invalid={invalid!r}: use a finite number (the sample value that marks a hole) or None")
        invalid = float(invalid) if float(invalid) != int(invalid) else int(invalid)
    if range is not None:
        try:
            a, b = (float(v) for v in range)
        except (TypeError, ValueError):
            raise ValueError(f"range={range!r}: use (near, far) for 'distance', (lo, hi) for 'inverse', or None") from None
        if np.isnan(a) or np.isnan(b):
            raise ValueError(f"range={range!r}: not a number")
        if kind == "distance":
            if not (0.0 < a < b) or np.isinf(a):
                raise ValueError(f"range={range!r}: 'distance' needs 0 < near < far (far may be inf)")
        elif not (0.0 <= a < b) or np.isinf(b):
            raise ValueError(f"range={range!r}: 'inverse' needs 0 <= lo < hi, both finite")
        range = (a, b)
    return dict(kind=kind, invalid=invalid, range=range)


def fixed_range(kind: str, range) -> Optional[Tuple[np.float32, np.float32]]:
    """(mn, mx) in units of u as float32, or None: 'distance' (near, far) -> (1 / far, 1 / near), one correctly rounded fp32
    division each (far = inf gives 0); 'inverse' (lo, hi) as they are"""
    if range is None:
        return None
    a, b = np.float32(range[0]), np.float32(range[1])
    if kind == "distance":
        return np.float32(1.0) / b, np.float32(1.0) / a
    return a, b


# ----------------------------------------------------------------------------- geometry and tables
def tables(Hd: int, Wd: int, H: int, W: int):
    """((nh, nw, top, left), ymin int32 [H], wy fp32 [H,Ky], xmin int32 [W], wx fp32 [W,Kx]): `frame_io.geometry` of the depth
    frame's own size and rows [top, top + H) / [left, left + W) of `frame_io.aa_weights` in fp32 -- what the host uploads and the
    oracle reads.  A tap past a row's own count has weight 0."""
    try:
        geo = geometry(Hd, Wd, H, W)
    except ValueError as e:
        raise ValueError(f"depth: {e}") from None
    nh, nw, top, left = geo
    if Hd / nh > MAX_SCALE or Wd / nw > MAX_SCALE:
        raise ValueError(f"depth: frame geometry {Hd}x{Wd} -> {H}x{W}: down-scale above {MAX_SCALE:g}")
    ymin, wy = aa_weights(Hd, nh, torch.float32)
    xmin, wx = aa_weights(Wd, nw, torch.float32)
    ymin, wy = ymin[top:top + H], wy[top:top + H]
    xmin, wx = xmin[left:left + W], wx[left:left + W]
    if wy.shape[1] > ops.DEPTH_MAX_TAPS or wx.shape[1] > ops.DEPTH_MAX_TAPS:
        raise ValueError(f"depth: frame geometry {Hd}x{Wd} -> {H}x{W}: more than {ops.DEPTH_MAX_TAPS} taps per axis")
    return (geo, ymin.to(torch.int32).contiguous(), wy.contiguous(), xmin.to(torch.int32).contiguous(), wx.contiguous())


def _as_frames(depth) -> np.ndarray:
    """[Hd,Wd] or [B,Hd,Wd], numpy or torch, -> a contiguous uint16 or float32 [B,Hd,Wd] array (fp16 and uint8 widened exactly)"""
    if torch.is_tensor(depth):
        depth = depth.detach().cpu()
        # (a torch int16 tensor holds the bits of uint16 samples, on the host as on the device: not every torch build copies uint16)
        depth = depth.view(torch.int16).numpy().view(np.uint16) if depth.dtype in (torch.uint16, torch.int16) else depth.numpy()
    z = np.asarray(depth)
    if z.dtype == np.float16:
        z = z.astype(np.float32)
    elif z.dtype == np.uint8:
        z = z.astype(np.uint16)
    if z.dtype not in (np.uint16, np.float32):
        raise ValueError(f"depth: expected uint16 or float32 samples (uint8 and float16 are widened), got {z.dtype}")
    if z.ndim == 2:
        z = z[None]
    if z.ndim != 3 or 0 in z.shape:
        raise ValueError(f"depth: expected [Hd,Wd] or [B,Hd,Wd], got {tuple(z.shape)}")
    return np.ascontiguousarray(z)


# ----------------------------------------------------------------------------- the oracle (numpy)
def convert_ref(z: np.ndarray, kind: str, invalid):
    """(u, v) float32 of uint16 / float32 samples: v = 1 where the sample is valid, u its inverse depth there and 0 elsewhere"""
    zf = z.astype(np.float32)
    if z.dtype == np.uint16:
        ok = np.ones(z.shape, bool) if invalid is None else z != invalid
    else:
        ok = np.isfinite(zf)
        if invalid is not None:
            ok &= zf != np.float32(invalid)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = np.float32(1.0) / zf if kind == "distance" else zf
        ok = ok & np.isfinite(u) & (u >= 0)
    return np.where(ok, u, np.float32(0.0)).astype(np.float32), ok.astype(np.float32)


def _taps(a: np.ndarray, lo: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    """sum_j w[:, j] * a[lo + j] along `axis`, taps ascending, every product and sum rounded to fp32"""
    n_in = a.shape[axis]
    a = np.moveaxis(a, axis, -1)
    acc = np.zeros(a.shape[:-1] + (lo.shape[0],), np.float32)
    for j in range(w.shape[1]):
        idx = np.minimum(lo + j, n_in - 1)                     # (a tap past the row's own count has weight 0)
        acc = acc + w[:, j] * a[..., idx]
    return np.moveaxis(acc, -1, axis)


def resample_ref(depth, H: int, W: int, kind="distance", invalid=0) -> np.ndarray:
    """R, float32 [B,H,W]: num / den of the normalised convolution where den > 0, NO_VALUE elsewhere (op 52's plane)"""
    z = _as_frames(depth)
    _, ymin, wy, xmin, wx = tables(z.shape[1], z.shape[2], H, W)
    ymin, wy, xmin, wx = ymin.numpy().astype(np.int64), wy.numpy(), xmin.numpy().astype(np.int64), wx.numpy()
    u, v = convert_ref(z, kind, invalid)
    num = _taps(_taps(u, xmin, wx, 2), ymin, wy, 1)
    den = _taps(_taps(v, xmin, wx, 2), ymin, wy, 1)
    has = den > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(has, num / np.where(has, den, np.float32(1.0)), NO_VALUE).astype(np.float32)


def partials_ref(R: np.ndarray) -> np.ndarray:
    """float32 [B tiles, 3]: {min, max, any} of R over the valued pixels of every tile ({+inf, -1, 0} where there is none)"""
    B, H, W = R.shape
    th, tw = ops.DEPTH_TILE_H, ops.DEPTH_TILE_W
    out = []
    for b in range(B):
        for y in range(0, H, th):
            for x in range(0, W, tw):
                t = R[b, y:y + th, x:x + tw]
                t = t[t >= 0]
                out.append((t.min(), t.max(), 1.0) if t.size else (np.inf, -1.0, 0.0))
    return np.asarray(out, np.float32)


def normalize_ref(R: np.ndarray, fixed=None) -> np.ndarray:
    """fp16 [B,3,H,W]: n = clamp((R - mn) / (mx - mn), 0, 1), dn = fp16(2 n - 1) (op 53).  mn, mx: `fixed` (float32, units of
    u) or the min and max of R over the valued pixels of all B frames; -1 for a pixel without a value, and everywhere where
    the map is flat.  With a fixed range that is mx <= mn: a caller's range, however narrow, is taken at its word.  With the
    frames' own range it is nothing valued, or fl(mx - mn) <= fl(FLAT mx): that holds mx <= mn, and the rounding noise of the
    resampling -- num and den of a constant frame are 2 x 34 products and sums each, so R moves from pixel to pixel by up to
    2 x (2 x 2 x 34 + 1) x 2^-24 < 2^-15.9 of its value, and stretching that to [-1, 1] would condition the stream on noise."""
    has = R >= 0
    n = np.zeros(R.shape, np.float32)
    if fixed is not None:
        mn, mx = np.float32(fixed[0]), np.float32(fixed[1])
        ok = mx > mn
    elif has.any():
        mn, mx = R[has].min(), R[has].max()
        ok = mx - mn > mx * FLAT
    else:
        ok = False
    if ok:
        with np.errstate(invalid="ignore", over="ignore"):
            q = (R - mn) / (mx - mn)
        n = np.where(has, np.minimum(np.maximum(q, np.float32(0.0)), np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    dn = (np.float32(2.0) * n - np.float32(1.0)).astype(np.float16)
    return np.ascontiguousarray(np.broadcast_to(dn[:, None], (R.shape[0], 3) + R.shape[1:]))


def depth_ref(depth, H: int, W: int, kind="distance", invalid=0, range=None) -> np.ndarray:
    """A depth frame [Hd,Wd] or batch [B,Hd,Wd] (uint16 or float32; fp16 and uint8 widened exactly) -> fp16 [B,3,H,W] in [-1, 1],
    the three channels equal: what `encode_depth` calls `dn`.

    Per sample z: valid when (uint16) z != invalid or (floats) z finite and != invalid (`invalid=None`: every value counts), and
    u finite and not negative; u = float(z) for kind="inverse" (MiDaS's convention, larger = nearer), 1 / float(z) for
    kind="distance".  Per output pixel, over `frame_io.geometry(Hd, Wd, H, W)` -- the same relative centred window the colour
    ingest looks at -- with the fp32 weights of `frame_io.aa_weights`: num = sum_y wy (sum_x wx v u), den = sum_y wy (sum_x wx
    v), R = num / den where den > 0; holes smaller than the filter's footprint are filled by their valid neighbours, larger ones
    have no value.  range=None: mn, mx = min, max of R over the valued pixels of all B frames jointly, taken after resampling (one
    flying pixel does not set the range); range=(near, far) for "distance" (mx = 1 / near, mn = 1 / far) or (lo, hi) for
    "inverse", in input units.  dn = fp16(2 clamp((R - mn) / (mx - mn), 0, 1) - 1); -1, the farthest, for a pixel without a value
    and for the whole map where it is flat: mx <= mn, or with range=None nothing valued or a range within FLAT = 2^-14 of mx
    (`normalize_ref`)."""
    s = check_settings(kind, invalid, range)
    R = resample_ref(depth, H, W, s["kind"], s["invalid"])
    return normalize_ref(R, fixed_range(s["kind"], s["range"]))


# ----------------------------------------------------------------------------- the device side
def _torch_frames(depth) -> torch.Tensor:
    """a depth frame or batch as a contiguous int16 (the bits of the uint16 samples: every torch build copies that dtype) or
    float32 [B,Hd,Wd] torch tensor; a device tensor stays where it is"""
    if torch.is_tensor(depth) and depth.is_cuda:
        z = depth
        if z.dtype == torch.float16:
            z = z.float()
        elif z.dtype == torch.uint8:
            z = z.to(torch.int16)
        elif z.dtype == torch.uint16:
            z = z.view(torch.int16)
        if z.dtype not in (torch.int16, torch.float32):              # (int16: the bits of uint16 samples)
            raise ValueError(f"depth: expected uint16 or float32 samples (uint8 and float16 are widened), got {depth.dtype}")
        if z.ndim == 2:
            z = z[None]
        if z.ndim != 3 or 0 in z.shape:
            raise ValueError(f"depth: expected [Hd,Wd] or [B,Hd,Wd], got {tuple(z.shape)}")
        return z if z.is_contiguous() else z.contiguous()
    z = _as_frames(depth)
    return torch.from_numpy(z.view(np.int16) if z.dtype == np.uint16 else z)


class _Slot:
    def __init__(self, Hd, Wd, H, W, device):
        nbytes = Hd * Wd * 4                                    # room for either dtype
        self.staging = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.dev_raw = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.R = torch.empty(1, H, W, dtype=torch.float32, device=device)
        self.partials = torch.empty(ops.depth_tiles(H, W), 3, dtype=torch.float32, device=device)
        self.out = torch.empty(1, 3, H, W, dtype=torch.float16, device=device)
        self.uploaded: Optional[torch.cuda.Event] = None    # behind the last H2D copy out of `staging`
        self.released = None                                # the caller's event behind the last reader of `out` (release())
        self.plans = {}                                     # (dtype, settings) -> plan: dev_raw -> out

    def views(self, dtype, Hd, Wd):
        n = Hd * Wd * (4 if dtype == torch.float32 else 2)
        return self.staging[:n].view(dtype).view(Hd, Wd), self.dev_raw[:n].view(dtype).view(1, Hd, Wd)


class HipDepthIngest:
    """Static buffers and plans for one `(Hd, Wd) -> (H, W)` depth stream.  Everything runs on `torch.cuda.current_stream()`.

    A single frame lands in one of TWO slots used in turn -- a pinned staging buffer, the device raw frame, R, the partials and
    the fp16 map; the returned tensor is a view of the slot, valid until the ingest after the next.  A consumer on another stream
    hands the event behind its last read to `release(view, event)` (the pipeline needs none: the tap and the VAE encode read the
    map on the stream the ingest ran on, in `__call__` and on `push`'s side stream alike).  A caller's device tensor is read in
    place, with no copy.  What that retains: a plan holds its source tensor, so a source pointer is kept only from its second
    meeting on -- a producer with static output buffers --, at most four plans (two sources x two slots), all dropped when a
    fifth comes or the geometry changes; a tensor met once, and a widened or re-packed copy of the caller's (`.float()`,
    `.contiguous()`), is held for its one run only.  A batch (B > 1) gets fresh tensors and is normalised jointly."""

    def __init__(self, height: int, width: int, device="cuda:0"):
        if (height * width) % 8:
            raise ValueError(f"HipDepthIngest: height * width = {height * width} must be a multiple of 8")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self._src = None                   # (Hd, Wd) the slots are planned for
        self._geo = self._tables = None
        self._slots = []
        self._turn = 0
        self.last_view = None
        self._device_plans = {}            # (source pointer, slot, dtype, settings) -> plan
        self._device_seen = ()             # the last four source pointers of device frames (integers: nothing is kept alive)
        self.plans_built = 0               # plans made so far (a kept plan is not made again)

    def _plan_source(self, Hd: int, Wd: int):
        geo, ymin, wy, xmin, wx = tables(Hd, Wd, self.height, self.width)
        self._geo = geo
        self._tables = tuple(t.to(self.device) for t in (xmin, wx, ymin, wy))
        self._src = (Hd, Wd)
        self._slots = [_Slot(Hd, Wd, self.height, self.width, self.device) for _ in range(2)]
        self._turn = 0
        self._device_plans.clear()

    def _plan(self, src, R, partials, out, B, s):
        (Hd, Wd), (nh, nw, top, left) = self._src, self._geo
        H, W = self.height, self.width
        pl = _lib.OpList()
        op, keep = ops.depth_ingest(src, R, partials, *self._tables, B=B, Hd=Hd, Wd=Wd, H=H, W=W, nh=nh, nw=nw, top=top, left=left,
                                    distance=s["kind"] == "distance", invalid=s["invalid"])
        pl.append(op, *keep)
        op, keep = ops.depth_normalize(R, partials, out, B=B, H=H, W=W, fixed=fixed_range(s["kind"], s["range"]))
        pl.append(op, *keep)
        self.plans_built += 1
        return pl

    def ingest(self, depth, kind="distance", invalid=0, range=None) -> torch.Tensor:
        """uint16 / float32 [Hd,Wd] or [B,Hd,Wd], on the host or already on the device -> fp16 [B,3,H,W] in [-1, 1]"""
        s = check_settings(kind, invalid, range)
        z = _torch_frames(depth)
        B, Hd, Wd = z.shape
        if self._src != (Hd, Wd):
            self._plan_source(Hd, Wd)
        H, W = self.height, self.width
        if B > 1:
            src = z if z.is_cuda else z.to(self.device, non_blocking=True)
            R = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
            partials = torch.empty(B * ops.depth_tiles(H, W), 3, dtype=torch.float32, device=self.device)
            out = torch.empty(B, 3, H, W, dtype=torch.float16, device=self.device)
            self._plan(src, R, partials, out, B, s).run()
            return out
        idx = self._turn
        slot = self._slots[idx]
        self._turn ^= 1
        cur = torch.cuda.current_stream()
        if slot.released is not None:
            cur.wait_event(slot.released)
            slot.released = None
        skey = (z.dtype, s["kind"], s["invalid"], s["range"])
        if z.is_cuda:
            # a caller's device frame, read in place (a kept plan keeps its source alive, so its pointer cannot become another
            # tensor's; a pointer seen for the first time, or a copy made here, fills two records and is let go)
            ptr = z.data_ptr()
            key = (ptr, idx) + skey
            plan = self._device_plans.get(key)
            if plan is None:
                plan = self._plan(z, slot.R, slot.partials, slot.out, 1, s)
                if ptr in self._device_seen and ptr == depth.data_ptr():
                    if len(self._device_plans) >= 4:
                        self._device_plans.clear()
                    self._device_plans[key] = plan
                self._device_seen = (self._device_seen + (ptr,))[-4:]
        else:
            host, dev = slot.views(z.dtype, Hd, Wd)
            if slot.uploaded is not None:
                slot.uploaded.synchronize()          # the copy out of this staging buffer two frames ago (long done)
            host.copy_(z[0])
            dev[0].copy_(host, non_blocking=True)
            slot.uploaded = slot.uploaded or torch.cuda.Event()
            slot.uploaded.record(cur)
            plan = slot.plans.get(skey)
            if plan is None:
                if len(slot.plans) >= 4:
                    slot.plans.clear()
                plan = slot.plans[skey] = self._plan(dev, slot.R, slot.partials, slot.out, 1, s)
        plan.run()
        self.last_view = slot.out
        return slot.out

    def release(self, slot_view: torch.Tensor, event) -> None:
        """`event` was recorded behind the last read of `slot_view` (a tensor `ingest` returned) on another stream"""
        for slot in self._slots:
            if slot.out.data_ptr() == slot_view.data_ptr():
                slot.released = event
                return
        raise ValueError("release: not a view of an ingest slot")
