"""Cut detection (csrc/cut.hip): find the scene cuts on the device, so that `rewarm()` (section 8.z20) no
longer needs somebody to call it.  Every frame that enters the stream is reduced, on the BYTES a viewer would see and in exact
integers, to a signature -- the sums of its luma over 8 x 8 blocks (a thumbnail) and a 64-bin histogram of its luma -- and compared
with the signature of the frame before:  a pan moves the thumbnail and hardly moves the histogram, a flash or an exposure step
moves the histogram and the thumbnail little, a cut moves both.

  * `check_settings`, `cut_params`, `signature_ref`, `measure_ref`, `cut_ref`   the arithmetic of L2D_OP_FRAME_CUT_SIG and
                      L2D_OP_FRAME_CUT in numpy int64 -- the kernels' oracle, held to equality; no float past `cut_params`;
  * `record_dict`     an int32 [8] record as a dict;
  * `HipCutDetect`    the static buffers, the two launches and the record's asynchronous copy of one stream; on CPU tensors (the
                      host route, the mocks) the same object runs `measure_ref`.

The defaults of `check_settings` are a guess, untuned on footage.

A state is `(thumb, hist, rec)`: uint16 [H/8, W/8], uint32 [64] and the int32 [8] record {cut, Dt, Dh, since, n, E_lo, E_hi,
flags}.  E, an int64 in units of 256 Dt, is the running level of Dt over the frames that were not cuts; bit 0 of `flags` says
that there is one."""
import collections
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .matte import luma
from .steady import source_bytes

BLOCK, BINS = ops.CUT_BLOCK, ops.CUT_BINS
MAX_PIXELS = ops.CUT_MAX_PIXELS
MAX_IN_FLIGHT = 256                        # records (and pinned slots) that may wait for a `collect`
NEVER = ops.CUT_NEVER                      # `since` of a stream that has seen no cut: 2^30, where it also saturates


# ----------------------------------------------------------------------------- settings
def _number(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
        raise ValueError(f"cut detect: {name}={v!r}: use a number in [{lo}, {hi}]")
    return float(v)


def check_settings(thumb=20.0, hist=0.35, ratio=3.0, gap=8) -> dict:
    """the settings as a dict, or ValueError.  `thumb`: byte levels of mean block-luma difference, [0, 255]; `hist`: the share of
    pixels that changed bin, [0, 1]; `ratio`: the multiple of the running level a cut's Dt must reach, [1, 64], or 0: no such
    test; `gap`: frames behind a cut in which no further cut is reported, an integer in 0..255.  (Defaults: a guess, untuned.)"""
    thumb = _number("thumb", thumb, 0.0, 255.0)
    hist = _number("hist", hist, 0.0, 1.0)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) \
            or not (float(ratio) == 0.0 or 1.0 <= float(ratio) <= 64.0):
        raise ValueError(f"cut detect: ratio={ratio!r}: use 0 (no level test) or a number in [1, 64]")
    if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)) or not 0 <= int(gap) <= 255:
        raise ValueError(f"cut detect: gap={gap!r}: use an integer from 0 to 255")
    return dict(thumb=thumb, hist=hist, ratio=float(ratio), gap=int(gap))


def check_size(H: int, W: int) -> Tuple[int, int]:
    if isinstance(H, bool) or isinstance(W, bool) or int(H) != H or int(W) != W or H < BLOCK or W < BLOCK or H % BLOCK or W % BLOCK \
            or H * W > MAX_PIXELS:
        raise ValueError(f"cut detect: {H} x {W}: H and W must be positive multiples of {BLOCK} with H W <= {MAX_PIXELS}")
    return int(H), int(W)


def cut_params(H: int, W: int, settings: Optional[dict] = None) -> Tuple[int, int, int, int]:
    """(Tt, Th, R, gap), the integers the op takes, computed in Python doubles: Tt = rint(thumb 64 nb), nb the number of blocks;
    Th = rint(hist 2 H W) (a pixel that changes bin leaves one and enters one); R = rint(256 ratio)"""
    H, W = check_size(H, W)
    s = check_settings(**(settings or {}))
    nb = (H // BLOCK) * (W // BLOCK)
    return int(np.rint(s["thumb"] * 64.0 * nb)), int(np.rint(s["hist"] * 2.0 * H * W)), int(np.rint(256.0 * s["ratio"])), s["gap"]


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy)
def signature_ref(x) -> Tuple[np.ndarray, np.ndarray]:
    """the fp16 [3,H,W] (or [1,3,H,W]) frame -> (thumb uint16 [H/8,W/8], hist uint32 [64]): with Y = `matte.luma` of
    `steady.source_bytes(x)`, thumb[by,bx] = the sum of Y over the 8 x 8 block (<= 16,320), hist[k] = the pixels with Y >> 2 == k"""
    b = source_bytes(x)
    _, H, W = b.shape
    check_size(H, W)
    Y = luma(b.transpose(1, 2, 0))
    assert Y.dtype == np.int64 and int(Y.min()) >= 0 and int(Y.max()) <= 255
    thumb = Y.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK).sum(axis=(1, 3))
    hist = np.bincount((Y >> 2).reshape(-1), minlength=BINS)
    assert int(thumb.max()) <= 255 * BLOCK * BLOCK and hist.shape == (BINS,) and int(hist.sum()) == H * W
    return thumb.astype(np.uint16), hist.astype(np.uint32)


def level_of(rec) -> int:
    """E of a record: the int64 whose halves are E_lo (the low 32 bits) and E_hi"""
    r = np.asarray(rec).astype(np.int64)
    return int((r[6] << 32) | (r[5] & 0xFFFFFFFF))


def measure_ref(sig, prev_sig, prev_rec, params) -> np.ndarray:
    """L2D_OP_FRAME_CUT on the host: the signature `sig` against `prev_sig` under the previous record -> the int32 [8] record.
    `prev_sig` None: INIT, {0, 0, 0, 2^30, 0, 0, 0, 0}.  `params`: `cut_params`' (Tt, Th, R, gap).  With s = min(since' + 1, 2^30):
    cut = Dt >= Tt and Dh >= Th and s > gap and (R == 0 or no level or 65536 Dt >= R E); on a cut since = 0 and E stays; otherwise
    since = s and E = 256 Dt without a level, else E + ((256 Dt - E) >> 3), a floor shift.  Python integers throughout."""
    Tt, Th, R, gap = (int(v) for v in params)
    if prev_sig is None:
        return np.array([0, 0, 0, NEVER, 0, 0, 0, 0], dtype=np.int32)
    thumb, hist = (np.asarray(a).astype(np.int64) for a in sig)
    pthumb, phist = (np.asarray(a).astype(np.int64) for a in prev_sig)
    if thumb.shape != pthumb.shape or hist.shape != (BINS,) or phist.shape != (BINS,):
        raise ValueError(f"cut detect: signatures of {thumb.shape} / {hist.shape} against {pthumb.shape} / {phist.shape}")
    Dt, Dh = int(np.abs(thumb - pthumb).sum()), int(np.abs(hist - phist).sum())
    p = [int(v) for v in np.asarray(prev_rec).reshape(8)]
    s = min(p[3] + 1, NEVER)
    E, has = level_of(prev_rec), p[7] & 1
    cut = Dt >= Tt and Dh >= Th and s > gap and (R == 0 or not has or 65536 * Dt >= R * E)
    flags = p[7]
    if cut:
        since = 0
    else:
        since = s
        E = 256 * Dt if not has else E + ((256 * Dt - E) >> 3)             # (Python's >> on a negative integer is the floor)
        flags |= 1
    assert 0 <= E < 1 << 62 and Dt < 1 << 31
    lo = E & 0xFFFFFFFF
    return np.array([int(cut), Dt, Dh, since, p[4] + 1, lo - (1 << 32) if lo >= 1 << 31 else lo, E >> 32, flags], dtype=np.int32)


def cut_ref(frames, **settings) -> np.ndarray:
    """int32 [len(frames), 8]: the records of a sequence of fp16 [3,H,W] frames, the first one INIT"""
    recs, prev, rec, params = [], None, None, None
    for x in frames:
        sig = signature_ref(x)
        if params is None:
            params = cut_params(8 * sig[0].shape[0], 8 * sig[0].shape[1], settings)
        rec = measure_ref(sig, prev, rec, params)
        recs.append(rec)
        prev = sig
    return np.stack(recs) if recs else np.zeros((0, 8), dtype=np.int32)


def record_dict(rec) -> dict:
    """an int32 [8] record as {cut, Dt, Dh, since, n, level, has_level}: `level` is E / 256, in units of Dt"""
    r = [int(v) for v in np.asarray(rec).reshape(8)]
    return dict(cut=bool(r[0]), Dt=r[1], Dh=r[2], since=r[3], n=r[4], level=level_of(rec) / 256.0, has_level=bool(r[7] & 1))


# ----------------------------------------------------------------------------- the device side
class HipCutDetect:
    """The detector of one `(H, W)` stream: two `(thumb, hist, rec)` states the launches ping-pong between, the partials of op 65,
    and pinned host slots for the records, one per frame in flight.  `measure(x)` launches ops 65 and 66 on
    `torch.cuda.current_stream()` and one asynchronous 32-byte copy of the record behind them; nothing waits, nothing is zeroed
    (the first frame carries INIT).  `collect()` hands out the records of the frames measured so far: the CALLER states, by
    calling it, that a host synchronisation lies behind their copies.  On CPU tensors the same calls run `measure_ref`."""

    def __init__(self, height: int, width: int, settings: Optional[dict] = None, device="cuda:0"):
        self.height, self.width = check_size(height, width)
        self.device = torch.device(device)
        self.settings = check_settings(**(settings or {}))
        self.params = cut_params(self.height, self.width, self.settings)
        self.states = self.partials = None          # made by the first frame on the device
        self._host = None                           # the host route's (signature, record)
        self._slots, self._free = [], []            # pinned int32 [8] tensors; the indices not in flight
        self._flying = collections.deque()          # (slot index or the record itself, the stream's handle)
        self._cur, self.frames = 0, 0
        self.base = 0                               # for the owner: where in ITS count of frames this detector's frame 0 lies
        self._plans = {}                            # (frame address, init, state, params) -> the two-op list: built once, replayed

    def configure(self, settings: dict) -> None:
        """new thresholds from the next frame on; the state (the previous signature, the level, `since`, n) carries on"""
        self.settings = check_settings(**settings)
        self.params = cut_params(self.height, self.width, self.settings)

    def restart(self) -> None:
        """the next frame is INIT (`prepare`); records not yet collected are dropped"""
        self.frames, self._host = 0, None
        self._free.extend(e[0] for e in self._flying if isinstance(e[0], int))
        self._flying.clear()

    @property
    def in_flight(self) -> int:
        return len(self._flying)

    def _slot(self) -> int:
        if not self._free:
            self._slots.append(torch.empty(8, dtype=torch.int32).pin_memory())
            self._free.append(len(self._slots) - 1)
        return self._free.pop()

    def measure(self, x: torch.Tensor) -> int:
        """the fp16 [3,H,W] (or [1,3,H,W]) frame -> its index n since the restart; its record comes out of a later `collect()`"""
        H, W = self.height, self.width
        if not torch.is_tensor(x) or tuple(x.shape[-3:]) != (3, H, W) or x.numel() != 3 * H * W:
            raise ValueError(f"cut detect: expected a [3,{H},{W}] frame, got {ops._got(x)}")
        if len(self._flying) >= MAX_IN_FLIGHT:
            raise RuntimeError(f"cut detect: {len(self._flying)} records wait and none is collected: `collect(stream)` hands out what was "
                               "measured on that stream, so push and pop must run under the same current stream")
        init = self.frames == 0
        if not x.is_cuda:
            sig = signature_ref(x)
            rec = measure_ref(sig, None if init else self._host[0], None if init else self._host[1], self.params)
            self._host = (sig, rec)
            self._flying.append((rec, 0))
        else:
            if x.dtype != torch.float16:
                raise ValueError(f"cut detect: expected an fp16 frame on the device, got {x.dtype}")
            x = x if x.is_contiguous() else x.contiguous()
            if self.states is None:
                nwg = ops.frame_cut_tiles(H, W)
                self.states = [(torch.empty(H // BLOCK, W // BLOCK, dtype=torch.uint16, device=self.device),
                                torch.empty(BINS, dtype=torch.uint32, device=self.device),
                                torch.empty(8, dtype=torch.int32, device=self.device)) for _ in range(2)]
                self.partials = torch.empty(nwg, ops.CUT_PARTIAL, dtype=torch.uint32, device=self.device)
            prev, nxt = self.states[self._cur], self.states[1 - self._cur]
            if x.data_ptr() % 16:
                raise ValueError("cut detect: the frame is not 16-byte aligned")
            key = (x.data_ptr(), init, self._cur, self.params)
            pl = self._plans.get(key)
            if pl is None:                          # (frames come from a few static slots: the builders' checks run once per slot)
                if len(self._plans) >= 16:
                    self._plans.clear()
                pl = self._plans[key] = _lib.OpList()
                op, keep = ops.frame_cut_sig(x, None if init else prev[0], nxt[0], self.partials, H=H, W=W)
                pl.append(op, *(t for t in keep if t is not x))       # (the list holds the frame's address, not the frame)
                Tt, Th, R, gap = self.params
                op, keep = ops.frame_cut(self.partials, None if init else prev, nxt, H=H, W=W, Tt=Tt, Th=Th, R=R, gap=gap)
                pl.append(op, *keep)
            pl.run()
            self._cur = 1 - self._cur
            j = self._slot()
            self._slots[j].copy_(nxt[2], non_blocking=True)
            self._flying.append((j, int(torch.cuda.current_stream().cuda_stream)))
        self.frames += 1
        return self.frames - 1

    def collect(self, stream=None) -> list:
        """the int32 [8] records (numpy, oldest first) of the frames measured since the last call -- `stream`: only those measured
        on that stream (its `synchronize()` lies behind the caller; `pop`'s), None: all (a device-wide `synchronize()` does).
        Records of the host route are complete as they are.  A record measured under another stream than the one named here is
        never handed out: `push` and `pop` must run under the same current stream (`measure` raises once MAX_IN_FLIGHT wait)."""
        handle = None if stream is None else int(stream.cuda_stream)
        out, rest = [], collections.deque()
        for item, s in self._flying:
            if not isinstance(item, int):
                out.append(item)
            elif handle is None or s == handle:
                out.append(self._slots[item].numpy().copy())
                self._free.append(item)
            else:
                rest.append((item, s))
        self._flying = rest
        return out
