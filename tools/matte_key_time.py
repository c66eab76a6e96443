"""Timing of the matte key (csrc/matte_key.hip, live2diff_amd/matte_key.py) on the MI355X.

    timeout -k 10 120 python tools/matte_key_time.py --out profiles/matte_key_time.txt

L2D_OP_MATTE_KEY at 512x512 in both variants (a colour key and a plate key; radius 0, 1 and 4; "replace", and "and" at radius 1)
and L2D_OP_FRAME_PLANAR_BYTES, beside L2D_OP_FRAME_MATTE_HOLD (radius 2, from the depth plane) -- the op whose tile form op 59
takes -- in the same run: device events around `--reps` back-to-back replays after a warm-up, the median of five runs
(microseconds per launch).  `tools/mask_time.py kernels` on the same box gives op 58's figures.  L2D_OP_MATTE_KEY_ADAPT (the adaptive plate, section 8.z18)
follows in the same run, INIT and STATE at the same radii: its yardstick is op 59 with a plate.  The plate gain (section 8.z19)
follows both: L2D_OP_MATTE_KEY_GAIN_HIST against the plate and against the state -- on the noise frame, whose ratios spread over
the bins, and on the plate's own frame, where every valid sample lands in bin 128 (a still room: the worst case of the LDS
atomics) --, L2D_OP_MATTE_KEY_GAIN, and ops 59 / 61 under L2D_MATTE_KEY_GAIN beside their unflagged rows above."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mask_time import _timed  # noqa: E402
from steady_time import say  # noqa: E402


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import matte_params
    from live2diff_amd.backdrop import frame_of
    from live2diff_amd.matte_key import adapt_params, gain_params, key_params, luma_weight, state_of
    from live2diff_amd.steady import steady_params
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# matte_key_time: {_lib.device_name()}, {args.reps} back-to-back replays per figure (device events), median of 5 runs, "
                  f"{W}x{H}")
    g = torch.Generator().manual_seed(0)
    src = (torch.randn(3, H, W, generator=g) * 0.6).half().to(dev)
    depth = (torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    plate = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
    plane = torch.empty(H, W, dtype=torch.float32, device=dev)
    lo2, inv, hard = key_params(40, 90)
    lo32, inv32, ramp_hard = matte_params(0.3, 0.7)
    kw = dict(H=H, W=W, L=luma_weight(0.25), lo2=lo2, inv=inv, hard=hard)
    med = {}
    for name, key in (("colour", (0, 177, 64)), ("plate", plate)):
        for r in (0, 1, 4):
            med[name, r] = _timed(args.out, args.reps, f"op 59 matte key, {name}, r = {r}, replace", ops.matte_key(src, plane, None, key, r=r, **kw))
        _timed(args.out, args.reps, f"op 59 matte key, {name}, r = 1, and",
               ops.matte_key(src, plane, depth, key, r=1, combine="and", lo32=lo32, inv32=inv32, ramp_hard=ramp_hard, **kw))
    # the adaptive plate: the state read is the plate's own, the state written another record (they ping-pong)
    state = torch.from_numpy(state_of(plate.cpu().numpy()).view(np.int16)).to(dev)
    nxt = torch.empty_like(state)
    a_bg, a_fg = adapt_params(1 / 32, 0.0)
    for name, pl, st in (("init", plate, None), ("state", None, state)):
        for r in (0, 1, 4):
            med[name, r] = _timed(args.out, args.reps, f"op 61 matte key adapt, {name}, r = {r}, replace",
                                  ops.matte_key_adapt(src, plane, None, pl, st, nxt, r=r, a_bg=a_bg, a_fg=a_fg, **kw))
        _timed(args.out, args.reps, f"op 61 matte key adapt, {name}, r = 1, and",
               ops.matte_key_adapt(src, plane, depth, pl, st, nxt, r=1, a_bg=a_bg, a_fg=a_fg, combine="and", lo32=lo32, inv32=inv32,
                                   ramp_hard=ramp_hard, **kw))
    say(args.out, "op 61 against op 59 with a plate: " + ", ".join(
        f"{name} r = {r} {med[name, r] / med['plate', r]:.2f} x" for name in ("init", "state") for r in (0, 1, 4)))
    # the plate gain: the samples, the medians, and the key's launches reading the record
    still = torch.from_numpy(np.array(frame_of(plate.cpu().numpy()))).to(dev)
    partials = torch.empty(ops.matte_key_gain_blocks(H, W), 3, ops.MATTE_KEY_GAIN_BINS, dtype=torch.int32, device=dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    lim, min_count = gain_params(2.0, 1 / 16, H, W)
    for name, key in (("plate", plate), ("state", state)):
        _timed(args.out, args.reps, f"op 62 matte key gain hist, {name}, noise frame", ops.matte_key_gain_hist(src, key, partials, H=H, W=W))
        _timed(args.out, args.reps, f"op 62 matte key gain hist, {name}, the plate's own frame",
               ops.matte_key_gain_hist(still, key, partials, H=H, W=W))
    _timed(args.out, args.reps, f"op 63 matte key gain, {partials.shape[0]} partials",
           ops.matte_key_gain(partials, record, H=H, W=W, lim=lim, min_count=min_count))
    for r in (0, 1, 4):
        med["gain plate", r] = _timed(args.out, args.reps, f"op 59 matte key, plate, gain, r = {r}, replace",
                                      ops.matte_key(src, plane, None, plate, r=r, gain=record, **kw))
    for name, pl, st in (("init", plate, None), ("state", None, state)):
        for r in (0, 1, 4):
            med["gain " + name, r] = _timed(args.out, args.reps, f"op 61 matte key adapt, {name}, gain, r = {r}, replace",
                                            ops.matte_key_adapt(src, plane, None, pl, st, nxt, r=r, a_bg=a_bg, a_fg=a_fg, gain=record, **kw))
    say(args.out, "under L2D_MATTE_KEY_GAIN against the unflagged launch: " + ", ".join(
        f"{name} r = {r} {med['gain ' + name, r] / med[name, r]:.2f} x" for name in ("plate", "init", "state") for r in (0, 1, 4)))
    bytes_ = torch.empty(3, H, W, dtype=torch.uint8, device=dev)
    _timed(args.out, args.reps, "op 60 frame planar bytes (the plate capture)", ops.frame_planar_bytes(src, bytes_, H=H, W=W))
    # the tile form's owner, in the same run: op 57 from the depth plane, radius 2, a steady state frame
    rec = [(torch.zeros(H, W, device=dev), torch.zeros(3, H, W, dtype=torch.uint8, device=dev)) for _ in range(2)]
    slo, sinv, shard = steady_params(2.0, 10.0)
    base = _timed(args.out, args.reps, "op 57 matte hold, r = 2, depth plane",
                  ops.frame_matte_hold(src, depth, rec[0][0], rec[0][1], rec[1][0], rec[1][1], H=H, W=W, lo32=slo, inv32=sinv,
                                       s32=0.8, r=2, hard=shard, init=False, ramp_lo32=lo32, ramp_inv32=inv32, ramp_hard=ramp_hard, far=False))
    say(args.out, f"op 59 against op 57: colour r = 1 {med['colour', 1] / base:.2f} x, plate r = 1 {med['plate', 1] / base:.2f} x, "
                  f"plate r = 4 {med['plate', 4] / base:.2f} x")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    kernels(args)


if __name__ == "__main__":
    main()
