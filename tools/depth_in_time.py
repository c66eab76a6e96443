"""Timing of the depth input (csrc/depth_in.hip, live2diff_amd/depth_io.py) on the MI355X.

    timeout -k 10 300 python tools/depth_in_time.py --out profiles/depth_in_time.txt

What a frame with `depth=` pays for its conditioning map -- L2D_OP_DEPTH_INGEST + L2D_OP_DEPTH_NORMALIZE -- beside the detector
path it replaces, exactly as `encode_depth` calls it (`HipDepthGlue.resize` to 384 x 384, `HipMidas` with random weights of the
real DPT-Hybrid geometry, `HipDepthGlue.normalize_resize` back to 512 x 512), from the same process: device events around
`--reps` back-to-back runs after a warm-up (microseconds per run), `--rounds` rounds with the variants alternating inside each
round, so that a drift of the box shows in every variant alike.  The figure of a variant is the median over the rounds; the
spread is given.  Depth frames: uint16 1280 x 720 and 640 x 480, each -> 512 x 512."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def timed_us(fn, reps):
    """device events around `reps` back-to-back calls of `fn`: microseconds per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib
    from live2diff_amd.depth_io import HipDepthIngest
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.vae_hip import HipDepthGlue
    dev, H, W = "cuda", args.size, args.size
    g = np.random.default_rng(0)
    midas = HipMidas(random_midas_state_dict(device=dev), device=dev)
    glue = HipDepthGlue(torch.device(dev))
    x = (torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(0)) * 0.5).clamp(-1, 1).half().to(dev)

    def detector():
        return glue.normalize_resize(midas(glue.resize(x, 384, 384)).to(torch.float16), H, W)

    say(args.out, f"# depth_in_time: {_lib.device_name()}, -> {H}x{W}, {args.reps} back-to-back runs per figure (device events), "
                  f"{args.rounds} rounds, the variants alternating inside a round; median (min .. max) microseconds per run")
    for Hd, Wd in ((720, 1280), (480, 640)):
        z = g.integers(300, 6000, (Hd, Wd)).astype(np.uint16)
        z[g.random((Hd, Wd)) < 0.03] = 0
        zdev = torch.from_numpy(z.view(np.int16)).to(dev)           # (int16: the bits of the uint16 samples)
        ing = HipDepthIngest(H, W, device=dev)
        for _ in range(4):
            ing.ingest(zdev)                                       # (both slots keep their plan for this pointer)
        plans = list(ing._device_plans.values())
        fixed = HipDepthIngest(H, W, device=dev)
        variants = [("the detector path (resize, HipMidas, normalize_resize)", detector),
                    ("ops 52 + 53, device frame read in place", lambda: ing.ingest(zdev)),
                    ("ops 52 + 53, fixed range", lambda: fixed.ingest(zdev, range=(300.0, 6000.0))),
                    ("host frame: staging copy, upload, ops 52 + 53", lambda: ing.ingest(z))]
        lists = []
        for name, fn in variants:
            timed_us(fn, 10)
            lists.append((name, fn, []))
        for _ in range(args.rounds):
            for _, fn, us in lists:
                us.append(timed_us(fn, args.reps))
        say(args.out, f"uint16 {Wd}x{Hd} -> {H}x{W}")
        med = {}
        for name, _, us in lists:
            med[name] = statistics.median(us)
            say(args.out, f"  {name:56s}: {med[name]:9.2f} us ({min(us):.2f} .. {max(us):.2f})")
        each = [round(u, 2) for u in plans[0].time_each_us(args.reps)]
        say(args.out, f"  in sequence, launch by launch (ingest, normalize): {each} us")
        say(args.out, f"  detector path / ops 52 + 53 = {med[variants[0][0]] / med[variants[1][0]]:.1f}")


if __name__ == "__main__":
    main()
