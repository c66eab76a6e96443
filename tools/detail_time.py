"""Timing of the detail mode (csrc/detail.hip, live2diff_amd/detail.py) on the MI355X.

    timeout -k 10 180 python tools/detail_time.py --out profiles/detail_time.txt

The three launches a frame with detail pays for behind its resize -- L2D_OP_FRAME_DETAIL_GAIN, the source frame's
L2D_OP_FRAME_RESIZE and L2D_OP_FRAME_DETAIL -- in sequence (the plan `HipDetail` runs), each one alone, and the plain
L2D_OP_FRAME_RESIZE launch of the styled frame beside them, from the same process, at 512x512 -> 1080x1920 and 512x512 ->
720x1280: device events around `--reps` back-to-back replays after a warm-up (microseconds per replay), `--rounds` rounds with
the variants alternating inside each round, so that a drift of the box shows in every variant alike.  The figure of a variant is
the median over the rounds; the spread is given."""
import argparse
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--radius", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib
    from live2diff_amd.detail import HipDetail, check_settings
    from live2diff_amd.resize import HipResize
    dev, H, W = "cuda", args.size, args.size
    settings = check_settings(radius=args.radius)
    g = torch.Generator().manual_seed(0)
    styled = (torch.randn(3, H, W, generator=g) * 0.7).half().to(dev)
    source = (torch.randn(3, H, W, generator=g) * 0.7).half().to(dev)
    say(args.out, f"# detail_time: {_lib.device_name()}, {H}x{W}, radius {args.radius}, {args.reps} back-to-back replays per figure "
                  f"(device events), {args.rounds} rounds, the variants alternating inside a round; median (min .. max) microseconds "
                  "per replay")
    for Ho, Wo in ((1080, 1920), (720, 1280)):
        rs = HipResize(H, W, Ho, Wo, "lanczos", device=dev)
        dt = HipDetail(H, W, Ho, Wo, "lanczos", device=dev)
        camera = torch.randint(0, 256, (Ho, Wo, 3), dtype=torch.uint8, generator=g).to(dev)
        rs.resize(styled, to_host=False)                 # (S holds a resized frame, as in the stream)
        three = dt.plan(rs.dev[0], styled, source, camera, settings)
        variants = [("op 46 resize of the styled frame (the plain launch)", rs._plan(styled)),
                    ("ops 50 + 46 + 51, the detail plan in sequence", three)]
        for name, i in (("op 50 gains", 0), ("op 46 resize of the source frame", 1), ("op 51 inject", 2)):
            fresh = dt.plan(rs.dev[0], styled, source, camera, settings)          # (a record carries its place in its own plan)
            pl = _lib.OpList()
            pl.append(fresh[i], *fresh._keep)
            variants.append((name + ", alone", pl))
        lists = []
        for name, pl in variants:
            pl.time_ms(20)
            lists.append((name, pl, []))
        for _ in range(args.rounds):
            for _, pl, us in lists:
                us.append(pl.time_ms(args.reps) * 1e3)
        say(args.out, f"{H}x{W} -> {Ho}x{Wo}")
        med = {}
        for name, _, us in lists:
            med[name] = statistics.median(us)
            say(args.out, f"  {name:52s}: {med[name]:7.2f} us ({min(us):.2f} .. {max(us):.2f})")
        each = [round(u, 2) for u in three.time_each_us(args.reps)]
        say(args.out, f"  in sequence, launch by launch (gains, source resize, inject): {each} us")
        say(args.out, f"  detail plan / plain resize = {med[variants[1][0]] / med[variants[0][0]]:.2f}")


if __name__ == "__main__":
    main()
