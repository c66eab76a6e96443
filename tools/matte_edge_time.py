"""Timing of the edge-aware matte (csrc/matte_edge.hip, live2diff_amd/matte.py) on the MI355X.

    timeout -k 10 120 python tools/matte_edge_time.py --out profiles/matte_edge_time.txt

L2D_OP_FRAME_MATTE_EDGE at 512x512 with radius 4 and 8, beside the plain L2D_OP_FRAME_MATTE launch (feather 0) on the same
frame and the pair a refined frame pays for (op 49, then op 43 reading its plane): device events around `--reps` back-to-back
replays after a warm-up (microseconds per launch), `--rounds` rounds with the variants alternating inside each round, so that a
drift of the box shows in every variant alike.  The figure of a variant is the median over the rounds; the spread is given."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE_H, TILE_W, PAD = 16, 64, 16         # matte_edge.hip ME_TH, ME_TW, ME_PAD


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def edge_bytes(H, W, r):
    """(compulsory bytes, bytes the launch asks for): one fp16 frame and one depth plane in, one fp32 plane out; every tile
    reads the rows of its halo of 2r in whole 8-pixel groups as well (served by L2 where tiles overlap)"""
    tiles = -(-H // TILE_H) * -(-W // TILE_W)
    groups = (TILE_W + 2 * PAD) // 8 - 2 * ((PAD - 2 * r) // 8)
    return H * W * (6 + 2 + 4), tiles * (TILE_H + 4 * r) * groups * 8 * 8 + H * W * 4


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import edge_E, matte_params
    dev, H, W = "cuda", args.size, args.size
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev)
    src = (torch.randn(3, H, W, generator=g) * 0.7).half().to(dev)
    depth = (torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
    plane = torch.empty(H, W, dtype=torch.float32, device=dev)
    lo32, inv32, hard = matte_params(0.3, 0.7)
    ramp = dict(lo32=lo32, inv32=inv32, hard=hard)

    def edge(r):
        return ops.frame_matte_edge(src, depth, plane, H=H, W=W, r=r, E=edge_E(r, 10.0), **ramp)

    variants = [("op 43 matte, feather 0 (the plain launch)", [ops.frame_matte(x, src, depth, out, B=1, H=H, W=W, r=0, **ramp)])]
    for r in (4, 8):
        variants.append((f"op 49 matte edge, r {r}", [edge(r)]))
    for r in (4, 8):
        variants.append((f"op 49 r {r} + op 43 on its plane", [edge(r), ops.frame_matte(x, src, None, out, B=1, H=H, W=W, r=0, plane=plane)]))
    lists = []
    for name, recs in variants:
        pl = _lib.OpList()
        for op, keep in recs:
            pl.append(op, *keep)
        pl.time_ms(20)
        lists.append((name, pl, []))
    for _ in range(args.rounds):
        for _, pl, us in lists:
            us.append(pl.time_ms(args.reps) * 1e3)
    say(args.out, f"# matte_edge_time: {_lib.device_name()}, {H}x{W}, {args.reps} back-to-back replays per figure (device events), "
                  f"{args.rounds} rounds, the variants alternating inside a round; median (min .. max) microseconds per replay")
    med = {}
    for name, _, us in lists:
        med[name] = statistics.median(us)
        say(args.out, f"{name:44s}: {med[name]:7.2f} us ({min(us):.2f} .. {max(us):.2f})")
    base = med[variants[0][0]]
    for r in (4, 8):
        need, asked = edge_bytes(H, W, r)
        m = med[f"op 49 matte edge, r {r}"]
        say(args.out, f"op 49 r {r} / op 43 = {m / base:.2f}; {need / 1e6:.2f} MB compulsory, {asked / 1e6:.2f} MB asked for with the halo")


if __name__ == "__main__":
    main()
