"""Timing of the backdrop (csrc/backdrop.hip, live2diff_amd/backdrop.py) on the MI355X.

    timeout -k 10 180 python tools/backdrop_time.py --out profiles/backdrop_time.txt

The matte composite with and without each backdrop kind, at 512x512 (L2D_OP_FRAME_MATTE) and at 512x512 -> 1080x1920
(L2D_OP_FRAME_MATTE_UP): the composite as it is (the real frame behind the matte), with a colour or an image (another pointer
in the same launch), and with the blur (L2D_OP_FRAME_BACKDROP_BLUR in front; at the output size L2D_OP_FRAME_RESIZE of the
blurred frame between the two), plus the blur launch alone at several settings.  Device events around `--reps` back-to-back
replays after a warm-up (microseconds per replay), `--rounds` rounds with the variants alternating inside each round, so that a
drift of the box shows in every variant alike.  The figure of a variant is the median over the rounds; the spread is given."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE_H, TILE_W, PAD = 16, 64, 24         # backdrop.hip BD_TH, BD_TW, BD_PAD


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def blur_bytes(H, W, r, passes):
    """(compulsory bytes, bytes the launch asks for): one fp16 frame and one depth plane in, one fp16 frame out; every tile
    reads the rows of its halo of passes * r in whole 8-pixel groups as well (served by L2 where tiles overlap)"""
    tiles = -(-H // TILE_H) * -(-W // TILE_W)
    halo = passes * r
    groups = (TILE_W + 2 * PAD) // 8 - 2 * ((PAD - halo) // 8)
    return H * W * (6 + 2 + 6), tiles * (TILE_H + 2 * halo) * groups * 8 * 8 + H * W * 6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out-height", type=int, default=1080)
    ap.add_argument("--out-width", type=int, default=1920)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib, ops
    from live2diff_amd.backdrop import HipBackdrop, check_settings
    from live2diff_amd.matte import _Slot, matte_params, table_words
    dev, H, W, Ho, Wo = "cuda", args.size, args.size, args.out_height, args.out_width
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev)
    slot = _Slot(H, W, dev)
    slot.source.copy_((torch.randn(3, H, W, generator=g) * 0.7).half())
    slot.depth.copy_((torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half())
    out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
    matte = dict(lo=0.3, hi=0.7, keep="near", feather=0, show=False)
    lo32, inv32, hard = matte_params(matte["lo"], matte["hi"])
    ramp = dict(lo32=lo32, inv32=inv32, hard=hard)
    hb = HipBackdrop(H, W, device=dev)
    room = torch.randint(0, 256, (720, 1280, 3), generator=g, dtype=torch.uint8).numpy()

    def blur(r, passes):
        return hb.blur_record(slot, matte, check_settings("blur", r, passes))

    def composite(kept):
        return ops.frame_matte(x, kept, slot.depth, out, B=1, H=H, W=W, r=0, **ramp)

    blur(6, 3)                                                             # (makes hb.frame)
    image16, _ = hb.stream(slot, matte, check_settings(room), room)
    variants = [("op 43 composite, the real frame behind", [composite(slot.source)]),
                ("op 43 composite over an image / a colour", [composite(image16)])]
    for r, passes in ((6, 3), (8, 3), (6, 1), (2, 1)):
        variants.append((f"op 54 blur alone, r {r}, {passes} passes", [blur(r, passes)]))
    for r, passes in ((6, 3), (8, 3)):
        variants.append((f"op 54 r {r} x {passes} + op 43 over its frame", [blur(r, passes), composite(hb.frame)]))

    # the output size: the styled bytes over the camera's own, over prepared bytes, and over the blurred frame resampled
    S, C, out_up = (torch.randint(0, 256, (1, Ho, Wo, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(3))
    tx, ty = (torch.from_numpy(table_words(i, o)).to(dev) for i, o in ((W, Wo), (H, Ho)))

    def composite_up(kept):
        return ops.frame_matte_up(S, kept, slot.depth, out_up, tx, ty, B=1, H=H, W=W, Ho=Ho, Wo=Wo, r=0, **ramp)

    image8, _ = hb.output(slot, matte, check_settings(room), Ho, Wo, room)
    blurred8, records = hb.output(slot, matte, check_settings("blur", 6, 3), Ho, Wo)
    variants += [(f"op 47 composite at {Ho}x{Wo}, the camera behind", [composite_up(C)]),
                 (f"op 47 composite at {Ho}x{Wo} over an image", [composite_up(image8[None])]),
                 ("op 54 r 6 x 3 + op 46 resize of its frame", list(records)),
                 ("op 54 r 6 x 3 + op 46 + op 47 over its bytes", list(records) + [composite_up(blurred8[None])])]
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
    say(args.out, f"# backdrop_time: {_lib.device_name()}, {H}x{W} (-> {Ho}x{Wo}), {args.reps} back-to-back replays per figure (device "
                  f"events), {args.rounds} rounds, the variants alternating inside a round; median (min .. max) microseconds per replay")
    med = {}
    for name, _, us in lists:
        med[name] = statistics.median(us)
        say(args.out, f"{name:50s}: {med[name]:7.2f} us ({min(us):.2f} .. {max(us):.2f})")
    base = med[variants[0][0]]
    for r, passes in ((6, 3), (8, 3)):
        need, asked = blur_bytes(H, W, r, passes)
        m = med[f"op 54 blur alone, r {r}, {passes} passes"]
        both = med[f"op 54 r {r} x {passes} + op 43 over its frame"]
        say(args.out, f"op 54 r {r} x {passes} / op 43 = {m / base:.2f}; a blurred frame adds {both - base:.2f} us to the composite; "
                      f"{need / 1e6:.2f} MB compulsory, {asked / 1e6:.2f} MB asked for with the halo")
    up = med[f"op 47 composite at {Ho}x{Wo}, the camera behind"]
    say(args.out, f"at {Ho}x{Wo} a blurred frame adds {med['op 54 r 6 x 3 + op 46 + op 47 over its bytes'] - up:.2f} us to the composite's {up:.2f} us")


if __name__ == "__main__":
    main()
