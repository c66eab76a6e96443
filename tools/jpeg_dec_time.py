"""Timing of the device-side JPEG decoder (csrc/jpeg_dec.hip, live2diff_amd/jpeg_io.py, the wrapper's bytes input) on the MI355X.

    timeout -k 10 300 python tools/jpeg_dec_time.py kernels --out profiles/jpeg_dec_time.txt && \\
    timeout -k 10 300 python tools/jpeg_dec_time.py route --out profiles/jpeg_dec_time.txt

Sources for everything: Pillow-encoded frames at quality 90 (4:2:0, standard tables, no restart markers -- what a browser's
`canvas.toBlob('image/jpeg')` and most cameras send), 640x480, 1280x720 and 1920x1080: a smooth frame (32 / 93 / 208 KB), the same
with sensor-like noise of sigma 6 on it ("textured": 77 / 229 / 514 KB, the size of a camera frame), and uniform noise (the worst case).

  kernels  the three-launch plan (entropy, idct, rgb): device events around `--reps` back-to-back replays after a warm-up
           (microseconds per plan) and the in-sequence time of every launch (`time_each_us`), per source; the sweep of `chunk_mcus`
           at 1280x720 the default is taken from; and the host's share per frame (`parse` + table blob + `l2d_jpeg_index`, wall clock)
           beside Pillow's `Image.open(...).convert("RGB")` of the same file on the same host.
  route    host bytes -> ingested fp16 [1,3,512,512] frame on the device, wall clock per frame including the synchronisation that
           ends it, three stacks alternating frame by frame in one process:
             D        `HipFrameIO.ingest(HipJpegDecoder.decode(file))`: one upload of the file, three decode launches, one ingest launch;
             P1, P2   the route without the device decoder: Pillow's decode on the host, then `HipFrameIO.ingest` of the uint8 frame
                      (staging copy, upload of H W 3 bytes, ingest launch).
           P1 against P2 is the run-to-run spread of one route against itself."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((480, 640), (720, 1280), (1080, 1920))
QUALITY = 90


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


KINDS = ("smooth", "textured", "noise")


def smooth(H, W, sigma=0.0):
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 51.0), 128 + 90 * np.cos(yy / 23.0), xx * 255.0 / W], -1)
    return np.clip(s + np.random.default_rng(0).normal(0, sigma, s.shape) if sigma else s, 0, 255).astype(np.uint8)


def source(kind, H, W):
    from PIL import Image
    u8 = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == "noise" else smooth(H, W, 6.0 * (kind == "textured"))
    b = io.BytesIO()
    Image.fromarray(u8).save(b, format="JPEG", quality=QUALITY)
    return b.getvalue()


def pillow_decode(f):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def wall_ms(fn, n):
    v = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(v), min(v)


def plan_of(dec, f):
    """decode once (fills the slot's buffers with this file), return that slot's plan: replaying it decodes the same file again"""
    out = dec.decode(f)
    dec.check()
    slot = next(s for slots, _ in dec._geo.values() for s in slots if s.out.data_ptr() == out.data_ptr())
    return slot.plan, out


def kernels(args):
    from live2diff_amd import _lib, jpeg, ops
    from live2diff_amd.jpeg_io import DEFAULT_CHUNK_MCUS, HipJpegDecoder
    dev = "cuda"
    say(args.out, f"# jpeg_dec_time kernels: {_lib.device_name()}, Pillow-encoded sources at quality {QUALITY} (4:2:0), chunk_mcus "
                  f"{DEFAULT_CHUNK_MCUS}, {args.reps} back-to-back replays per figure (device events)")
    files = {(k, H, W): source(k, H, W) for H, W in SIZES for k in KINDS}
    for (k, H, W), f in files.items():
        pl, out = plan_of(HipJpegDecoder(device=dev), f)
        assert np.array_equal(out.cpu().numpy(), pillow_decode(f)), "the decoder's frame differs from Pillow's"
        pl.time_ms(20)
        us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
        each = pl.time_each_us(20)
        say(args.out, f"decode {W}x{H} {k}: {min(us):.2f} us per plan (3 runs: {', '.join(f'{u:.2f}' for u in us)}); in sequence entropy "
                      f"{each[0]:.2f} + idct {each[1]:.2f} + rgb {each[2]:.2f} us; file {len(f)} bytes")
    say(args.out, f"# chunk_mcus sweep at 1280x720 ({args.reps} replays, best of 3), microseconds per plan")
    for cm in (1, 2, 4, 8, 16, 40, 80):
        cells = []
        for k in KINDS:
            pl, _ = plan_of(HipJpegDecoder(device=dev, chunk_mcus=cm), files[(k, 720, 1280)])
            pl.time_ms(20)
            cells.append(f"{k} {min(pl.time_ms(args.reps) * 1e3 for _ in range(3)):.2f} (entropy {pl.time_each_us(20)[0]:.2f})")
        say(args.out, f"chunk_mcus {cm}: " + ", ".join(cells))
    say(args.out, f"# host share per frame, wall clock, median (min) of {args.host_reps} runs, this host")
    for (k, H, W), f in files.items():
        def host():
            info = jpeg.parse(f)
            ops.jpeg_index(info, f, DEFAULT_CHUNK_MCUS, jpeg.table_blob(info))
        a, b = wall_ms(host, args.host_reps), wall_ms(lambda: pillow_decode(f), args.host_reps)
        say(args.out, f"host {W}x{H} {k}: parse + blob + l2d_jpeg_index {a[0]:.3f} ms ({a[1]:.3f}); Pillow open + convert {b[0]:.3f} ms ({b[1]:.3f})")


def route(args):
    from live2diff_amd import _lib
    from live2diff_amd.frame_io import HipFrameIO
    from live2diff_amd.jpeg_io import HipJpegDecoder
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# jpeg_dec_time route: {_lib.device_name()}, host bytes -> ingested fp16 [1,3,{H},{W}] on the device, wall clock with the "
                  f"synchronisation behind it, {args.frames} frames per stack after {args.warmup} warm-up, stacks alternating frame by frame")
    for Hs, Ws in SIZES:
        for k in KINDS if args.noise else KINDS[:2]:
            f = source(k, Hs, Ws)
            dec, iod, io1, io2 = HipJpegDecoder(device=dev), HipFrameIO(H, W, device=dev), HipFrameIO(H, W, device=dev), HipFrameIO(H, W, device=dev)

            def device():
                x = iod.ingest(dec.decode(f))
                torch.cuda.current_stream().synchronize()
                dec.check()
                return x

            def parent(io_):
                x = io_.ingest(pillow_decode(f))
                torch.cuda.current_stream().synchronize()
                return x

            stacks = [("D ", device), ("P1", lambda: parent(io1)), ("P2", lambda: parent(io2))]
            t = {n: [] for n, _ in stacks}
            for i in range(args.warmup + args.frames):
                got = {}
                for n, fn in stacks:
                    t0 = time.perf_counter()
                    got[n] = fn()
                    if i >= args.warmup:
                        t[n].append((time.perf_counter() - t0) * 1e3)
                if i == 0:
                    assert torch.equal(got["D "], got["P1"]) and torch.equal(got["P1"], got["P2"]), "the routes ingest different frames"
            med = {n: statistics.median(v) for n, v in t.items()}
            line = "; ".join(f"{n.strip()} median {med[n]:.3f} ms (p10 {sorted(v)[len(v) // 10]:.3f}, p90 {sorted(v)[len(v) * 9 // 10]:.3f})" for n, v in t.items())
            say(args.out, f"route {Ws}x{Hs} {k} ({len(f)} bytes): {line}; D - mean(P1, P2) = {med['D '] - (med['P1'] + med['P2']) / 2:+.3f} ms; "
                          f"|P1 - P2| = {abs(med['P1'] - med['P2']):.3f} ms")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=("kernels", "route"))
    ap.add_argument("--out", default=None, help="append the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--noise", action="store_true", help="route: the noise sources too")
    args = ap.parse_args(argv)
    {"kernels": kernels, "route": route}[args.mode](args)


if __name__ == "__main__":
    main()
