"""Timing of the device-side JPEG encoder (csrc/jpeg.hip, live2diff_amd/jpeg_io.py, the wrapper's "jpeg" output type) on the MI355X.

    timeout -k 10 120 python tools/jpeg_time.py kernels --out profiles/jpeg_time.txt && \\
    timeout -k 10 900 python tools/jpeg_time.py route --out profiles/jpeg_time.txt

  kernels  the three-launch plan (dct, huff, pack) at 512x512, 512x768 and 576x1024, quality 75, on a smooth frame and on uniform
           noise: device events around `--reps` back-to-back replays after a warm-up (microseconds per plan), the in-sequence time
           of every launch (`time_each_us`), the file's size, and the egress launch the plan replaces beside it.
  route    host uint8 frame -> host JPEG bytes at full size (SD-1.5 widths, 512x512, 4 denoising steps, synthetic weights as
           bench.py builds them), wall clock per frame, three stacks alternating frame by frame in one process:
             J        the wrapper's "jpeg" path (ingest -> pipeline -> dct, huff, pack -> D2H of the file);
             P1, P2   the route without the device encoder: the wrapper's "u8" path (egress launch, D2H of H W 3 bytes) followed by
                      Pillow's `save(format="JPEG", quality=75, restart_marker_rows=1)` -- the same file, byte for byte.
           P1 against P2 is the run-to-run spread of one route against itself.  Pillow's encode alone and the bytes each route
           copies per frame are reported beside it."""
import argparse
import io
import os
import statistics
import sys
import time
from types import SimpleNamespace

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


def smooth(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 51.0), 128 + 90 * np.cos(yy / 23.0), xx * 255.0 / W], -1)
    return np.clip(s + np.random.default_rng(0).normal(0, 6, s.shape), 0, 255).astype(np.uint8)


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.jpeg_io import HipJpegEncoder
    dev = "cuda"
    say(args.out, f"# jpeg_time kernels: {_lib.device_name()}, quality 75, {args.reps} back-to-back replays per figure (device events)")
    for H, W in ((512, 512), (512, 768), (576, 1024)):
        enc = HipJpegEncoder(H, W, 75, device=dev)
        for name, f in (("smooth", smooth(H, W)), ("noise", np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8))):
            x = (torch.from_numpy(f).to(dev).permute(2, 0, 1)[None].float() / 127.5 - 1.0).half().contiguous()     # what a decoder hands over
            size = len(enc.encode(x[0]))
            pl = enc.plan(x, 1)
            pl.time_ms(20)
            us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
            each = pl.time_each_us(20)
            say(args.out, f"jpeg {H}x{W} {name}: {min(us):.2f} us per plan (3 runs: {', '.join(f'{u:.2f}' for u in us)}); in sequence "
                          f"dct {each[0]:.2f} + huff {each[1]:.2f} + pack {each[2]:.2f} us; file {size} bytes of {H * W * 3} raw")
        x = (torch.rand(1, 3, H, W, device=dev) * 2 - 1).half()
        out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
        pl = _lib.OpList()
        pl.append(*ops.frame_egress(x, out, B=1, H=H, W=W))
        pl.time_ms(20)
        us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
        say(args.out, f"egress {H}x{W} (the launch the plan replaces): {min(us):.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)})")


def pillow_jpeg(u8, quality=75):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(u8).save(b, format="JPEG", quality=quality, restart_marker_rows=1)
    return b.getvalue()


def route(args):
    from live2diff_amd import _lib
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, HipPromptEncoder, random_clip_text_state_dict
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    from live2diff_amd.config import sd15_config
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.vae_hip import HipTinyVAE, random_taesd_state_dict
    from live2diff_amd.weights import device_random_state_dict
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper
    dev, H, W, N = "cuda", 512, 512, 4
    cfg = sd15_config()
    unet_sd = device_random_state_dict(cfg, dev)
    vae_sd, midas_sd = random_taesd_state_dict(device=dev), random_midas_state_dict(device=dev)
    clip_sd = random_clip_text_state_dict(SD15_CLIP, 3)
    tok = ClipTokenizer.from_dir(os.path.join(ROOT, "tests", "golden", "clip_tok"))
    first = []

    def pipe():
        unet = HipStreamingUNet(first[0] if first else unet_sd, cfg, H // 8, W // 8, N, device=dev)
        first.append(unet)
        penc = HipPromptEncoder(HipClipTextEncoder(clip_sd, dev, SD15_CLIP), tok, default_clip_skip=1)
        return SimpleNamespace(device=torch.device(dev), vae_scale_factor=8, unet=unet, vae=HipTinyVAE(vae_sd, device=dev),
                               depth_model=HipMidas(midas_sd, device=dev), scheduler=None, _encode_prompt=penc._encode_prompt)

    kw = dict(num_inference_steps=50, t_index_list=[25, 31, 37, 43], width=W, height=H, warmup_frames=cfg.sink_size, window_size=cfg.window_size)
    g = torch.Generator().manual_seed(1)
    warm = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, generator=g).numpy()
    frames = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, generator=g).numpy()

    def wrapper(output_type):
        torch.manual_seed(0)
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type=output_type, seed=3, device=dev, **kw)
        w.prepare(warm, "a cat")
        return w

    wj, w1, w2 = wrapper("jpeg"), wrapper("u8"), wrapper("u8")
    stacks = [("J  wrapper jpeg path", wj), ("P1 wrapper u8 path + Pillow save", lambda f: pillow_jpeg(w1(f))),
              ("P2 the same route again", lambda f: pillow_jpeg(w2(f)))]
    t = {name: [] for name, _ in stacks}
    sizes, same, last = [], 0, {}
    for i in range(args.warmup + args.frames):
        for name, fn in stacks:
            t0 = time.perf_counter()
            o = fn(frames[i % 4])
            dt = time.perf_counter() - t0
            assert isinstance(o, bytes) and o[:2] == b"\xff\xd8"
            last[name[:2]] = o
            if i >= args.warmup:
                t[name].append(dt * 1e3)
        same += last["J "] == last["P1"] == last["P2"]
        sizes.append(len(last["J "]))
    say(args.out, f"# jpeg_time route: {_lib.device_name()}, SD-1.5 widths (synthetic weights), {H}x{W}, {N} denoising steps, quality 75, "
                  f"{args.frames} frames per stack after {args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 "
                  f"frame -> host JPEG bytes")
    med = {}
    for name, _ in stacks:
        v = sorted(t[name])
        med[name[:2]] = statistics.median(v)
        say(args.out, f"{name}: median {statistics.median(v):.3f} ms, p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f}, "
                      f"min {v[0]:.3f}, max {v[-1]:.3f}")
    spread = abs(med["P1"] - med["P2"])
    say(args.out, f"J - mean(P1, P2) = {med['J '] - (med['P1'] + med['P2']) / 2:+.3f} ms; |P1 - P2| (one route against itself) = {spread:.3f} ms")
    say(args.out, f"files: the three stacks gave the same bytes in {same} of {len(sizes)} frames; size median {int(statistics.median(sizes))} "
                  f"bytes (min {min(sizes)}, max {max(sizes)}); copied to the host per frame: J {wj.jpeg.last_copied_bytes} bytes in "
                  f"{wj.jpeg.last_copies} copy, P {H * W * 3} bytes")
    u8 = w1(frames[0])
    enc = []
    for _ in range(args.frames):
        t0 = time.perf_counter()
        pillow_jpeg(u8)
        enc.append((time.perf_counter() - t0) * 1e3)
    say(args.out, f"Pillow save alone on such a frame, this host: median {statistics.median(enc):.3f} ms (min {min(enc):.3f})")
    each = wj.jpeg._batches[1].plan.time_each_us(20)
    say(args.out, f"the plan inside J, in sequence: dct {each[0]:.2f} + huff {each[1]:.2f} + pack {each[2]:.2f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("part", choices=["kernels", "route"])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernels": kernels, "route": route}[args.part](args)


if __name__ == "__main__":
    main()
