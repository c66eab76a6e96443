"""Timing of the depth matte (csrc/matte.hip, live2diff_amd/matte.py) on the MI355X.

    timeout -k 10 120 python tools/matte_time.py kernels --out profiles/matte_time.txt && \\
    timeout -k 10 900 python tools/matte_time.py route --out profiles/matte_time.txt

  kernels  L2D_OP_FRAME_MATTE at 512x512 with feather radius 0, 4 and 8 beside L2D_OP_FRAME_EGRESS on the same frame: device events
           around `--reps` back-to-back replays after a warm-up (microseconds per launch), the bytes each variant moves and
           what share of the achievable HBM rate that is.
  route    host uint8 frame -> host uint8 frame through the wrapper's "u8" output at full size (SD-1.5 widths, 512x512, 4
           denoising steps, synthetic weights as bench.py builds them), wall clock per frame, three stacks alternating frame by
           frame in one process: matte off, matte on (soft ramp, feather 4), and matte off again -- off against off is the
           run-to-run spread of one route against itself."""
import argparse
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

HBM_ACHIEVABLE = 6.3e12        # bytes / s: what streaming kernels reach on this part (8 TB/s is the specification)
TILE_H, TILE_W, HALO_W = 16, 64, 80      # matte.hip MT_TH, MT_TW, MT_MW


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def matte_bytes(H, W, r):
    """(compulsory bytes, bytes the launch asks for): two fp16 frames and one depth plane in, one uint8 frame out; with r > 0
    every tile reads the depth of its halo as well (served by L2 where tiles overlap)"""
    compulsory = H * W * (6 + 6 + 2 + 3)
    if r == 0:
        return compulsory, compulsory
    tiles = -(-H // TILE_H) * -(-W // TILE_W)
    return compulsory, H * W * (6 + 6 + 3) + tiles * (TILE_H + 2 * r) * HALO_W * 2


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import matte_params
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# matte_time kernels: {_lib.device_name()}, {H}x{W}, {args.reps} back-to-back replays per figure (device events); "
                  f"share = bytes / {HBM_ACHIEVABLE / 1e12:.1f} TB/s over the time")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev)
    src = (torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev)
    depth = (torch.randn(1, H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)

    def timed(op):
        pl = _lib.OpList()
        pl.append(op[0], *op[1])
        pl.time_ms(20)
        return [pl.time_ms(args.reps) * 1e3 for _ in range(3)]

    us = timed(ops.frame_egress(x, out, B=1, H=H, W=W))
    nbytes = H * W * 9
    say(args.out, f"op 35 egress          : {min(us):6.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)}); {nbytes / 1e6:.2f} MB moved, "
                  f"{nbytes / (min(us) * 1e-6) / HBM_ACHIEVABLE:.1%} of the HBM rate")
    lo32, inv32, hard = matte_params(0.3, 0.7)
    for r in (0, 4, 8):
        us = timed(ops.frame_matte(x, src, depth, out, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, r=r))
        need, asked = matte_bytes(H, W, r)
        say(args.out, f"op 43 matte, feather {r}: {min(us):6.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)}); {need / 1e6:.2f} MB "
                      f"moved ({asked / 1e6:.2f} MB asked for with the halo), {need / (min(us) * 1e-6) / HBM_ACHIEVABLE:.1%} of the HBM rate")
    lo32, inv32, hard = matte_params(0.5, 0.5)
    us = timed(ops.frame_matte(x, src, depth, out, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, r=8, far=True))
    say(args.out, f"op 43 hard, far, feather 8: {min(us):6.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)})")


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

    def wrapper(matte):
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type="u8", seed=3, device=dev, **kw)
        if matte:
            w.set_matte(0.3, 0.7, feather=4)
        w.prepare(warm, "a cat")
        return w

    stacks = [("off1 matte off", wrapper(False)), ("on   matte on (0.3, 0.7, feather 4)", wrapper(True)), ("off2 matte off, the same route again", wrapper(False))]
    t = {name: [] for name, _ in stacks}
    for i in range(args.warmup + args.frames):
        for name, fn in stacks:
            t0 = time.perf_counter()
            o = fn(frames[i % 4])
            dt = time.perf_counter() - t0
            assert o.shape == (H, W, 3) and o.dtype == np.uint8
            if i >= args.warmup:
                t[name].append(dt * 1e3)
    say(args.out, f"# matte_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, {args.frames} frames per stack after "
                  f"{args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 frame -> host uint8 frame")
    med = {}
    for name, _ in stacks:
        v = sorted(t[name])
        med[name[:4]] = statistics.median(v)
        say(args.out, f"{name}: median {statistics.median(v):.3f} ms, p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f}, min {v[0]:.3f}, max {v[-1]:.3f}")
    say(args.out, f"on - mean(off1, off2) = {med['on  '] - (med['off1'] + med['off2']) / 2:+.3f} ms; |off1 - off2| (one route against itself) = "
                  f"{abs(med['off1'] - med['off2']):.3f} ms")


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
