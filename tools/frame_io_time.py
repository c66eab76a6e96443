"""Timing of the device-side frame I/O (csrc/frame_io.hip, live2diff_amd/frame_io.py, live2diff_amd/wrapper.py) on the MI355X.

    timeout -k 10 120 python tools/frame_io_time.py kernels --out profiles/frame_io_time.txt && \\
    timeout -k 10 900 python tools/frame_io_time.py route --out profiles/frame_io_time.txt

  kernels  the ingest launch at 720x1280 -> 512x512 and 1080x1920 -> 512x768 and the egress launch at 512x512, device events
           around `--reps` replays after a warm-up (microseconds per launch).
  route    host uint8 frame -> host uint8 frame at full size (SD-1.5 widths, 512x512, 4 denoising steps, synthetic weights as
           bench.py builds them), wall clock per frame, three stacks alternating frame by frame in one process:
             W   the wrapper's "u8" path (pinned staging -> H2D of Hs Ws 3 bytes -> ingest launch -> pipeline -> egress launch
                 -> D2H of H W 3 bytes);
             P1, P2   the route the pipeline class alone offers for the same frame: np.uint8 -> `StreamAnimateDiffusionDepth.__call__`
                 (`_ImageProcessor`: uint8 -> fp32 on the host, fp32 upload) -> the reference's image_utils expressions on the
                 result (`x / 2 + 0.5 -> clamp -> cpu -> permute -> float -> x 255 -> round -> uint8`).
           At the identity geometry (512x512 source) all three do the same arithmetic; P1 against P2 is the run-to-run spread of
           one route against itself.  The wrapper on 720x1280 sources (antialiased resize + crop) is reported beside it, not
           compared: the pipeline class resizes in nearest mode, a different and cheaper filter."""
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


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.frame_io import geometry
    dev = "cuda"
    say(args.out, f"# frame_io_time kernels: {_lib.device_name()}, {args.reps} replays per figure (device events)")
    for (Hs, Ws), (H, W) in (((720, 1280), (512, 512)), ((1080, 1920), (512, 768)), ((512, 512), (512, 512))):
        nh, nw, top, left = geometry(Hs, Ws, H, W)
        src = torch.randint(0, 256, (1, Hs, Ws, 3), dtype=torch.uint8, device=dev)
        dst = torch.empty(1, 3, H, W, dtype=torch.float16, device=dev)
        pl = _lib.OpList()
        pl.append(*ops.frame_ingest(src, dst, B=1, Hs=Hs, Ws=Ws, H=H, W=W, nh=nh, nw=nw, top=top, left=left))
        pl.time_ms(20)
        us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
        say(args.out, f"ingest {Hs}x{Ws} -> {H}x{W}: {min(us):.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)}); "
                      f"{Hs * Ws * 3 / 1e6:.2f} MB in, {H * W * 6 / 1e6:.2f} MB out")
    x = (torch.rand(1, 3, 512, 512, device=dev) * 2 - 1).half()
    out = torch.empty(1, 512, 512, 3, dtype=torch.uint8, device=dev)
    pl = _lib.OpList()
    pl.append(*ops.frame_egress(x, out, B=1, H=512, W=512))
    pl.time_ms(20)
    us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
    say(args.out, f"egress 512x512: {min(us):.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)})")


def reference_u8(x):
    """image_utils.postprocess_image(x, "pil") up to the PIL object (image_utils.py:13,20,30)"""
    images = (x / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
    return (images * 255).round().astype("uint8")[0]


def route(args):
    from live2diff_amd import _lib
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, HipPromptEncoder, random_clip_text_state_dict
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    from live2diff_amd.config import sd15_config
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.pipeline_stream_animation_depth import StreamAnimateDiffusionDepth
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
    big = torch.randint(0, 256, (4, 720, 1280, 3), dtype=torch.uint8, generator=g).numpy()

    def wrapper():
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type="u8", seed=3, device=dev, **kw)
        w.prepare(warm, "a cat")
        return w

    def parent():
        s = StreamAnimateDiffusionDepth(pipe(), **kw)
        s.image_processor.assume_unit_range = True        # what bench.py sets: no `.min()` probe on the parent's side either
        s.prepare_cache(H, W, N)
        s.prepare(list(warm), prompt="a cat", seed=3)
        s.enable_device_step(seed=3)
        return lambda f: reference_u8(s(f))

    w, wbig = wrapper(), wrapper()
    stacks = [("W  wrapper u8 path, 512x512 source", w), ("P1 pipeline class + image_utils, 512x512 source", parent()),
              ("P2 the same route again", parent()), ("W720 wrapper u8 path, 720x1280 source (resize + crop)", None)]
    t = {name: [] for name, _ in stacks}
    n = args.warmup + args.frames
    for i in range(n):
        for name, fn in stacks:
            f = frames[i % 4] if fn is not None else big[i % 4]
            fn = fn or wbig
            t0 = time.perf_counter()
            o = fn(f)
            dt = time.perf_counter() - t0
            assert o.shape == (H, W, 3) and o.dtype == np.uint8
            if i >= args.warmup:
                t[name].append(dt * 1e3)
    say(args.out, f"# frame_io_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, {args.frames} frames per "
                  f"stack after {args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 frame -> host uint8 frame")
    med = {}
    for name, _ in stacks:
        v = sorted(t[name])
        med[name[:2]] = statistics.median(v)
        say(args.out, f"{name}: median {statistics.median(v):.3f} ms, p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f}, "
                      f"min {v[0]:.3f}, max {v[-1]:.3f}")
    spread = abs(med["P1"] - med["P2"])
    say(args.out, f"W - mean(P1, P2) = {med['W '] - (med['P1'] + med['P2']) / 2:+.3f} ms; |P1 - P2| (one route against itself) = {spread:.3f} ms")


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
