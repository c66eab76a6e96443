"""Timing of the output size (csrc/resize.hip, live2diff_amd/resize.py) on the MI355X.

    timeout -k 10 120 python tools/resize_time.py kernels --out profiles/resize_time.txt && \\
    timeout -k 10 900 python tools/resize_time.py route --out profiles/resize_time.txt

  kernels  L2D_OP_FRAME_RESIZE from a 512x512 frame to 1080x1080, 1088x1920 and 256x256, each filter, from the fp16 frame and from
           a uint8 frame, beside L2D_OP_FRAME_EGRESS on the same frame: device events around `--reps` back-to-back replays after
           a warm-up (microseconds per launch).
  route    on ONE wrapper at full size (SD-1.5 widths, 512x512, 4 denoising steps, synthetic weights as bench.py builds them),
           for "u8" and for "jpeg": the output route alone (the last fp16 frame on the device -> the host frame or file) and the
           whole call (host uint8 frame -> host frame or file), wall clock, with the output size off, on (1088x1088, Lanczos) and
           off again, alternating call by call -- off is the route as it was before there was an output size, and off against
           off is the run-to-run spread of one route against itself."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

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
    from live2diff_amd.resize import axis_table
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# resize_time kernels: {_lib.device_name()}, source {H}x{W}, {args.reps} back-to-back replays per figure (device events)")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev)
    u = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, generator=g).to(dev)

    def timed(op):
        pl = _lib.OpList()
        pl.append(op[0], *op[1])
        pl.time_ms(20)
        return [pl.time_ms(args.reps) * 1e3 for _ in range(3)]

    out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
    us = timed(ops.frame_egress(x, out, B=1, H=H, W=W))
    say(args.out, f"op 35 egress {H}x{W}                  : {min(us):6.2f} us per launch (3 runs: {', '.join(f'{v:.2f}' for v in us)})")
    for Ho, Wo in ((1080, 1080), (1088, 1920), (256, 256)):
        out = torch.empty(1, Ho, Wo, 3, dtype=torch.uint8, device=dev)
        for resample in ("lanczos", "bicubic", "bilinear"):
            tx, ty = (torch.from_numpy(axis_table(i, o, resample)).to(dev) for i, o in ((W, Wo), (H, Ho)))
            for name, src in (("fp16 ", x), ("uint8", u)):
                us = timed(ops.frame_resize(src, out, tx, ty, B=1, H=H, W=W, Ho=Ho, Wo=Wo))
                say(args.out, f"op 46 {name} -> {Ho:4d}x{Wo:<4d} {resample:8s}: {min(us):6.2f} us per launch (3 runs: "
                              f"{', '.join(f'{v:.2f}' for v in us)}); {Ho * Wo * 3 / 1e6:.2f} MB written")


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
    Ho, Wo = 1088, 1088
    cfg = sd15_config()
    tok = ClipTokenizer.from_dir(os.path.join(ROOT, "tests", "golden", "clip_tok"))
    penc = HipPromptEncoder(HipClipTextEncoder(random_clip_text_state_dict(SD15_CLIP, 3), dev, SD15_CLIP), tok, default_clip_skip=1)
    pipe = SimpleNamespace(device=torch.device(dev), vae_scale_factor=8, scheduler=None, _encode_prompt=penc._encode_prompt,
                           unet=HipStreamingUNet(device_random_state_dict(cfg, dev), cfg, H // 8, W // 8, N, device=dev),
                           vae=HipTinyVAE(random_taesd_state_dict(device=dev), device=dev),
                           depth_model=HipMidas(random_midas_state_dict(device=dev), device=dev))
    g = torch.Generator().manual_seed(1)
    warm = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, generator=g).numpy()
    frames = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, generator=g).numpy()
    w = StreamAnimateDiffusionDepthWrapper.from_components(pipe, output_type="u8", seed=3, device=dev, num_inference_steps=50,
                                                           t_index_list=[25, 31, 37, 43], width=W, height=H,
                                                           warmup_frames=cfg.sink_size, window_size=cfg.window_size)
    w.prepare(warm, "a cat")
    say(args.out, f"# resize_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, one wrapper; {args.frames} calls per "
                  f"variant after {args.warmup} warm-up, variants alternating call by call; output size {Ho}x{Wo} lanczos; wall clock")
    variants = ("off1", "on  ", "off2")

    w.set_output_size(Ho, Wo)
    size = w._size

    def switch(name):
        # (`clear_output_size` frees the tables, the buffers and the encoder, and the next frame would build them again inside the
        # timed call: the setting alone is taken away and put back)
        w._size = size if name == "on  " else None

    def show(tag, t):
        med = {}
        for name in variants:
            v = sorted(t[name])
            med[name] = statistics.median(v)
            say(args.out, f"{tag} {name}: median {med[name]:.3f} ms, p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f}, min {v[0]:.3f}")
        say(args.out, f"{tag} on - mean(off1, off2) = {med['on  '] - (med['off1'] + med['off2']) / 2:+.3f} ms; |off1 - off2| = "
                      f"{abs(med['off1'] - med['off2']):.3f} ms")

    for ot in ("u8", "jpeg"):
        w.output_type = ot
        # the whole call
        t = {name: [] for name in variants}
        for i in range(args.warmup + args.frames):
            for name in variants:
                switch(name)
                t0 = time.perf_counter()
                o = w(frames[i % 4])
                dt = time.perf_counter() - t0
                assert (o.shape == ((Ho, Wo, 3) if name == "on  " else (H, W, 3))) if ot == "u8" else o[:2] == b"\xff\xd8"
                if i >= args.warmup:
                    t[name].append(dt * 1e3)
        show(f"{ot:4s} whole call  ", t)
        # the output route alone, on the frame the stream made last
        x = w.stream.prev_image_result
        t = {name: [] for name in variants}
        for i in range(args.warmup + args.frames):
            for name in variants:
                switch(name)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = w._finish(x, None) if name == "on  " else w.postprocess_image(x, output_type=ot)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    t[name].append(dt * 1e3)
        show(f"{ot:4s} output route", t)
        if ot == "jpeg":
            say(args.out, f"jpeg file: {len(o)} bytes at {H}x{W}")
    w.clear_output_size()


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
