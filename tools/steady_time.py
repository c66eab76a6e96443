"""Timing of the steady mode (csrc/steady.hip, live2diff_amd/steady.py) on the MI355X.

    timeout -k 10 120 python tools/steady_time.py kernels --out profiles/steady_time.txt && \\
    timeout -k 10 900 python tools/steady_time.py route --out profiles/steady_time.txt

  kernels  L2D_OP_FRAME_STEADY at 512x512 with r = 0, 2, 8 (and the init form) beside L2D_OP_FRAME_MATTE with feather 0, 2, 8 on
           the same frame -- the yardstick: the same tile plan, 1 / 1.2 of the bytes: device events around `--reps`
           back-to-back replays after a warm-up, the minimum of three runs (microseconds per launch), and the bytes each launch
           moves.
  route    host uint8 frame -> host uint8 frame through the wrapper's "u8" output at full size (SD-1.5 widths, 512x512, 4
           denoising steps, synthetic weights as bench.py builds them), wall clock per frame, three stacks alternating frame
           by frame in one process: steady off, steady on (defaults), and steady off again -- off against off is the run-to-run
           spread of one route against itself.  The frames hold three quarters of the picture still.

    timeout -k 10 120 python tools/steady_time.py kernels --follow 4 --out profiles/steady_follow_time.txt

  kernels --follow R[,BIAS]   follow (csrc/steady_follow.hip): L2D_OP_FRAME_STEADY alone beside
           L2D_OP_FRAME_MOTION + L2D_OP_FRAME_STEADY_FOLLOW in one OpList, at 512x512 and 1280x720, at the search range R given and
           at 4 and 8, in the same run with the same device events; the source is the previous one panned by (3, -2) pixels."""
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


def parse_follow(text):
    """`R[,BIAS]` -> `steady.check_follow`'s dict"""
    from live2diff_amd.steady import check_follow
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise ValueError(f"--follow {text!r}: use R[,BIAS]")
    return check_follow(int(parts[0]), int(parts[1]) if len(parts) > 1 else 256)


def follow_kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.steady import HipSteady, steady_params
    dev, follow = "cuda", parse_follow(args.follow)
    say(args.out, f"# steady_time kernels --follow: {_lib.device_name()}, bias {follow['bias']}, steady r = 2, {args.reps} back-to-back replays "
                  f"per figure (device events), minimum of 3 runs; the source is the previous one panned by (3, -2)")
    lo32, inv32, hard = steady_params(2, 10)
    settings = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)
    for H, W in ((512, 512), (720, 1280)):
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(1, 3, H, W, generator=g) * 0.6).half().to(dev)
        canvas = torch.nn.functional.avg_pool2d(torch.randint(0, 256, (3, H + 16, W + 16), generator=g).float()[None], 3, 1, 1)[0].round()
        src0, src1 = ((canvas[:, 8 + oy:8 + oy + H, 8 + ox:8 + ox + W] / 127.5 - 1.0).half().to(dev)[None].contiguous()
                      for oy, ox in ((0, 0), (-3, 2)))
        st = HipSteady(H, W, device=dev)
        st.steady(x, src0, settings, init=True)                                      # (a state for what follows)
        st.steady(x, src1, settings, follow=follow)                                  # (... and a field buffer)
        moved = float((st.field != 0).any(dim=-1).float().mean())
        (prev_out, prev_bytes), (out, next_bytes) = st.records[st._cur], st.records[1 - st._cur]
        common = dict(H=H, W=W, lo32=lo32, inv32=inv32, s32=0.8, r=2, hard=hard)

        def timed(name, *ops_):
            pl = _lib.OpList()
            for op in ops_:
                pl.append(op[0], *op[1])
            pl.time_ms(20)
            us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
            say(args.out, f"{H}x{W} {name:40s}: {min(us):7.2f} us (3 runs: {', '.join(f'{u:.2f}' for u in us)})")
            return min(us)

        base = timed("op 48 steady alone", ops.frame_steady(x, src1, prev_out, prev_bytes, out, next_bytes, **common))
        timed("op 56 follow alone (the field as it is)", ops.frame_steady_follow(x, src1, prev_out, prev_bytes, out, next_bytes, st.field, **common))
        for R in sorted({follow["search"], 4, 8}):
            motion = ops.frame_motion(src1, prev_bytes, st.field, H=H, W=W, search=R, bias=follow["bias"])
            timed(f"op 55 motion alone, R = {R}", motion)
            both = timed(f"ops 55 + 56, R = {R}", motion, ops.frame_steady_follow(x, src1, prev_out, prev_bytes, out, next_bytes, st.field, **common))
            say(args.out, f"{H}x{W} ops 55 + 56 at R = {R} against op 48: {both / base:.2f} x, {both - base:+.2f} us")
        say(args.out, f"{H}x{W} share of blocks with a vector at R = {follow['search']}: {moved:.2f}")


def kernels(args):
    if args.follow:
        return follow_kernels(args)
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import matte_params
    from live2diff_amd.steady import HipSteady, steady_params
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# steady_time kernels: {_lib.device_name()}, {H}x{W}, {args.reps} back-to-back replays per figure (device events), "
                  f"minimum of 3 runs")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.6).half().to(dev)
    before = torch.randint(0, 256, (3, H, W), generator=g)
    now = (before + torch.randint(-1, 2, (3, H, W), generator=g)).clamp(0, 255)
    now[:, :, : W // 4] = torch.randint(0, 256, (3, H, W // 4), generator=g)          # a quarter of the picture moves
    src0, src1 = ((b / 127.5 - 1.0).half().to(dev)[None] for b in (before, now))
    depth = (torch.randn(1, H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    u8 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
    st = HipSteady(H, W, device=dev)
    settings = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)
    st.steady(x, src0, settings, init=True)                                          # (a state for what follows)
    (prev_out, prev_bytes), (out, next_bytes) = st.records[st._cur], st.records[1 - st._cur]

    def timed(name, op, nbytes):
        pl = _lib.OpList()
        pl.append(op[0], *op[1])
        pl.time_ms(20)
        us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
        say(args.out, f"{name:34s}: {min(us):6.2f} us per launch (3 runs: {', '.join(f'{u:.2f}' for u in us)}); {nbytes / 1e6:.2f} MB moved")

    lo32, inv32, hard = matte_params(0.3, 0.7)
    for r in (0, 2, 8):
        timed(f"op 43 matte, feather {r}", ops.frame_matte(x, src1, depth, u8, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, r=r),
              H * W * 17)
    lo32, inv32, hard = steady_params(2, 10)
    for r in (0, 2, 8):
        timed(f"op 48 steady, r = {r}", ops.frame_steady(x, src1, prev_out, prev_bytes, out, next_bytes, H=H, W=W, lo32=lo32, inv32=inv32,
                                                        s32=0.8, r=r, hard=hard), H * W * 30)
    timed("op 48 steady, init", ops.frame_steady(x, src1, None, None, out, next_bytes, H=H, W=W, lo32=lo32, inv32=inv32, s32=0.8, r=2,
                                                 hard=hard, init=True), H * W * 21)


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
    fresh = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, generator=g).numpy()
    frames = np.stack([fresh[0]] * 4)
    for k in range(4):
        frames[k, :, k * W // 8:k * W // 8 + W // 4] = fresh[k, :, k * W // 8:k * W // 8 + W // 4]

    def wrapper(steady):
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type="u8", seed=3, device=dev, **kw)
        if steady:
            w.set_steady()
        w.prepare(warm, "a cat")
        return w

    stacks = [("off1 steady off", wrapper(False)), ("on   steady on (delay line + 1 launch)", wrapper(True)),
              ("off2 steady off, the same route again", wrapper(False))]
    t = {name: [] for name, _ in stacks}
    for i in range(args.warmup + args.frames):
        for name, fn in stacks:
            t0 = time.perf_counter()
            o = fn(frames[i % 4])
            dt = time.perf_counter() - t0
            assert o.shape == (H, W, 3) and o.dtype == np.uint8
            if i >= args.warmup:
                t[name].append(dt * 1e3)
    say(args.out, f"# steady_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, {args.frames} frames per stack "
                  f"after {args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 frame -> host uint8 frame")
    med = {}
    for name, _ in stacks:
        v = sorted(t[name])
        med[name[:4]] = statistics.median(v)
        say(args.out, f"{name}: median {statistics.median(v):.3f} ms ({1e3 / statistics.median(v):.2f} frames/s), p10 {v[len(v) // 10]:.3f}, "
                      f"p90 {v[len(v) * 9 // 10]:.3f}, min {v[0]:.3f}, max {v[-1]:.3f}")
    off = (med["off1"] + med["off2"]) / 2
    say(args.out, f"on - mean(off1, off2) = {med['on  '] - off:+.3f} ms; |off1 - off2| (one route against itself) = "
                  f"{abs(med['off1'] - med['off2']):.3f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("part", choices=["kernels", "route"])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--follow", default=None, metavar="R[,BIAS]", help="with `kernels`: time op 48 beside ops 55 + 56 instead")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernels": kernels, "route": route}[args.part](args)


if __name__ == "__main__":
    main()
