"""Timing of the matte hold (csrc/matte_hold.hip, live2diff_amd/matte.py) on the MI355X.

    timeout -k 10 120 python tools/matte_hold_time.py kernels --out profiles/matte_hold_time.txt && \\
    timeout -k 10 900 python tools/matte_hold_time.py route --out profiles/matte_hold_time.txt

  kernels  L2D_OP_FRAME_MATTE_HOLD alone (the depth form and the plane form, r = 2, and r = 0 and 8), and L2D_OP_FRAME_MOTION +
           L2D_OP_FRAME_MATTE_HOLD at search = 4 in one OpList, at 512x512 and 1280x720, beside L2D_OP_FRAME_STEADY (r = 2) and
           L2D_OP_FRAME_MATTE (feather 2) on the same frame -- the yardsticks -- in the same run with the same device events
           around `--reps` back-to-back replays after a warm-up, the minimum of three runs (microseconds per launch).  The
           source is the previous one panned by (3, -2) pixels.
  route    host uint8 frame -> host uint8 frame through the wrapper's "u8" output at full size (SD-1.5 widths, 512x512, 4
           denoising steps, synthetic weights as bench.py builds them) under a matte, wall clock per frame, three stacks
           alternating frame by frame in one process: hold off, hold on (defaults), and hold off again -- off against off is
           the run-to-run spread of one route against itself."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from steady_time import say  # noqa: E402


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import HipMatteHold, matte_params
    from live2diff_amd.steady import HipSteady, steady_params
    dev = "cuda"
    say(args.out, f"# matte_hold_time kernels: {_lib.device_name()}, {args.reps} back-to-back replays per figure (device events), minimum "
                  f"of 3 runs; the source is the previous one panned by (3, -2)")
    lo32, inv32, hard = steady_params(2, 10)
    rlo, rinv, rhard = matte_params(0.3, 0.7)
    for H, W in ((512, 512), (720, 1280)):
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(1, 3, H, W, generator=g) * 0.6).half().to(dev)
        canvas = torch.nn.functional.avg_pool2d(torch.randint(0, 256, (3, H + 16, W + 16), generator=g).float()[None], 3, 1, 1)[0].round()
        src0, src1 = ((canvas[:, 8 + oy:8 + oy + H, 8 + ox:8 + ox + W] / 127.5 - 1.0).half().to(dev)[None].contiguous()
                      for oy, ox in ((0, 0), (-3, 2)))
        depth = (torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
        mplane = torch.rand(H, W, generator=g).to(dev)
        u8 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
        st = HipSteady(H, W, device=dev)
        st.steady(x, src0, dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False), init=True)      # (a state for op 48)
        (prev_out, sbytes), (out, snext) = st.records[st._cur], st.records[1 - st._cur]
        hd = HipMatteHold(H, W, device=dev)
        (pp, pb), (op_, nb) = hd.records
        field = torch.zeros((H + 7) // 8, W // 8, 2, dtype=torch.int8, device=dev)
        common = dict(H=H, W=W, lo32=lo32, inv32=inv32, s32=0.8, hard=hard)
        ramp = dict(ramp_lo32=rlo, ramp_inv32=rinv, ramp_hard=rhard)
        ops.run(ops.frame_matte_hold(src0[0], depth, None, None, pp, pb, r=2, init=True, **ramp, **common))      # (a state for op 57)

        def timed(name, *ops_):
            pl = _lib.OpList()
            for op in ops_:
                pl.append(op[0], *op[1])
            pl.time_ms(20)
            us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
            say(args.out, f"{H}x{W} {name:44s}: {min(us):7.2f} us (3 runs: {', '.join(f'{u:.2f}' for u in us)})")
            return min(us)

        hold = lambda r, **kw: ops.frame_matte_hold(src1[0], kw.pop("depth", depth), pp, pb, op_, nb, r=r, **kw, **common)
        matte = timed("op 43 matte, feather 2 (17 B / pixel)", ops.frame_matte(x, src1, depth[None], u8, B=1, H=H, W=W, lo32=rlo, inv32=rinv,
                                                                               hard=rhard, r=2))
        base = timed("op 48 steady, r = 2 (30 B / pixel)", ops.frame_steady(x, src1, prev_out, sbytes, out, snext, r=2, **common))
        mine = timed("op 57 hold, depth, r = 2 (22 B / pixel)", hold(2, **ramp))
        timed("op 57 hold, plane, r = 2 (24 B / pixel)", hold(2, depth=None, plane=mplane))
        for r in (0, 8):
            timed(f"op 57 hold, depth, r = {r}", hold(r, **ramp))
        timed("op 57 hold, depth, init", hold(2, init=True, **ramp))
        motion = ops.frame_motion(src1[0], pb, field, H=H, W=W, search=4, bias=256)
        timed("op 55 motion alone, search = 4", motion)
        timed("op 57 hold, depth, follow alone (field as is)", hold(2, field=field, **ramp))
        both = timed("ops 55 + 57, search = 4", motion, hold(2, field=field, **ramp))
        say(args.out, f"{H}x{W} op 57 against op 48: {mine / base:.2f} x ({mine - base:+.2f} us); against op 43: {mine / matte:.2f} x; "
                      f"ops 55 + 57 against op 57: {both - mine:+.2f} us")


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
    from types import SimpleNamespace
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

    def wrapper(hold):
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type="u8", seed=3, device=dev, **kw)
        w.set_matte(0.3, 0.7, keep="far", feather=2)
        if hold:
            w.set_matte_hold(search=args.search)
        w.prepare(warm, "a cat")
        return w

    stacks = [("off1 matte, hold off", wrapper(False)), (f"on   matte, hold on (search {args.search})", wrapper(True)),
              ("off2 matte, hold off, the same route again", wrapper(False))]
    t = {name: [] for name, _ in stacks}
    for i in range(args.warmup + args.frames):
        for name, fn in stacks:
            t0 = time.perf_counter()
            o = fn(frames[i % 4])
            dt = time.perf_counter() - t0
            assert o.shape == (H, W, 3) and o.dtype == np.uint8
            if i >= args.warmup:
                t[name].append(dt * 1e3)
    say(args.out, f"# matte_hold_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, {args.frames} frames per "
                  f"stack after {args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 frame -> host uint8 frame")
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
    ap.add_argument("--search", type=int, default=0, help="with `route`: the hold's search range (0: the same coordinates)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernels": kernels, "route": route}[args.part](args)


if __name__ == "__main__":
    main()
