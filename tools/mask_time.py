"""Timing of the matte from the caller (csrc/mask_in.hip, live2diff_amd/mask_io.py) on the MI355X.

    timeout -k 10 120 python tools/mask_time.py kernels --out profiles/mask_time.txt && \\
    timeout -k 10 120 python tools/mask_time.py planes --out profiles/mask_time.txt && \\
    timeout -k 10 900 python tools/mask_time.py route --out profiles/mask_time.txt

  kernels  L2D_OP_MASK_INGEST to 512x512 from a 512x512 uint8 mask, a 1280x720 uint8 mask and a 1280x720 float32 mask ("replace",
           and "and" for the first), beside L2D_OP_DEPTH_INGEST at the same geometries (uint16 for the byte cases: it has no
           uint8 form) in the same run: device events around `--reps` back-to-back replays after a warm-up, the median of five
           runs (microseconds per launch).  Op 52 resamples two planes where op 58 resamples one.
  planes   L2D_OP_FRAME_MATTE_EDGE (r = 4) and L2D_OP_FRAME_BACKDROP_BLUR (r = 6, 3 passes) at 512x512 with the depth plane
           (flag clear) and, where the library has the flag, with the fp32 plane.  Run it once more with L2D_LIB naming the
           parent commit's library for the parent's flag-clear figure on the same box.
  route    host uint8 frame -> host uint8 frame through the wrapper's "u8" output at full size (SD-1.5 widths, 512x512, 4
           denoising steps, synthetic weights as bench.py builds them) under a matte, wall clock per frame, three stacks
           alternating frame by frame in one process: no mask, a 1280x720 uint8 host mask per frame, and no mask again -- off
           against off is the run-to-run spread of one route against itself."""
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


def _timed(out, reps, name, *ops_):
    from live2diff_amd import _lib
    pl = _lib.OpList()
    for op in ops_:
        pl.append(op[0], *op[1])
    pl.time_ms(20)
    us = sorted(pl.time_ms(reps) * 1e3 for _ in range(5))
    say(out, f"{name:58s}: median {statistics.median(us):7.2f} us (5 runs: {', '.join(f'{u:.2f}' for u in us)})")
    return statistics.median(us)


def kernels(args):
    from live2diff_amd import _lib, depth_io, mask_io, ops
    from live2diff_amd.matte import matte_params
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# mask_time kernels: {_lib.device_name()}, {args.reps} back-to-back replays per figure (device events), median of 5 runs")
    g = torch.Generator().manual_seed(0)
    depth = (torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    plane = torch.empty(H, W, dtype=torch.float32, device=dev)
    R = torch.empty(1, H, W, dtype=torch.float32, device=dev)
    partials = torch.empty(ops.depth_tiles(H, W), 3, dtype=torch.float32, device=dev)
    lo32, inv32, hard = matte_params(0.3, 0.7)
    for (Hm, Wm), dtype in (((512, 512), torch.uint8), ((720, 1280), torch.uint8), ((720, 1280), torch.float32)):
        (nh, nw, top, left), ymin, wy, xmin, wx = mask_io.tables(Hm, Wm, H, W)
        tabs = tuple(t.to(dev) for t in (xmin, wx, ymin, wy))
        geo = dict(H=H, W=W, nh=nh, nw=nw, top=top, left=left)
        if dtype == torch.float32:
            m, z = torch.rand(Hm, Wm, generator=g).to(dev), (torch.rand(1, Hm, Wm, generator=g) * 4 + 0.5).to(dev)
        else:
            m = torch.randint(0, 256, (Hm, Wm), generator=g, dtype=torch.uint8).to(dev)
            z = torch.randint(300, 5000, (1, Hm, Wm), generator=g, dtype=torch.int16).to(dev)      # (op 52 has no uint8 form: uint16)
        tag = f"{Wm}x{Hm} {'fp32' if dtype == torch.float32 else 'uint8'} -> {W}x{H}"
        mine = _timed(args.out, args.reps, f"op 58 mask ingest, replace, {tag}", ops.mask_ingest(m, plane, None, *tabs, Hm=Hm, Wm=Wm, **geo))
        if (Hm, Wm) == (512, 512):
            _timed(args.out, args.reps, f"op 58 mask ingest, and, {tag}",
                   ops.mask_ingest(m, plane, depth, *tabs, Hm=Hm, Wm=Wm, combine="and", lo32=lo32, inv32=inv32, hard=hard, **geo))
        base = _timed(args.out, args.reps, f"op 52 depth ingest, {'fp32' if dtype == torch.float32 else 'uint16'}, same geometry",
                      ops.depth_ingest(z, R, partials, *tabs, B=1, Hd=Hm, Wd=Wm, distance=True, invalid=0, **geo))
        say(args.out, f"{tag}: op 58 against op 52: {mine / base:.2f} x ({mine - base:+.2f} us)")
    assert depth_io.tables(720, 1280, H, W)[0] == mask_io.tables(720, 1280, H, W)[0]


def planes(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import edge_E, matte_params
    dev, H, W = "cuda", 512, 512
    say(args.out, f"# mask_time planes: {_lib.device_name()}, library {os.path.relpath(_lib.LIB_PATH, ROOT)}, {args.reps} back-to-back replays "
                  f"per figure (device events), median of 5 runs, 512x512")
    g = torch.Generator().manual_seed(0)
    src = (torch.randn(3, H, W, generator=g) * 0.6).half().to(dev)
    depth = (torch.randn(H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    mplane = (torch.randint(0, 256, (H, W), generator=g).float() / 255.0).to(dev)
    out32 = torch.empty(H, W, dtype=torch.float32, device=dev)
    out16 = torch.empty(3, H, W, dtype=torch.float16, device=dev)
    lo32, inv32, hard = matte_params(0.3, 0.7)
    ramp = dict(lo32=lo32, inv32=inv32, hard=hard)
    has_flag = hasattr(_lib, "OP_MASK_INGEST") and not args.flag_clear_only
    e0 = _timed(args.out, args.reps, "op 49 matte edge, r = 4, depth plane (flag clear)",
                ops.frame_matte_edge(src, depth, out32, H=H, W=W, r=4, E=edge_E(4, 10.0), **ramp))
    b0 = _timed(args.out, args.reps, "op 54 backdrop blur, r = 6, 3 passes, depth plane (flag clear)",
                ops.frame_backdrop_blur(src, depth, out16, H=H, W=W, r=6, passes=3, **ramp))
    if has_flag:
        e1 = _timed(args.out, args.reps, "op 49 matte edge, r = 4, fp32 plane (flag set)",
                    ops.frame_matte_edge(src, None, out32, H=H, W=W, r=4, E=edge_E(4, 10.0), plane=mplane))
        b1 = _timed(args.out, args.reps, "op 54 backdrop blur, r = 6, 3 passes, fp32 plane (flag set)",
                    ops.frame_backdrop_blur(src, None, out16, H=H, W=W, r=6, passes=3, plane=mplane))
        say(args.out, f"flag set against flag clear: op 49 {e1 - e0:+.2f} us, op 54 {b1 - b0:+.2f} us")


def route(args):
    from types import SimpleNamespace

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
    masks = [(torch.rand(720, 1280, generator=g) < 0.5).to(torch.uint8).mul(255).numpy() for _ in range(4)]

    def wrapper():
        w = StreamAnimateDiffusionDepthWrapper.from_components(pipe(), output_type="u8", seed=3, device=dev, **kw)
        w.set_matte(0.3, 0.7, keep="far", feather=2)
        w.prepare(warm, "a cat")
        return w

    stacks = [("off1 matte, no mask (the ramp alone)", wrapper(), False), ("on   matte, a 1280x720 uint8 host mask per frame", wrapper(), True),
              ("off2 matte, no mask, the same route again", wrapper(), False)]
    t = {name: [] for name, _, _ in stacks}
    for i in range(args.warmup + args.frames):
        for name, fn, masked in stacks:
            t0 = time.perf_counter()
            o = fn(frames[i % 4], mask=masks[i % 4]) if masked else fn(frames[i % 4])
            dt = time.perf_counter() - t0
            assert o.shape == (H, W, 3) and o.dtype == np.uint8
            if i >= args.warmup:
                t[name].append(dt * 1e3)
    say(args.out, f"# mask_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, {args.frames} frames per "
                  f"stack after {args.warmup} warm-up, stacks alternating frame by frame; wall clock host uint8 frame -> host uint8 frame")
    med = {}
    for name, _, _ in stacks:
        v = sorted(t[name])
        med[name[:4]] = statistics.median(v)
        say(args.out, f"{name}: median {statistics.median(v):.3f} ms ({1e3 / statistics.median(v):.2f} frames/s), p10 {v[len(v) // 10]:.3f}, "
                      f"p90 {v[len(v) * 9 // 10]:.3f}, min {v[0]:.3f}, max {v[-1]:.3f}")
    off = (med["off1"] + med["off2"]) / 2
    say(args.out, f"on - mean(off1, off2) = {med['on  '] - off:+.3f} ms; |off1 - off2| (one route against itself) = "
                  f"{abs(med['off1'] - med['off2']):.3f} ms; mask buffers allocated: {stacks[1][1]._mask_tap.allocated}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("part", choices=["kernels", "planes", "route"])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--flag-clear-only", action="store_true", help="with `planes`: only the depth-plane forms (a library without the flags)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernels": kernels, "planes": planes, "route": route}[args.part](args)


if __name__ == "__main__":
    main()
