"""Timing of the matte at the output size (csrc/matte.hip, csrc/resize.hip, live2diff_amd/matte.py) on the
MI355X: stream 512x512, camera 1080x1920, output 1088x1088 Lanczos.

    timeout -k 10 120 python tools/matte_up_time.py kernels --out profiles/matte_up_time.txt && \\
    timeout -k 10 900 python tools/matte_up_time.py route --out profiles/matte_up_time.txt

  kernels  device events around `--reps` back-to-back replays after a warm-up (microseconds per launch): the camera resample at
           ingest (L2D_OP_FRAME_RESIZE, the 1080x1080 window of the 1080x1920 frame through its row pitch), the output pair of
           `matte_source="camera"` (L2D_OP_FRAME_RESIZE from the fp16 frame + L2D_OP_FRAME_MATTE_UP) and the output pair of
           `matte_source="stream"` (L2D_OP_FRAME_MATTE + L2D_OP_FRAME_RESIZE from its uint8 frame), feather 0, 2 and 8.
  route    on ONE wrapper at full size (SD-1.5 widths, 512x512, 4 denoising steps, synthetic weights as bench.py builds them),
           matte 0.3..0.7 feather 2, for "u8" and for "jpeg": the output route alone (the last fp16 frame on the device -> the host
           frame or file) and the whole call (host 1080x1920 uint8 frame -> host frame or file), wall clock, medians over
           `--frames` calls, in three blocks: "stream", "camera", "stream" again -- "stream" is the route as it was before there
           was a matte source, and stream against stream is the run-to-run spread of one route against itself."""
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

H = W = 512
HS, WS = 1080, 1920
HO = WO = 1088


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def kernels(args):
    from live2diff_amd import _lib, ops
    from live2diff_amd.matte import matte_params, table_words
    from live2diff_amd.resize import axis_table, camera_box
    dev = "cuda"
    say(args.out, f"# matte_up_time kernels: {_lib.device_name()}, stream {H}x{W}, camera {HS}x{WS}, output {HO}x{WO} lanczos, {args.reps} "
                  "back-to-back replays per figure (device events)")
    g = torch.Generator().manual_seed(0)
    styled, source = ((torch.randn(1, 3, H, W, generator=g) * 0.7).half().to(dev) for _ in range(2))
    depth = (torch.randn(1, H, W, generator=g) * 0.6).clamp(-1, 1).half().to(dev)
    camera = torch.randint(0, 256, (1, HS, WS, 3), dtype=torch.uint8, generator=g).to(dev)
    y0, x0, bh, bw = camera_box(HS, WS, H, W)

    def timed(*made):
        pl = _lib.OpList()
        for op, keep in made:
            pl.append(op, *keep)
        pl.time_ms(20)
        us = [pl.time_ms(args.reps) * 1e3 for _ in range(3)]
        return f"{min(us):6.2f} us (3 runs: {', '.join(f'{v:.2f}' for v in us)})"

    cam_out, sty_out, dst = (torch.empty(1, HO, WO, 3, dtype=torch.uint8, device=dev) for _ in range(3))
    u8 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
    ctx, cty = (torch.from_numpy(axis_table(i, o, "lanczos")).to(dev) for i, o in ((bw, WO), (bh, HO)))
    tx, ty = (torch.from_numpy(axis_table(i, o, "lanczos")).to(dev) for i, o in ((W, WO), (H, HO)))
    ux, uy = (torch.from_numpy(table_words(i, o)).to(dev) for i, o in ((W, WO), (H, HO)))
    window = camera.reshape(-1)[(y0 * WS + x0) * 3:]
    ingest = ops.frame_resize(window, cam_out, ctx, cty, B=1, H=bh, W=bw, Ho=HO, Wo=WO, src_pitch=WS)
    say(args.out, f"ingest  op 46, window ({y0}, {x0}, {bh}, {bw}) of the camera frame -> {HO}x{WO}: {timed(ingest)}")
    lo32, inv32, hard = matte_params(0.3, 0.7)
    kw = dict(lo32=lo32, inv32=inv32, hard=hard)
    say(args.out, f"        op 46, fp16 {H}x{W} -> {HO}x{WO} alone                        : "
                  f"{timed(ops.frame_resize(styled, sty_out, tx, ty, B=1, H=H, W=W, Ho=HO, Wo=WO))}")
    for r in (0, 2, 8):
        up = ops.frame_matte_up(sty_out, cam_out, depth, dst, ux, uy, B=1, H=H, W=W, Ho=HO, Wo=WO, r=r, **kw)
        say(args.out, f"        op 47 alone, feather {r}                                      : {timed(up)}")
        say(args.out, f"output  camera: op 46 (fp16 -> {HO}x{WO}) + op 47, feather {r}        : "
                      f"{timed(ops.frame_resize(styled, sty_out, tx, ty, B=1, H=H, W=W, Ho=HO, Wo=WO), up)}")
        say(args.out, f"output  stream: op 43 ({H}x{W}) + op 46 (uint8 -> {HO}x{WO}), feather {r}: "
                      f"{timed(ops.frame_matte(styled, source, depth, u8, B=1, H=H, W=W, r=r, **kw), ops.frame_resize(u8, dst, tx, ty, B=1, H=H, W=W, Ho=HO, Wo=WO))}")


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
    dev, N = "cuda", 4
    cfg = sd15_config()
    tok = ClipTokenizer.from_dir(os.path.join(ROOT, "tests", "golden", "clip_tok"))
    penc = HipPromptEncoder(HipClipTextEncoder(random_clip_text_state_dict(SD15_CLIP, 3), dev, SD15_CLIP), tok, default_clip_skip=1)
    pipe = SimpleNamespace(device=torch.device(dev), vae_scale_factor=8, scheduler=None, _encode_prompt=penc._encode_prompt,
                           unet=HipStreamingUNet(device_random_state_dict(cfg, dev), cfg, H // 8, W // 8, N, device=dev),
                           vae=HipTinyVAE(random_taesd_state_dict(device=dev), device=dev),
                           depth_model=HipMidas(random_midas_state_dict(device=dev), device=dev))
    g = torch.Generator().manual_seed(1)
    warm = torch.randint(0, 256, (8, HS, WS, 3), dtype=torch.uint8, generator=g).numpy()
    frames = torch.randint(0, 256, (4, HS, WS, 3), dtype=torch.uint8, generator=g).numpy()
    w = StreamAnimateDiffusionDepthWrapper.from_components(pipe, output_type="u8", seed=3, device=dev, num_inference_steps=50,
                                                           t_index_list=[25, 31, 37, 43], width=W, height=H,
                                                           warmup_frames=cfg.sink_size, window_size=cfg.window_size)
    w.set_matte(0.3, 0.7, feather=2)
    w.set_output_size(HO, WO)
    w.prepare(warm, "a cat")
    say(args.out, f"# matte_up_time route: {_lib.device_name()}, SD-1.5 widths, {H}x{W}, {N} denoising steps, one wrapper; camera {HS}x{WS}, "
                  f"matte 0.3..0.7 feather 2, output size {HO}x{WO} lanczos; medians over {args.frames} calls per block after {args.warmup} "
                  "warm-up; blocks stream, camera, stream; wall clock")

    def med(tag, v):
        v = sorted(v)
        m = statistics.median(v)
        say(args.out, f"{tag}: median {m:.3f} ms, p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f}, min {v[0]:.3f}")
        return m

    for ot in ("u8", "jpeg"):
        w.output_type = ot
        whole, alone = {}, {}
        for name, source in (("stream1", "stream"), ("camera ", "camera"), ("stream2", "stream")):
            w.set_matte_source(source)
            t = []
            for i in range(args.warmup + args.frames):
                t0 = time.perf_counter()
                o = w(frames[i % 4])
                dt = time.perf_counter() - t0
                assert o.shape == (HO, WO, 3) if ot == "u8" else o[:2] == b"\xff\xd8"
                if i >= args.warmup:
                    t.append(dt * 1e3)
            assert (w._matte_line.last.camera is not None) == (source == "camera")
            whole[name] = med(f"{ot:4s} whole call   {name}", t)
            # the output route alone, on the frame the stream made last and the slot it was paired with
            x, slot = w.stream.prev_image_result, w._matte_line.last
            t = []
            for i in range(args.warmup + args.frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = w._finish(x, slot)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    t.append(dt * 1e3)
            alone[name] = med(f"{ot:4s} output route {name}", t)
        for tag, m in (("whole call  ", whole), ("output route", alone)):
            say(args.out, f"{ot:4s} {tag} camera - mean(stream1, stream2) = {m['camera '] - (m['stream1'] + m['stream2']) / 2:+.3f} ms; "
                          f"|stream1 - stream2| = {abs(m['stream1'] - m['stream2']):.3f} ms")
    w.set_matte_source("stream")


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
