"""Timing of the cut detector (live2diff_amd/cut.py, csrc/cut.hip) on the MI355X.

    timeout -k 10 600 python tools/cut_time.py kernels --out profiles/cut_time.txt
    timeout -k 10 900 python tools/cut_time.py frame --out profiles/cut_time.txt

  kernels  L2D_OP_FRAME_CUT_SIG (op 65) and L2D_OP_FRAME_CUT (op 66) at `--size` (512 x 512), each alone and the two as a frame
           launches them, beside the plate gain's L2D_OP_MATTE_KEY_GAIN_HIST / L2D_OP_MATTE_KEY_GAIN (ops 62 / 63) at the same size:
           the yardstick of DESIGN.md section 8.z19, two launches of the same kind (a histogram per work-group into partials, one
           work-group that sums them).  Device events around `--reps` back-to-back replays of one list (`OpList.time_ms`, as
           tools/matte_key_time.py measures);
  frame    `StreamAnimateDiffusionDepth.__call__` with the detector on against off: SD-1.5 widths at cfg-2 (512 x 512 frames, 2
           denoising steps), synthetic weights, the tiny VAE, the depth detector and the device step; device events around the call,
           and the host clock around the call and its synchronise.

The variants alternate within a round; the minimum and the median over `--rounds` rounds are reported."""
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


def timed(fn, reps=1):
    """(device ms, wall ms) per call: events around `reps` back-to-back calls, a host clock around them and a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, 1e3 * (time.perf_counter() - t0) / reps


def stat(v, unit="ms", scale=1.0):
    return f"min {min(v) * scale:.3f} {unit}, median {statistics.median(v) * scale:.3f} {unit}"


def kernels(args):
    from live2diff_amd import _lib, cut, ops
    dev = "cuda"
    H, W = args.size
    g = torch.Generator().manual_seed(11)
    a, b = ((torch.rand(3, H, W, generator=g) * 2.2 - 1.1).to(torch.float16).to(dev) for _ in range(2))
    det = cut.HipCutDetect(H, W, device=dev)
    det.measure(a)
    det.measure(b)                                       # both states hold a signature now
    torch.cuda.synchronize()
    det.collect()
    prev, nxt = det.states[det._cur], det.states[1 - det._cur]
    Tt, Th, R, gap = det.params
    lists = {}

    def plan(*built):
        pl = _lib.OpList()
        for op, keep in built:
            pl.append(op, *keep)
        return pl

    sig = lambda: ops.frame_cut_sig(a, prev[0], nxt[0], det.partials, H=H, W=W)
    dec = lambda: ops.frame_cut(det.partials, prev, nxt, H=H, W=W, Tt=Tt, Th=Th, R=R, gap=gap)
    lists["op 65 frame_cut_sig"] = plan(sig())
    lists["op 66 frame_cut"] = plan(dec())
    lists["ops 65 + 66, one list"] = plan(sig(), dec())
    plate = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).to(dev)
    nblk = ops.matte_key_gain_blocks(H, W)
    gp = torch.empty(nblk, 3, ops.MATTE_KEY_GAIN_BINS, dtype=torch.int32, device=dev)
    grec = torch.empty(8, dtype=torch.int32, device=dev)
    hist = lambda: ops.matte_key_gain_hist(a, plate, gp, H=H, W=W)
    med = lambda: ops.matte_key_gain(gp, grec, H=H, W=W, lim=256, min_count=H * W // 16)
    lists["op 62 matte_key_gain_hist"] = plan(hist())
    lists["op 63 matte_key_gain"] = plan(med())
    lists["ops 62 + 63, one list"] = plan(hist(), med())
    for pl in lists.values():
        pl.time_ms(20)
    say(args.out, f"# cut_time kernels: {_lib.device_name()}, {H}x{W}: op 65 on {ops.frame_cut_tiles(H, W)} work-groups of 512 lanes, op 66 on one "
                  f"of 256; op 62 on {nblk} work-groups of 512 lanes, op 63 on one of 1,024; {args.reps} back-to-back replays per figure, "
                  f"{args.rounds} rounds, variants alternating")
    t = {k: [] for k in lists}
    for _ in range(args.rounds):
        for k, pl in lists.items():
            t[k].append(pl.time_ms(args.reps))           # (l2d_time_ops: the replays and their events are issued by the library)
    for k, v in t.items():
        say(args.out, f"  {k:>28s}: device {stat(v, 'us', 1e3)} per replay")
    frame_bytes = 6 * H * W
    say(args.out, f"  op 65 reads {frame_bytes / 1e6:.2f} MB: {frame_bytes / (min(t['op 65 frame_cut_sig']) * 1e-3) / 1e12:.2f} TB/s at the minimum "
                  f"(latency-bound on {ops.frame_cut_tiles(H, W)} work-groups, as ops 62 / 63 are)")


def frame(args):
    from live2diff_amd import _lib, cut
    from live2diff_amd.config import sd15_config, tiny_config
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.pipeline_stream_animation_depth import StreamAnimateDiffusionDepth
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.vae_hip import HipTinyVAE, random_taesd_state_dict
    from live2diff_amd.weights import device_random_state_dict
    dev, N = "cuda", 2
    H = W = 64 if args.tiny else 512
    cfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=192) if args.tiny else sd15_config()
    F_, L = cfg.sink_size, cfg.window_size
    unet = HipStreamingUNet(device_random_state_dict(cfg, dev), cfg, H // 8, W // 8, N, device=dev)
    pipe = SimpleNamespace(device=dev, vae_scale_factor=8, unet=unet, vae=HipTinyVAE(random_taesd_state_dict(device=dev), device=dev),
                           depth_model=HipMidas(random_midas_state_dict(device=dev), device=dev), scheduler=None)
    s = StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, do_add_noise=True,
                                    warmup_frames=F_, window_size=L)
    s.image_processor.assume_unit_range = True
    g = torch.Generator().manual_seed(4321)
    s.prepare_cache(H, W, N)
    s.prepare([torch.rand(3, H, W, generator=g) for _ in range(F_)], prompt_embeds=torch.randn(1, 77, cfg.cross_attention_dim, generator=g), seed=3)
    s.enable_device_step()
    frames = [torch.rand(1, 3, H, W, generator=g).to(dev) for _ in range(4)]
    det = cut.HipCutDetect(H, W, device=dev)
    for i in range(8):
        s.cut_detector = det if i % 2 else None
        s(frames[i % 4])
    say(args.out, f"# cut_time frame: {_lib.device_name()}, {'tiny' if args.tiny else 'SD-1.5'} widths, {H}x{W} frames, N = {N}: __call__ with the "
                  f"detector on against off, {args.calls} calls per figure, {args.rounds} rounds, variants alternating")
    t = {"off": [], "on": []}
    k = 0
    for _ in range(args.rounds):
        for name in ("off", "on"):
            s.cut_detector = det if name == "on" else None

            def call():
                nonlocal k
                k += 1
                s(frames[k % 4])
            t[name].append(timed(call, args.calls))
    s.cut_detector = None
    slots = len(det._slots)                                # (a frame's record is collected in its own call: one slot serves)
    # the host's share: `measure` alone, eight calls back to back, then a synchronise and a `collect` outside the clock (the
    # builders' checks run once per frame address)
    xs = [s.image_processor.preprocess(f, H, W).to(device=dev, dtype=s.dtype) for f in frames]      # (what `__call__` hands it)
    for i in range(8):
        det.measure(xs[i % 4])                             # (the eight pinned slots are made here, not under the clock)
    torch.cuda.synchronize()
    det.collect()
    host = 0.0
    for r in range(25):
        t0 = time.perf_counter()
        for i in range(8):
            det.measure(xs[i % 4])
        host += time.perf_counter() - t0
        torch.cuda.synchronize()
        det.collect()
    host_us = 1e6 * host / 200
    for name, v in t.items():
        say(args.out, f"  detector {name:>3s}: device {stat([a for a, _ in v])}; wall {stat([b for _, b in v])} per frame")
    d_dev = (statistics.median([a for a, _ in t["on"]]) - statistics.median([a for a, _ in t["off"]])) * 1e3
    d_wall = (statistics.median([b for _, b in t["on"]]) - statistics.median([b for _, b in t["off"]])) * 1e3
    say(args.out, f"  on - off, medians: device {d_dev:+.1f} us, wall {d_wall:+.1f} us per frame; records collected: {len(s.cut_records)}, "
                  f"pinned slots in the stream: {slots}; host time of measure() alone: {host_us:.1f} us; finite: {bool(torch.isfinite(s.prev_image_result).all())}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=("kernels", "frame"))
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200, help="kernels: back-to-back replays per figure")
    ap.add_argument("--calls", type=int, default=10, help="frame: calls per figure")
    ap.add_argument("--size", type=lambda t: tuple(int(v) for v in t.lower().split("x")), default=(512, 512), metavar="HxW")
    ap.add_argument("--tiny", action="store_true", help="frame: the tiny test configuration at 64 x 64 (a rehearsal of the tool)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    (kernels if args.mode == "kernels" else frame)(args)


if __name__ == "__main__":
    main()
