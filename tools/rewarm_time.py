"""Timing of the re-warm (live2diff_amd/pipeline_stream_animation_depth.py `rewarm`, csrc/sink_commit.hip) on the MI355X.

    timeout -k 10 900 python tools/rewarm_time.py --out profiles/rewarm_time.txt

SD-1.5 widths at cfg-2 (512 x 512 frames, 64 x 64 latent, 2 denoising steps, L = 16, F = 8), synthetic weights, the pipeline class
with the tiny VAE, the depth detector and the device step, `keep_recent=True`:

  loop     the row loop of `prepare` (N warm-up passes over F frames, the LCM step and the re-noise between them) on the shadow caches;
  rewarm   `rewarm()` on the warm-up window and `rewarm(*recent_window())` on the recent one: that loop plus the commit -- wall clock
           (a host clock around the call and a synchronise) and device time (events around the call);
  commit   L2D_OP_SINK_COMMIT, one launch over all layers, against the same bytes moved by one strided `copy_` per layer, and
           against bytes / 6.5 TB/s (bytes = the sink part read once and written once);
  frame    the frame that follows a re-warm against the stream's steady frame (events around `__call__`).

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

HBM_TBS = 6.5


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


def stat(v):
    return f"min {min(v):.3f} ms, median {statistics.median(v):.3f} ms"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="back-to-back replays per figure of the commit and of the copies")
    ap.add_argument("--tiny", action="store_true", help="the tiny test configuration at 64 x 64 (a rehearsal of the tool)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib, ops
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
                                    warmup_frames=F_, window_size=L, keep_recent=True)
    s.image_processor.assume_unit_range = True
    g = torch.Generator().manual_seed(4321)
    s.prepare_cache(H, W, N)
    s.prepare([torch.rand(3, H, W, generator=g) for _ in range(F_)], prompt_embeds=torch.randn(1, 77, cfg.cross_attention_dim, generator=g), seed=3)
    s.enable_device_step()
    frames = [torch.rand(1, 3, H, W, generator=g).to(dev) for _ in range(4)]
    for i in range(F_ + 4):
        s(frames[i % 4])
    live = s.kv_cache_list
    cache_bytes = sum(c.numel() * c.element_size() for c in live)
    sink_bytes = cache_bytes * F_ // L
    say(args.out, f"# rewarm_time: {_lib.device_name()}, {'tiny' if args.tiny else 'SD-1.5'} widths, {H}x{W} frames, N = {N}, L = {L}, F = {F_}: "
                  f"{len(live)} KV caches, {cache_bytes / 1e9:.3f} GB live + the same again for the shadows; the sink part is "
                  f"{sink_bytes / 1e9:.3f} GB; {args.rounds} rounds, variants alternating")

    # ---- the row loop, rewarm("warmup"), rewarm("recent")
    s.rewarm()                                                     # (makes the shadows and the commit's table; warms the warm-up plan)
    s.rewarm(*s.recent_window())
    x, d = s.warmup_window
    noise = lambda t: torch.randn(t.shape, generator=gen, device=t.device, dtype=t.dtype)
    t = {k: [] for k in ("loop", "warmup", "recent")}
    for _ in range(args.rounds):
        gen = s.rewarm_generator()
        t["loop"].append(timed(lambda: s._warm_rows(x, d, s._shadow, noise)))
        t["warmup"].append(timed(s.rewarm))
        t["recent"].append(timed(lambda: s.rewarm(*s.recent_window())))
    names = {"loop": "row loop of prepare (on the shadows)", "warmup": 'rewarm("warmup")', "recent": 'rewarm("recent")'}
    for k, v in t.items():
        say(args.out, f"  {names[k]:>38s}: device {stat([a for a, _ in v])}; wall {stat([b for _, b in v])}")

    # ---- the commit alone, against per-layer strided copies
    hit = s._commit
    op = ops.sink_commit(hit[0], hit[1])
    commit = lambda: ops.run(op)

    def copies():
        for c, sh in zip(live, s._shadow):
            c[:, :, :, :F_].copy_(sh[:, :, :, :F_])
    for fn in (commit, copies):
        for _ in range(3):
            fn()
    tc = {"op": [], "copy_": []}
    for _ in range(args.rounds):
        tc["op"].append(timed(commit, args.reps)[0])
        tc["copy_"].append(timed(copies, args.reps)[0])
    floor = 2 * sink_bytes / (HBM_TBS * 1e12) * 1e3
    say(args.out, f"commit, {2 * sink_bytes / 1e9:.3f} GB moved (read + write), {len(hit[1])} records; bytes / {HBM_TBS} TB/s = {floor:.3f} ms:")
    for k, label in (("op", "L2D_OP_SINK_COMMIT, one launch"), ("copy_", f"{len(live)} strided copy_ calls")):
        lo = min(tc[k])
        say(args.out, f"  {label:>38s}: device {stat(tc[k])}; {2 * sink_bytes / lo / 1e9:.2f} TB/s at the minimum = "
                      f"{100 * floor / lo:.0f} % of {HBM_TBS} TB/s")
    say(args.out, f"  one launch vs the copy_ loop: {min(tc['copy_']) / min(tc['op']):.2f}x")

    # ---- the frame behind a re-warm, against the steady frame
    steady, after = [], []
    for r in range(args.rounds):
        for i in range(3):
            s(frames[i % 4])
        steady.append(timed(lambda: s(frames[3]))[0])
        s.rewarm()
        after.append(timed(lambda: s(frames[0]))[0])
    say(args.out, f"frame (events around __call__): steady {stat(steady)}; the frame behind a re-warm {stat(after)}")
    say(args.out, f"re-warms done: {s.rewarms}; finite: {bool(torch.isfinite(s.prev_image_result).all())}")


if __name__ == "__main__":
    main()
