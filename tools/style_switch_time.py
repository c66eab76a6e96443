"""Timing of the style switch / style blend (csrc/wblend.hip, live2diff_amd/style_bank.py) on the MI355X.

    timeout -k 10 600 python tools/style_switch_time.py --out profiles/style_switch_time.txt

SD-1.5 widths at cfg-2 (64 x 64 latent, 2 denoising steps), synthetic weights.  For K = 1 (switch), 2 and 3 (blends) sources:

  op      L2D_OP_WEIGHT_BLEND, one launch over the whole packed set, with plain and with non-temporal loads / stores;
  torch   the same work as the per-tensor torch loop on the same tensors -- K = 1 `copy_`; K = 2 `copy_` + `lerp_`; K >= 2 also
          `copy_` + `mul_` + `add_(alpha=)` per further source; and for K = 2 the single-pass `torch.lerp(out=)`.

Device events around `--reps` back-to-back replays, after a warm-up; the variants alternate within a round, `--rounds` rounds, the
minimum and the median over rounds are reported.  Bytes moved = (K + 1) x the set's bytes (K reads, one write); the rate is
stated as a fraction of the 6.29 TB/s a float4 copy reaches on this part.  Then a UNet frame step directly after a switch (the
conditioning launches re-run) next to the steady-state step."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_PEAK_TBS = 6.29


def say(out, line):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps):
    """milliseconds per call: device events around `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_loop(dst, srcs, w):
    K = len(srcs)
    if K == 1:
        def run():
            for k, d in dst.items():
                d.copy_(srcs[0][k])
    elif K == 2:
        def run():
            for k, d in dst.items():
                d.copy_(srcs[0][k])
                d.lerp_(srcs[1][k], w[1])
    else:
        def run():
            for k, d in dst.items():
                d.copy_(srcs[0][k])
                d.mul_(w[0])
                for j in range(1, K):
                    d.add_(srcs[j][k], alpha=w[j])
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the tiny test configuration instead of SD-1.5 widths (a rehearsal of the tool)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from live2diff_amd import _lib
    from live2diff_amd.config import sd15_config, tiny_config
    from live2diff_amd.style_bank import WeightBlender, clone_set
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import device_random_state_dict
    dev, h, w, N = "cuda", (8 if args.tiny else 64), (8 if args.tiny else 64), 2
    cfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=192) if args.tiny else sd15_config()
    unet = HipStreamingUNet(device_random_state_dict(cfg, dev), cfg, h, w, N, device=dev)
    sets = [clone_set(unet.packed_state()) for _ in range(3)]
    srcs = [s.W for s in sets]
    nbytes = unet.weight_bytes()
    wb = WeightBlender(unet.W, dev)
    say(args.out, f"# style_switch_time: {_lib.device_name()}, {'tiny' if args.tiny else 'SD-1.5'} widths, {h}x{w} latent, N = {N}: "
                  f"{len(unet.W)} tensors, {nbytes / 1e9:.3f} GB per set ({min(t.numel() * t.element_size() for t in unet.W.values())} B .. "
                  f"{max(t.numel() * t.element_size() for t in unet.W.values()) / 1e6:.1f} MB); {args.reps} replays per figure, "
                  f"{args.rounds} rounds, variants alternating (device events)")
    mixes = {1: [1.0], 2: [0.5, 0.5], 3: [0.25, 0.25, 0.5]}
    best = {}
    for K, mix in mixes.items():
        variants = [("op plain", lambda K=K, mix=mix: wb.apply(srcs[:K], mix, nt=0)),
                    ("op non-temporal", lambda K=K, mix=mix: wb.apply(srcs[:K], mix, nt=1)),
                    ("torch loop", torch_loop(unet.W, srcs[:K], mix))]
        if K == 2:
            variants.append(("torch lerp(out=)", lambda mix=mix: [torch.lerp(srcs[0][k], srcs[1][k], mix[1], out=d) for k, d in unet.W.items()]))
        n_rec = len(wb._table(srcs[:K])[1])
        for _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                t[name].append(timed(fn, args.reps))
        moved = (K + 1) * nbytes
        say(args.out, f"K = {K} ({n_rec} records, {moved / 1e9:.2f} GB moved):")
        for name, _ in variants:
            lo, med = min(t[name]), statistics.median(t[name])
            best[(K, name)] = lo
            say(args.out, f"  {name:>18s}: min {lo:.3f} ms, median {med:.3f} ms; {moved / lo / 1e9:.2f} TB/s at the minimum = "
                          f"{100 * moved / lo / 1e9 / COPY_PEAK_TBS:.0f} % of {COPY_PEAK_TBS} TB/s")
    for K in mixes:
        op = min(best[(K, "op plain")], best[(K, "op non-temporal")])
        say(args.out, f"K = {K}: one launch {op:.3f} ms vs torch loop {best[(K, 'torch loop')]:.3f} ms = {best[(K, 'torch loop')] / op:.2f}x")

    # a frame step directly after a switch (conditioning re-run) next to the steady-state step
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float16)
    from live2diff_amd.pipeline_stream_animation_depth import ring_buffer_init
    rb = ring_buffer_init(N, cfg.window_size, cfg.sink_size)
    kv = unet.prepare_cache(N)
    for c in kv:
        c.normal_(generator=g)
    kw = dict(encoder_hidden_states=rn(N, 77, cfg.cross_attention_dim), temporal_attention_mask=rb[0].half().to(dev),
              depth_sample=rn(N, 4, 1, h, w), kv_cache=kv, pe_idx=rb[1].to(dev), update_idx=rb[2].to(dev))
    x, ts = rn(N, 4, 1, h, w), torch.tensor([399, 199][:N], device=dev)
    step = lambda: unet(x, ts, **kw)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    steady, after, both = [], [], []
    for _ in range(args.rounds):
        steady.append(timed(step, args.reps))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        a_ms = b_ms = 0.0
        for _ in range(args.reps):
            ev[0].record()
            unet.load_mix([sets[1]], [1.0])
            ev[1].record()
            step()
            ev[2].record()
            ev[2].synchronize()
            a_ms += ev[1].elapsed_time(ev[2]) / args.reps
            b_ms += ev[0].elapsed_time(ev[2]) / args.reps
        after.append(a_ms)
        both.append(b_ms)
    say(args.out, f"UNet step (boundary call, {len(unet._plans['stream'].cond_pl)} conditioning launches re-run after a switch): steady "
                  f"{min(steady):.3f} ms (median {statistics.median(steady):.3f}); directly after a switch {min(after):.3f} ms (median "
                  f"{statistics.median(after):.3f}); switch + that step {min(both):.3f} ms (median {statistics.median(both):.3f})")


if __name__ == "__main__":
    main()
