"""Device time of the CLIP text encoder (HipClipTextEncoder, SD-1.x size, random weights) -> one JSON line.

  * per encode: hipEvent pair around each replay (the hipGraph of the static plan), median of 60 after 10 warm-ups, for B = 1 / 2 and
    clip_skip None / 2; launches per encode; layer-weight bytes over the time (GB/s);
  * the same encode through the fp32 torch restatement (tests/clip_ref.py) on the same GPU, as the comparison point;
  * per-launch split of the B = 1 plan (l2d_time_each) summed by op kind;
  * prompt-update latency on the host clock: tokenize + encode + synchronise (HipPromptEncoder._encode_prompt, the call
    update_prompt makes), with the synthetic test vocabulary (tests/golden/clip_tok).
`--once`: one encode per configuration and nothing else (for a kernel trace).
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from live2diff_amd import _lib  # noqa: E402
from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, HipPromptEncoder, clip_launches, random_clip_text_state_dict  # noqa: E402
from live2diff_amd.clip_tokenizer import ClipTokenizer  # noqa: E402

DEV = "cuda"


def events_ms(fn, warm=10, reps=60):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    once = "--once" in sys.argv
    sd = random_clip_text_state_dict(SD15_CLIP, 0)
    enc = HipClipTextEncoder({k: v.half() for k, v in sd.items()}, DEV)
    g = torch.Generator().manual_seed(0)
    ids = {B: torch.randint(0, 49406, (B, 77), generator=g).to(DEV) for B in (1, 2)}
    if once:
        for B in (1, 2):
            for k in (None, 2):
                enc.encode(ids[B], k)
        torch.cuda.synchronize()
        print(json.dumps({"once": True}))
        return
    res = {"device": _lib.device_name(), "layer_weight_MB": round(enc.layer_weight_bytes / 2**20, 1), "encode": {}}
    for B in (1, 2):
        for k in (None, 2):
            st = enc.plan(B, k)
            enc.run_plan(st, ids[B])
            ms = events_ms(lambda: st.graph.launch())
            layers = 12 - (k or 0)
            res["encode"][f"B{B}_skip{k}"] = {"ms": round(ms, 4), "launches": len(st.pl), "target_launches": clip_launches(SD15_CLIP, k),
                                              "weight_GBps": round(enc.layer_weight_bytes * layers / 12 / ms / 1e6, 1)}
    from clip_ref import clip_text_forward
    sd_dev = {k: v.to(DEV) for k, v in sd.items()}
    with torch.no_grad():
        for B in (1, 2):
            res["encode"][f"B{B}_skipNone"]["torch_fp32_ms"] = round(events_ms(lambda: clip_text_forward(sd_dev, SD15_CLIP, ids[B]),
                                                                              warm=3, reps=20), 4)
    st = enc.plan(1, None)
    each = st.pl.time_each_us(reps=20)
    names = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    fam = {}
    for op, us in zip(st.pl._ops, each):
        key = names.get(op.kind, str(op.kind)) + ("" if op.kind != _lib.OP_CLIP_LINEAR else f"_K{op.i[1]}_N{op.i[2]}")
        fam.setdefault(key, [0, 0.0])
        fam[key][0] += 1
        fam[key][1] += us
    res["B1_launch_split_us"] = {k: [n, round(us, 1)] for k, (n, us) in sorted(fam.items(), key=lambda kv: -kv[1][1])}
    tok = ClipTokenizer.from_dir(os.path.join(ROOT, "tests", "golden", "clip_tok"))
    pe = HipPromptEncoder(enc, tok, default_clip_skip=2)
    lat = []
    for i in range(30):
        t0 = time.perf_counter()
        pe._encode_prompt(prompt=f"origami style, paper folding, colorful {i}", device=DEV, num_videos_per_prompt=1,
                          do_classifier_free_guidance=False)
        torch.cuda.synchronize()
        lat.append(1e3 * (time.perf_counter() - t0))
    res["prompt_update_host_ms"] = round(statistics.median(lat[5:]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
