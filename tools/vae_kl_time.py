"""Device time of the SD AutoencoderKL (HipAutoencoderKL, SD-1.5 configuration, random weights) -> one JSON line.

  * encode / decode per configuration (512^2 B = 1, the 8-frame warm-up batch at 512^2, 384^2, 512x768): hipEvent pair around
    each plan replay, median of 20 after 3 warm-ups; achieved TFLOP/s from FLOPs counted from shapes;
  * per-launch split of the 512^2 B = 1 plans (OpList.time_each_us) summed by op kind;
  * the mid-block attention op alone at B = 1, T = 4096 (and its fraction of the 2.5 PF fp16 MFMA peak);
  * the same encode / decode through the restatement tests/vae_kl_ref.py in fp16 on the same GPU, as the comparison point;
  * the VAE share of a frame (two encodes + one decode at 512^2, what `StreamAnimateDiffusionDepth.__call__` runs) with the full
    VAE and with HipTinyVAE.
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from live2diff_amd import _lib, ops  # noqa: E402
from live2diff_amd.vae_kl_hip import BLOCK_OUT, HipAutoencoderKL, random_vae_kl_state_dict, sd_vae_param_spec  # noqa: E402

DEV = "cuda"
PEAK_TFLOPS = 2500.0


def events_ms(fn, warm=3, reps=20):
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


def flops(side, B, H, W):
    """multiply-adds x 2 of every conv / linear / attention product, counted from shapes (image H x W)"""
    spec = sd_vae_param_spec()
    f = 0

    def conv(name, h, w):
        nonlocal f
        co, ci, kh, kw = spec[name + ".weight"] if len(spec[name + ".weight"]) == 4 else spec[name + ".weight"] + (1, 1)
        f += 2 * co * ci * kh * kw * h * w

    def resnet(p, h, w):
        conv(p + ".conv1", h, w)
        conv(p + ".conv2", h, w)
        if p + ".conv_shortcut.weight" in spec:
            conv(p + ".conv_shortcut", h, w)

    def mid(p, h, w):
        nonlocal f
        resnet(p + ".resnets.0", h, w)
        resnet(p + ".resnets.1", h, w)
        T = h * w
        f += 2 * 4 * T * 512 * 512 + 2 * 2 * T * T * 512

    if side == "enc":
        h, w = H, W
        conv("encoder.conv_in", h, w)
        for i in range(4):
            for j in range(2):
                resnet(f"encoder.down_blocks.{i}.resnets.{j}", h, w)
            if i < 3:
                h, w = h // 2, w // 2
                conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", h, w)
        mid("encoder.mid_block", h, w)
        conv("encoder.conv_out", h, w)
    else:
        h, w = H // 8, W // 8
        conv("decoder.conv_in", h, w)
        mid("decoder.mid_block", h, w)
        for i in range(4):
            for j in range(3):
                resnet(f"decoder.up_blocks.{i}.resnets.{j}", h, w)
            if i < 3:
                h, w = h * 2, w * 2
                conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", h, w)
        conv("decoder.conv_out", h, w)
    return B * f


def main():
    sd = random_vae_kl_state_dict(device=DEV)
    vae = HipAutoencoderKL(sd, device=DEV)
    res = {"device": _lib.device_name(), "block_out_channels": BLOCK_OUT, "configs": {}}
    g = torch.Generator().manual_seed(0)
    for B, H, W in ((1, 512, 512), (8, 512, 512), (1, 384, 384), (1, 512, 768)):
        x = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).half().to(DEV)
        z = torch.randn(B, 4, H // 8, W // 8, generator=g).half().to(DEV)
        vae.encode(x)
        vae.decode(z)
        row = {}
        for side, inp in (("enc", x), ("dec", z)):
            st = vae._plan(side, B, *inp.shape[2:])
            st.inp.copy_(inp.reshape(st.inp.shape))
            ms = events_ms(st.pl.run)
            fl = flops(side, B, H, W)
            row[side] = {"ms": round(ms, 3), "launches": len(st.pl), "TFLOP": round(fl / 1e12, 3), "TFLOPs": round(fl / ms / 1e9, 1)}
        res["configs"][f"B{B}_{H}x{W}"] = row
    names = {v: k[3:].lower() for k, v in vars(_lib).items() if k.startswith("OP_") and isinstance(v, int)}
    for side, shape in (("enc", (1, 512, 512)), ("dec", (1, 64, 64))):
        st = vae._plan(side, *shape)
        each = st.pl.time_each_us(reps=10)
        fam = {}
        for op, us in zip(st.pl._ops, each):
            k = names.get(op.kind, str(op.kind))
            fam.setdefault(k, [0, 0.0])
            fam[k][0] += 1
            fam[k][1] += us
        res[f"{side}_512_launch_split_us"] = {k: [n, round(us, 1)] for k, (n, us) in sorted(fam.items(), key=lambda kv: -kv[1][1])}
    # the attention op alone
    T = 4096
    qkv = torch.randn(T, 1536, generator=g).half().to(DEV)
    out = torch.empty(T, 512, dtype=torch.float16, device=DEV)
    S = ops.vae_attn_schedule(1, T)
    n_img, n_ws = ops.vae_attn_sizes(1, T, S)
    img = torch.empty(n_img, dtype=torch.float16, device=DEV)
    ws = torch.empty(max(1, n_ws), dtype=torch.float32, device=DEV)
    pl = _lib.OpList()
    pl.append(*ops.vae_attn(qkv, out, img, ws, B=1, T=T, ld=1536, ldo=512, S=S))
    us = events_ms(pl.run, warm=5, reps=50) * 1e3
    fl = 2 * 2 * T * T * 512
    res["attn_B1_T4096"] = {"us": round(us, 1), "splits": S, "GFLOP": round(fl / 1e9, 1), "TFLOPs": round(fl / us / 1e6, 1),
                            "fraction_of_peak": round(fl / us / 1e6 / PEAK_TFLOPS, 3)}
    # comparison point: the fp16 restatement on the same GPU
    import vae_kl_ref as R
    sd16 = {k: v.half() for k, v in sd.items()}
    x = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).half().to(DEV)
    z = torch.randn(1, 4, 64, 64, generator=g).half().to(DEV)
    with torch.no_grad():
        res["torch_fp16_512"] = {"enc_ms": round(events_ms(lambda: R.encode(x, sd16)), 3),
                                 "dec_ms": round(events_ms(lambda: R.decode(z, sd16)), 3)}
    # the VAE share of one frame: encode_image + encode_depth + decode at 512^2
    from live2diff_amd.vae_hip import HipTinyVAE, random_taesd_state_dict
    tiny = HipTinyVAE(random_taesd_state_dict(device=DEV), device=DEV)

    def frame(v):
        v.encode(x)
        v.encode(x)
        v.decode(z)
    res["frame_vae_ms_512"] = {"kl": round(events_ms(lambda: frame(vae)), 3), "tiny": round(events_ms(lambda: frame(tiny)), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
