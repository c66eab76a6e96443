"""Outputs of the REFERENCE's `image_utils.postprocess_image` (live2diff/image_utils.py:9-68) on fp16 frames.
Run in the build container (needs the reference checkout, like gen_golden_filter.py): python tests/golden/gen_frame_io_golden.py
Writes tests/golden/frame_io.npz:
  x            fp16 [2,3,16,24] in [-1.5, 1.5] with x = 0 (v = 0.5, 255 v = 127.5: the one exact tie an fp16 v in [0, 1] can produce;
               half-to-even gives 128), -1, 1 and their fp16 neighbours planted
  pil / pt / np   `postprocess_image(x, output_type=...)`: uint8 [2,16,24,3] (np.array of the PIL images), fp16 [2,3,16,24],
               float32 [2,16,24,3]
  sweep_x / sweep_u8   every finite fp16 in [-2, 2] as [1,3,n,1] planes (the three channels carry the same values) and its uint8
`image_utils.py` imports torchvision at module level (used by `process_image` only): a stub module stands in for it."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("L2D_REFERENCE", "/root/reference")


def load_image_utils():
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    spec = importlib.util.spec_from_file_location("ref_image_utils", os.path.join(REFERENCE, "live2diff", "image_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_input():
    g = torch.Generator().manual_seed(2024)
    x = (torch.rand(2, 3, 16, 24, generator=g) * 3.0 - 1.5).to(torch.float16)
    one = torch.tensor(1.0, dtype=torch.float16)
    ulp_in, ulp_out = 2.0 ** -11, 2.0 ** -10               # fp16 spacing just below / above 1
    planted = [0.0, -0.0, 1.0, -1.0, 1.0 - ulp_in, 1.0 + ulp_out, -1.0 + ulp_in, -1.0 - ulp_out, 1.5, -1.5, 2.0 ** -14, 6e-8]
    flat = x.view(-1)
    for i, v in enumerate(planted):
        flat[i * 7] = v
    assert float(one) == 1.0
    return x


def all_fp16(lo=-2.0, hi=2.0):
    bits = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    keep = np.isfinite(bits) & (bits >= lo) & (bits <= hi)
    return torch.from_numpy(bits[keep].copy())


def main():
    mod = load_image_utils()
    x = fixture_input()
    pil = np.stack([np.array(im) for im in mod.postprocess_image(x, output_type="pil")])
    pt = mod.postprocess_image(x, output_type="pt")
    npy = mod.postprocess_image(x, output_type="np")
    sw = all_fp16()
    sx = sw.view(1, 1, -1, 1).repeat(1, 3, 1, 1).contiguous()
    su = np.array(mod.postprocess_image(sx, output_type="pil")[0])[:, 0, 0]
    out = os.path.join(HERE, "frame_io.npz")
    np.savez_compressed(out, x=x.numpy(), pil=pil, pt=pt.numpy(), np=npy, sweep_x=sw.numpy(), sweep_u8=su)
    print("wrote", out, os.path.getsize(out), "bytes;", sw.numel(), "sweep values; pil", pil.shape, pil.dtype, "pt", pt.dtype, "np", npy.dtype)


if __name__ == "__main__":
    main()
