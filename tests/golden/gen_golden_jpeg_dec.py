"""Writes tests/golden/jpeg_dec_pillow.npz: JPEG files written by the installed Pillow (libjpeg-turbo) and the pixels the same
Pillow decodes from them -- the pin of `live2diff_amd.jpeg.decode_ref`, which in turn is the oracle of csrc/jpeg_dec.hip.

    python tests/golden/gen_golden_jpeg_dec.py

Covered, one file per (size, sampling, restart markers, tables), quality and content rotating over them: sizes 8x8, 16x16,
23x17, 17x23 and 100x75 (width x height: one MCU, and partial MCUs in either or both directions for all three layouts); 4:4:4,
4:2:2, 4:2:0; standard and optimised Huffman tables; no restart markers, one per MCU, one per MCU row; quality 1, 50, 95, 100;
flat, gradient and uniform-noise content.  Plus `noise_q100`, 256x192 noise at quality 100 (many stuffed FF 00 pairs: the hard
case of the bit reader), and `roundtrip`, what the project's own encoder writes for a 64x48 frame.  Every entry `f_<name>` is a
file, `p_<name>` its decoded pixels.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, ImageFile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
ImageFile.MAXBLOCK = 1 << 22          # `optimize=True` needs the whole file in one buffer; the default fails on noisy frames

SIZES = ((8, 8), (16, 16), (23, 17), (17, 23), (100, 75))
QUALITIES = (1, 50, 95, 100)
CONTENTS = ("flat", "gradient", "noise")
RESTARTS = (("none", {}), ("blocks", {"restart_marker_blocks": 1}), ("rows", {"restart_marker_rows": 1}))
SEED = 2
NOISE_SEED = 70       # of `noise_q100`: with chunk_mcus = 1 a chunk begins in the byte behind a stuffed FF 00 and one ends inside an FF
#                       (tests/test_jpeg_dec_cpu.py asserts it; about one seed in forty gives both)


def content(kind, W, H, rng):
    if kind == "flat":
        return np.full((H, W, 3), (200, 30, 90), np.uint8)
    if kind == "gradient":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def write(u8, **kw):
    b = io.BytesIO()
    Image.fromarray(u8).save(b, format="JPEG", **kw)
    return b.getvalue()


def pixels(f):
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def main():
    from live2diff_amd import jpeg
    rng = np.random.default_rng(SEED)
    out, i = {}, 0
    for W, H in SIZES:
        for ss, sname in ((0, "444"), (1, "422"), (2, "420")):
            for rname, rkw in RESTARTS:
                for opt in (False, True):
                    q, kind = QUALITIES[i % 4], CONTENTS[(i // 4 + i) % 3]
                    i += 1
                    name = f"{W}x{H}_{sname}_{rname}_{'opt' if opt else 'std'}_q{q}_{kind}"
                    out[name] = write(content(kind, W, H, rng), quality=q, subsampling=ss, optimize=opt, **rkw)
    out["noise_q100"] = write(content("noise", 256, 192, np.random.default_rng(NOISE_SEED)), quality=100, subsampling=2)
    yy, xx = np.mgrid[0:48, 0:64]
    frame = np.clip(np.stack([128 + 100 * np.sin(xx / 9.0 + yy / 13.0), 128 + 90 * np.cos(yy / 7.0), xx * 4.0], -1)
                    + rng.normal(0, 6, (48, 64, 3)), 0, 255).astype(np.uint8)
    out["roundtrip"] = jpeg.encode_ref(frame, 75)
    arrays = {"roundtrip_source": frame}
    for name, f in out.items():
        arrays["f_" + name] = np.frombuffer(f, np.uint8)
        arrays["p_" + name] = pixels(f)
    path = os.path.join(HERE, "jpeg_dec_pillow.npz")
    np.savez_compressed(path, **arrays)
    combos = {(n.split("_")[-2], n.split("_")[-1]) for n in out if n[0].isdigit()}
    print(f"{len(out)} files, {sum(len(f) for f in out.values())} bytes of JPEG, {os.path.getsize(path)} bytes written; "
          f"{len(combos)} of 12 (quality, content) pairs")


if __name__ == "__main__":
    main()
