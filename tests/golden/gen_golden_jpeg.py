"""Writes tests/golden/jpeg_pillow.npz: small uint8 frames and the bytes Pillow wrote for them with
`save(format="JPEG", quality=q, restart_marker_rows=1)` (default 4:2:0 sub-sampling, standard Huffman tables) -- the independent
implementation `live2diff_amd.jpeg.encode_ref` is pinned to, byte for byte (tests/test_jpeg_cpu.py).  Needs Pillow; the tests do not.

    python tests/golden/gen_golden_jpeg.py

Keys: `frame_<i>` uint8 [H,W,3]; `jpeg_<i>_q<q>` uint8 [n] for q in QUALITIES; `pillow_version`."""
import io
import os

import numpy as np

QUALITIES = (1, 10, 50, 75, 95, 100)


def frames():
    """(name, uint8 [H,W,3]): one content kind per size"""
    rng = np.random.default_rng(20240607)
    yy, xx = np.mgrid[0:64, 0:64]
    smooth = np.stack([128 + 100 * np.sin(xx / 17.0 + yy / 29.0), 128 + 90 * np.cos(yy / 11.0), xx * 255.0 / 64], -1)
    yield "smooth + noise 64x64", np.clip(smooth + rng.normal(0, 6, smooth.shape), 0, 255).astype(np.uint8)
    yield "uniform noise 64x96", rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:128, 0:64]
    yield "0 / 255 checkerboard 128x64", np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    yield "constant 192x256", np.full((192, 256, 3), (200, 30, 90), np.uint8)


def main():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (name, f) in enumerate(frames()):
        out[f"frame_{i}"] = f
        for q in QUALITIES:
            b = io.BytesIO()
            Image.fromarray(f).save(b, format="JPEG", quality=q, restart_marker_rows=1)
            data = b.getvalue()
            assert b"\xff\xdd\x00\x04" in data, "this Pillow ignores restart_marker_rows"
            out[f"jpeg_{i}_q{q}"] = np.frombuffer(data, np.uint8)
            print(f"{name}, quality {q}: {len(data)} bytes")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
