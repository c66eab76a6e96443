"""A folder of image files (PIL) or an .npy stack of uint8 frames -> StreamAnimateDiffusionDepthWrapper -> a folder of PNGs.

    python tools/stream_frames.py --config configs/toonyou.yaml --input frames/ --output out/ [--prompt "..."] [--height 512 --width 512]

Follows the reference's test.py: the first `--skip` (2) frames are dropped, the next 8 are the warm-up window, and because the
stream batch holds `batch_size` denoising steps in flight, the output of call t belongs to input frame t - (batch_size - 1)
(test.py:101,169-174): the first batch_size - 1 outputs are discarded and as many trailing frames are fed again to flush.
Frames of any size are resized + centre-cropped on the device (frame_io.HipFrameIO).  Prints `inference_time_ema`."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def read_frames(path: str) -> np.ndarray:
    """uint8 [F,Hs,Ws,3]"""
    if path.endswith(".npy"):
        arr = np.load(path)
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
            raise ValueError(f"{path}: expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}")
        return arr
    from PIL import Image
    names = sorted(n for n in os.listdir(path) if n.lower().endswith(EXTS))
    if not names:
        raise FileNotFoundError(f"--input: no image files in {path}")
    frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names]
    if len({f.shape for f in frames}) != 1:
        raise ValueError(f"{path}: frames differ in size")
    return np.stack(frames)


def align(outputs, batch_size: int):
    """outputs of the calls -> outputs per input frame: drop the first batch_size - 1 (test.py:169-174)"""
    return outputs[batch_size - 1:]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--input", required=True, help="folder of images, or .npy uint8 [F,H,W,3]")
    ap.add_argument("--output", required=True)
    ap.add_argument("--prompt", default=None, help="default: the config's `prompt`")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--engine-dir", default="engines")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--full-vae", action="store_true", help="the SD AutoencoderKL instead of the tiny VAE")
    args = ap.parse_args(argv)

    from PIL import Image

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper, load_config, stream_sizes
    cfg = load_config(args.config)
    sink = stream_sizes(cfg)[1]
    frames = read_frames(args.input)[args.skip:]
    if len(frames) <= sink:
        raise ValueError(f"{len(frames)} frames after --skip: need more than the {sink} warm-up frames")
    w = StreamAnimateDiffusionDepthWrapper(args.config, few_step_model_type="lcm", num_inference_steps=cfg.get("num_inference_steps", 50),
                                           t_index_list=cfg.get("t_index_list"), strength=cfg.get("strength"), output_type="u8",
                                           height=args.height, width=args.width, use_tiny_vae=not args.full_vae, seed=args.seed,
                                           engine_dir=args.engine_dir)
    prompt = args.prompt if args.prompt is not None else str(cfg.get("prompt", ""))
    os.makedirs(args.output, exist_ok=True)
    warm = w.prepare(frames[:sink], prompt)
    for i, f in enumerate(warm):
        Image.fromarray((f.float().cpu().numpy() * 255).round().astype("uint8")).save(os.path.join(args.output, f"{i:05d}.png"))
    rest = frames[sink:]
    feed = list(rest) + [rest[-1]] * (w.batch_size - 1)                   # flush the frames still in the stream batch
    outs = align([w(f) for f in feed], w.batch_size)
    for i, o in enumerate(outs):
        Image.fromarray(o).save(os.path.join(args.output, f"{sink + i:05d}.png"))
    print(f"{len(warm)} warm-up + {len(outs)} frames -> {args.output}; inference_time_ema {w.stream.inference_time_ema * 1e3:.2f} ms "
          f"({1.0 / max(w.stream.inference_time_ema, 1e-9):.1f} fps)")


if __name__ == "__main__":
    main()
