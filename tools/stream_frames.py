"""A folder of image files (PIL) or an .npy stack of uint8 frames -> StreamAnimateDiffusionDepthWrapper -> a folder of PNGs.

    python tools/stream_frames.py --config configs/toonyou.yaml --input frames/ --output out/ [--prompt "..."] [--height 512 --width 512]

Follows the reference's test.py: the first `--skip` (2) frames are dropped, the next 8 are the warm-up window, and because the
stream batch holds `batch_size` denoising steps in flight, the output of call t belongs to input frame t - (batch_size - 1)
(test.py:101,169-174): the first batch_size - 1 outputs are discarded and as many trailing frames are fed again to flush.
Frames of any size are resized + centre-cropped on the device (frame_io.HipFrameIO).  Prints `inference_time_ema`.

    ... --depth depth/ [--depth-kind distance --depth-range 300,5000]

takes every frame's conditioning depth from a 16-bit PNG of the same file name (any size; 0 marks a hole) instead of the built-in
detector, which is then not even built (`depth_source="input"`, depth_io.py); with an .npy input, `--depth` is an .npy stack
[F,Hd,Wd] of uint16 or float32.

    ... --mask masks/ [--matte 0,1,2] [--mask-input and,invert]

cuts every frame by its own mask -- an image of the same file name (any size; mode L, 1, I;16 or F), the output of a person
segmenter or a keyer -- in place of the depth ramp, or combined with it (`mask=`, mask_io.py); with an .npy input, `--mask` is an
.npy stack [F,Hm,Wm] of uint8, uint16, bool or float32.  A mask needs a matte: `--matte LO,HI[,FEATHER[,far]]` (default `0,1`)
gives the ramp that `and` / `or` combine with, and the feather."""
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


def read_depths(path: str, input_path: str) -> np.ndarray:
    """uint16 / float32 [F,Hd,Wd]: one depth frame per frame of `input_path`, matched by file name"""
    if path.endswith(".npy"):
        arr = np.load(path)
        if arr.dtype not in (np.uint16, np.float32) or arr.ndim != 3:
            raise ValueError(f"{path}: expected uint16 or float32 [F,Hd,Wd], got {arr.dtype} {arr.shape}")
        return arr
    if input_path.endswith(".npy"):
        raise ValueError("--depth: an .npy input has no file names to match: give the depth frames as an .npy stack too")
    from PIL import Image
    by_stem = {os.path.splitext(n)[0]: n for n in os.listdir(path) if n.lower().endswith(".png")}
    frames = []
    for n in sorted(n for n in os.listdir(input_path) if n.lower().endswith(EXTS)):
        stem = os.path.splitext(n)[0]
        if stem not in by_stem:
            raise FileNotFoundError(f"--depth: {path} has no {stem}.png for the frame {n}")
        img = Image.open(os.path.join(path, by_stem[stem]))
        if img.mode not in ("I;16", "I;16L", "I;16B", "I"):
            raise ValueError(f"--depth: {by_stem[stem]} is no 16-bit PNG (mode {img.mode!r})")
        frames.append(np.asarray(img).astype(np.uint16))
    if len({f.shape for f in frames}) != 1:
        raise ValueError(f"{path}: depth frames differ in size")
    return np.stack(frames)


def read_masks(path: str, input_path: str) -> list:
    """one mask per frame of `input_path`, matched by file name: uint8 / uint16 / float32 [Hm,Wm] arrays (an .npy stack: its rows)"""
    from live2diff_amd.mask_io import _as_mask, load
    if path.endswith(".npy"):
        arr = np.load(path)
        if arr.ndim != 3:
            raise ValueError(f"{path}: expected [F,Hm,Wm], got {arr.shape}")
        return [_as_mask(m) for m in arr]
    if input_path.endswith(".npy"):
        raise ValueError("--mask: an .npy input has no file names to match: give the masks as an .npy stack too")
    by_stem = {os.path.splitext(n)[0]: n for n in os.listdir(path) if n.lower().endswith(EXTS + (".tif", ".tiff"))}
    masks = []
    for n in sorted(n for n in os.listdir(input_path) if n.lower().endswith(EXTS)):
        stem = os.path.splitext(n)[0]
        if stem not in by_stem:
            raise FileNotFoundError(f"--mask: {path} has no image named {stem} for the frame {n}")
        masks.append(_as_mask(load(os.path.join(path, by_stem[stem]), f"--mask: {by_stem[stem]}")))
    return masks


def parse_matte(text: str) -> dict:
    """`LO,HI[,FEATHER[,far]]` -> the keywords of `wrapper.set_matte`"""
    from live2diff_amd.matte import check_settings
    parts = [t.strip() for t in text.split(",")]
    if not 2 <= len(parts) <= 4 or (len(parts) == 4 and parts[3] != "far"):
        raise ValueError(f"--matte {text!r}: use LO,HI[,FEATHER[,far]]")
    try:
        lo, hi, feather = float(parts[0]), float(parts[1]), int(parts[2]) if len(parts) > 2 else 0
    except ValueError:
        raise ValueError(f"--matte {text!r}: LO and HI are numbers in [0, 1], FEATHER an integer") from None
    s = check_settings(lo, hi, keep="far" if len(parts) == 4 else "near", feather=feather)
    return dict(lo=s["lo"], hi=s["hi"], keep=s["keep"], feather=s["feather"])


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
    ap.add_argument("--depth", default=None, help="folder of 16-bit PNGs named like the frames (or .npy [F,Hd,Wd]): depth from the caller")
    ap.add_argument("--depth-kind", default="distance", choices=("distance", "inverse"))
    ap.add_argument("--depth-range", default=None, help="A,B: a fixed (near, far) / (lo, hi) in the units of the samples; default: per frame")
    ap.add_argument("--mask", default=None, help="folder of mask images named like the frames (or .npy [F,Hm,Wm]): the matte from the caller")
    ap.add_argument("--mask-input", default="replace", help="COMBINE[,invert]: replace (default), and, or -- how a mask meets the depth ramp")
    ap.add_argument("--matte", default=None, help="LO,HI[,FEATHER[,far]]: the depth matte (with --mask, default 0,1: the ramp `and` / `or` read)")
    ap.add_argument("--cut-detect", default=None, nargs="?", const="on", metavar="THUMB,HIST[,RATIO[,GAP]]",
                    help="find scene cuts on the device (wrapper.set_cut_detect; the defaults are a guess, untuned on footage); their frame "
                         "indices are printed at the end")
    ap.add_argument("--auto-rewarm", action="store_true",
                    help="re-warm the sinks by themselves once the last frames all lie behind a cut (keeps the recent window; needs --cut-detect)")
    args = ap.parse_args(argv)
    cut_detect = None
    if args.cut_detect is not None:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from mjpeg_server import parse_cut_detect_arg
        try:
            cut_detect = parse_cut_detect_arg(args.cut_detect)
        except ValueError as e:
            ap.error("--cut-detect: " + str(e))
    if args.auto_rewarm and cut_detect is None:
        ap.error("--auto-rewarm needs --cut-detect")

    from PIL import Image

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper, load_config, stream_sizes
    cfg = load_config(args.config)
    sink = stream_sizes(cfg)[1]
    frames = read_frames(args.input)[args.skip:]
    if len(frames) <= sink:
        raise ValueError(f"{len(frames)} frames after --skip: need more than the {sink} warm-up frames")
    depths, more = None, {}
    if args.depth is not None:
        depths = read_depths(args.depth, args.input)[args.skip:]
        if len(depths) != len(frames):
            raise ValueError(f"--depth: {len(depths)} depth frames for {len(frames)} frames")
        rng = None if args.depth_range is None else tuple(float(v) for v in args.depth_range.split(","))
        more = dict(depth_source="input", depth_input=dict(kind=args.depth_kind, invalid=0, range=rng))
    masks = None
    if args.mask is not None:
        from live2diff_amd.mask_io import check_settings as check_mask_input
        masks = read_masks(args.mask, args.input)[args.skip:]
        if len(masks) != len(frames):
            raise ValueError(f"--mask: {len(masks)} masks for {len(frames)} frames")
        parts = [t.strip() for t in args.mask_input.split(",")]
        if len(parts) > 2 or (len(parts) == 2 and parts[1] != "invert"):
            raise ValueError(f"--mask-input {args.mask_input!r}: use replace, and or or, optionally followed by ,invert")
        more["mask_input"] = check_mask_input(parts[0], len(parts) == 2)
    matte = parse_matte(args.matte if args.matte is not None else "0,1") if (args.matte is not None or masks is not None) else None
    w = StreamAnimateDiffusionDepthWrapper(args.config, few_step_model_type="lcm", num_inference_steps=cfg.get("num_inference_steps", 50),
                                           t_index_list=cfg.get("t_index_list"), strength=cfg.get("strength"), output_type="u8",
                                           height=args.height, width=args.width, use_tiny_vae=not args.full_vae, seed=args.seed,
                                           engine_dir=args.engine_dir, keep_recent=args.auto_rewarm, **more)
    if cut_detect is not None:
        w.set_cut_detect(**cut_detect)
        w.set_auto_rewarm(args.auto_rewarm)
    prompt = args.prompt if args.prompt is not None else str(cfg.get("prompt", ""))
    os.makedirs(args.output, exist_ok=True)
    if matte is not None:
        w.set_matte(matte["lo"], matte["hi"], keep=matte["keep"], feather=matte["feather"])      # (before `prepare`: the line is primed)
    warm = w.prepare(frames[:sink], prompt, warmup_depths=None if depths is None else depths[:sink],
                     **({} if masks is None else {"warmup_masks": masks[:sink]}))
    for i, f in enumerate(warm):
        Image.fromarray((f.float().cpu().numpy() * 255).round().astype("uint8")).save(os.path.join(args.output, f"{i:05d}.png"))
    rest = frames[sink:]
    feed = list(rest) + [rest[-1]] * (w.batch_size - 1)                   # flush the frames still in the stream batch
    dfeed = [None] * len(feed) if depths is None else list(depths[sink:]) + [depths[-1]] * (w.batch_size - 1)
    mfeed = [None] * len(feed) if masks is None else list(masks[sink:]) + [masks[-1]] * (w.batch_size - 1)
    outs = align([w(f, depth=d, **({} if m is None else {"mask": m})) for f, d, m in zip(feed, dfeed, mfeed)], w.batch_size)
    for i, o in enumerate(outs):
        Image.fromarray(o).save(os.path.join(args.output, f"{sink + i:05d}.png"))
    print(f"{len(warm)} warm-up + {len(outs)} frames -> {args.output}; inference_time_ema {w.stream.inference_time_ema * 1e3:.2f} ms "
          f"({1.0 / max(w.stream.inference_time_ema, 1e-9):.1f} fps)")
    if cut_detect is not None:
        # (indices count the frames behind the warm-up window; file names are `sink` further on)
        print(f"cuts at frames {[sink + n for n in w.cuts]} ({len(w.cuts)}); {w.auto_rewarms} automatic re-warms")


if __name__ == "__main__":
    main()
