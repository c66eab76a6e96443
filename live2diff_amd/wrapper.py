"""`StreamAnimateDiffusionDepthWrapper` -- the reference's public interface (live2diff/utils/wrapper.py:17-297, driven by test.py
and demo/vid2vid.py) on the native parts only: config path in, `prepare(warmup_frames, prompt)`, then `wrapper(image) -> image`.
Model files in, camera-sized uint8 frames in, uint8 frames out; it imports neither diffusers, omegaconf, torchvision nor
transformers.

  * `load_config`      the reference's YAML schema (configs/*.yaml, `base:` inheritance) with PyYAML;
  * `load_components`  the assembly order of wrapper.py:404-470 and pipeline_animatediff_depth.py:250-305 on state dicts:
                       2D UNet -> inflate -> motion checkpoint -> DreamBooth -> few-step LoRA -> LoRAs -> `HipStreamingUNet`
                       (through the packed-weight cache), text encoder, VAE, depth detector;
  * the wrapper        frames go through `frame_io.HipFrameIO` (one launch in, one launch out); `prepare` enables the device step.

Differences from the reference, all on purpose: nothing is fetched from a hub (`few_step_lora_path` / `taesd_path` are config
keys), a missing file raises FileNotFoundError naming its config key (the reference prints a traceback and exits), keywords the
backend cannot honour raise ValueError at construction, `"u8"` is a fifth output type and `"jpeg"` (with `jpeg_quality`) a sixth:
the frame leaves the device as the JPEG file the reference's demo makes of it on the host (jpeg_io.HipJpegEncoder).  A frame may
also ARRIVE as a JPEG file (`bytes`, what the reference's demo receives from the browser, demo/util.py:22): it is decoded on the
device (jpeg_io.HipJpegDecoder) and ingested there like a uint8 frame (`jpeg_decode="host"` decodes with Pillow instead).
`set_matte` composites the output over the stream's own source frame by a matte of the frame's depth map (matte.py);
`set_color_lock` holds the output's per-channel colour statistics to the source's, a running average's or a reference image's
(color_lock.py).  `set_output_size` (or the `output_size` keyword) resamples the uint8 frame to a size of the caller's choice
with Pillow's arithmetic, behind both and in front of the JPEG encoder or the copy to the host (resize.py).
`set_matte_source("camera")` composites the matte at the output size over the camera's own pixels (matte.HipMatteUp).
`set_steady` holds the previous output pixel where the frame's source did not move (steady.py), behind the colour lock.
`set_steady_follow` lets it look where each 8 x 8 block of the source came from, so that it also holds under a moving camera.
`set_matte_edge` refines the matte by the source frame, so that its edges land on the frame's own (matte.edge_ref).
`set_matte_hold` keeps the matte still where the camera is still: the matte filtered in time by steady's measure (matte.hold_ref).
`set_detail` brings the camera's fine detail into the frame at the output size, behind the resize (detail.py).
`set_backdrop` puts the room blurred, a colour or an image behind the matte in place of the real frame (backdrop.py).
`wrapper(image, depth=d)` conditions a frame on the caller's own depth frame -- an RGB-D camera's, another estimator's -- instead
of the built-in detector's; `set_depth_input` says how it is read, `depth_source="input"` builds no detector at all (depth_io.py).

Every frame leaves through one chain, `_route`: colour lock, then steady (`_finish`, in front of it) -> matte composite, or egress -> resize
-> detail -> JPEG encoder, or copy to the host.  A stage that is not set is not in the chain; on the device each stage is one launch that
hands its static buffer to the next, and only the last one copies to the host.
"""
import functools
import os
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import convert, ops
from .config import UNetConfig
from .pipeline_stream_animation_depth import StreamAnimateDiffusionDepth

OUTPUT_TYPES = ("pil", "pt", "np", "latent", "u8", "jpeg")


# ----------------------------------------------------------------------------- config
def _merge(base: dict, over: dict) -> dict:
    out = dict(base)
    for k, v in over.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def load_config(path: Union[str, os.PathLike]) -> dict:
    """The reference's `load_config` (live2diff/utils/config.py:10-17) as plain dicts: the file, recursively merged over the file
    its `base:` key names.  The reference resolves `base` against the working directory (`./configs/base_config.yaml`); here it is
    also looked for beside the config and one directory up, so a config directory works from anywhere."""
    import yaml
    path = str(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"config_path: {path} does not exist")
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    base = cfg.pop("base", None)
    if base:
        here = os.path.dirname(os.path.abspath(path))
        for cand in (base, os.path.join(here, base), os.path.join(os.path.dirname(here), base), os.path.join(here, os.path.basename(base))):
            if os.path.isfile(cand):
                return _merge(load_config(cand), cfg)
        raise FileNotFoundError(f"base: {base} (named by {path}) does not exist")
    return cfg


def stream_sizes(cfg: dict):
    """(window_size, sink_size, temporal_position_encoding_max_len) of a config"""
    mm = (cfg.get("unet_additional_kwargs") or {}).get("motion_module_kwargs") or {}
    att = mm.get("attention_kwargs") or {}
    return int(att.get("window_size", 16)), int(att.get("sink_size", 8)), int(mm.get("temporal_position_encoding_max_len", 24))


# ----------------------------------------------------------------------------- one loader per file kind (tests substitute them)
def _need(key: str, path, kind=os.path.exists):
    if path is None:
        raise FileNotFoundError(f"{key}: not set in the config")
    if not kind(str(path)):
        raise FileNotFoundError(f"{key}: {path} does not exist")
    return str(path)


def load_tensors(path: str) -> dict:
    """a .safetensors file, or a torch checkpoint (.ckpt / .pt / .bin) -- tensors only, on the CPU"""
    if str(path).endswith(".safetensors"):
        return convert.load_safetensors(str(path))
    return torch.load(str(path), map_location="cpu", weights_only=True)


def _model_file(folder: str) -> str:
    for name in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin", "model.safetensors", "pytorch_model.bin"):
        if os.path.isfile(os.path.join(folder, name)):
            return os.path.join(folder, name)
    raise FileNotFoundError(f"pretrained_model_path: no weight file in {folder}")


def load_unet_config(model_dir: str, cfg: dict) -> UNetConfig:
    """widths / text width from `unet/config.json` when the directory has one (SD-1.5 values otherwise); window, sink and the
    PE length from the config's `unet_additional_kwargs`"""
    import json
    window, sink, max_len = stream_sizes(cfg)
    kw = {}
    p = os.path.join(model_dir, "unet", "config.json")
    if os.path.isfile(p):
        with open(p) as f:
            j = json.load(f)
        if "block_out_channels" in j:
            kw["block_out_channels"] = tuple(j["block_out_channels"])
        if "cross_attention_dim" in j:
            kw["cross_attention_dim"] = int(j["cross_attention_dim"])
    return UNetConfig(window_size=window, sink_size=sink, temporal_max_len=max(max_len, window), **kw)


def load_unet_2d(model_dir: str) -> dict:
    return load_tensors(_model_file(_need("pretrained_model_path", os.path.join(model_dir, "unet"), os.path.isdir)))


def load_motion_checkpoint(path: str) -> dict:
    return load_tensors(_need("motion_module_path", path, os.path.isfile))


def load_depth_state_dict(path: str) -> dict:
    sd = load_tensors(_need("depth_model_path", path, os.path.isfile))
    return sd["model"] if "optimizer" in sd else sd            # (MiDaS' own loader, DPTDepthModel.load)


def load_style_file(key: str, path: str) -> dict:
    return load_tensors(_need(key, path, os.path.isfile))


def load_taesd(path: str) -> dict:
    path = _need("taesd_path", path)
    return load_tensors(_model_file(path) if os.path.isdir(path) else path)


def load_vae_kl(model_dir: str) -> dict:
    return load_tensors(_model_file(_need("pretrained_model_path", os.path.join(model_dir, "vae"), os.path.isdir)))


def load_prompt_encoder(model_dir: str, device, clip_skip, dreambooth=None, loras=None):
    """`clip_hip.load_text_encoder` in pieces, with the style's text half merged in between (converter/convert.py:47-50, 72-88)"""
    import json

    from .clip_hip import HipClipTextEncoder, HipPromptEncoder, config_from_json
    from .clip_tokenizer import ClipTokenizer
    te = _need("pretrained_model_path", os.path.join(model_dir, "text_encoder"), os.path.isdir)
    with open(os.path.join(te, "config.json")) as f:
        ccfg = config_from_json(json.load(f))
    sd = text_encoder_state_dict(model_dir, dreambooth, loras)
    tok = ClipTokenizer.from_dir(os.path.join(model_dir, "tokenizer"), max_length=ccfg.max_position_embeddings)
    return HipPromptEncoder(HipClipTextEncoder(sd, device, ccfg), tok, clip_skip)


# ----------------------------------------------------------------------------- assembly
def _style(cfg: dict, dreambooth_path, lora_dict):
    """(dreambooth path or None, {lora path: strength}) -- the keyword wins over the config; the config's lora_list comes first"""
    third = cfg.get("third_party_dict") or {}
    loras = {}
    for item in third.get("lora_list") or []:
        loras[item["lora"]] = item["lora_alpha"]
    loras.update(lora_dict or {})
    return dreambooth_path or third.get("dreambooth"), loras


def load_style_unet(cfg: dict, ucfg: UNetConfig, lat_h: int, lat_w: int, denoising_steps_num: int, *, device="cuda",
                    dreambooth_path=None, lora_dict=None, few_step_model_type: str = "lcm",
                    engine_dir: Optional[Union[str, os.PathLike]] = "engines"):
    """One style's `HipStreamingUNet` (through the packed-weight cache) plus its DreamBooth state dict and [(LoRA, strength)]: what
    `load_components` builds the stream from and `add_style` a resident weight set."""
    from .unet_hip import HipStreamingUNet
    model_dir = _need("pretrained_model_path", cfg.get("pretrained_model_path"), os.path.isdir)
    db_path, loras = _style(cfg, dreambooth_path, lora_dict)
    name = Path(db_path).stem if db_path else "sd15"
    cache = None
    if engine_dir is not None:
        stem = HipStreamingUNet.packed_cache_name(name, few_step_model_type, ucfg.window_size, loras, lat_h, lat_w, denoising_steps_num)
        cache = os.path.join(str(engine_dir), stem + ".safetensors")
    # every file is looked at before anything is converted: a typo in the config costs no minutes of packing
    _need("motion_module_path", cfg.get("motion_module_path"), os.path.isfile)
    _need("few_step_lora_path", cfg.get("few_step_lora_path"), os.path.isfile)
    dreambooth = load_style_file("third_party_dict.dreambooth", db_path) if db_path else None
    if dreambooth is not None and "state_dict" in dreambooth:
        dreambooth = dreambooth["state_dict"]
    lora_sds = [(load_style_file("lora", p), float(a)) for p, a in loras.items()]
    if cache is not None and os.path.isfile(cache):
        unet = HipStreamingUNet(cache, ucfg, lat_h, lat_w, denoising_steps_num, device=device)
    else:
        sd2d = load_unet_2d(model_dir)
        base = convert.inflate_2d_unet(sd2d, ucfg)
        sd = convert.build_state_dict(base, ucfg, dreambooth=dreambooth, loras=lora_sds,
                                      motion_ckpt=load_motion_checkpoint(cfg["motion_module_path"]),
                                      few_step_lora=load_style_file("few_step_lora_path", cfg["few_step_lora_path"]))
        left = [k for k in base if k not in sd2d and sd[k] is base[k]]       # zero placeholders nothing replaced
        if left:
            raise KeyError(f"{len(left)} UNet parameters come from neither the 2D UNet nor the motion checkpoint: {left[:8]}")
        unet = HipStreamingUNet(sd, ucfg, lat_h, lat_w, denoising_steps_num, device=device)
        if cache is not None:
            os.makedirs(os.path.dirname(cache), exist_ok=True)
            unet.save_packed(cache)
    return unet, dreambooth, lora_sds


def text_encoder_state_dict(model_dir: str, dreambooth=None, loras=None) -> dict:
    """the text encoder's state dict with the style's text half merged in (converter/convert.py:47-50, 72-88)"""
    te = _need("pretrained_model_path", os.path.join(model_dir, "text_encoder"), os.path.isdir)
    has_te = dreambooth is not None and any(k.startswith(convert.LDM_CLIP_PREFIX) for k in dreambooth)
    return convert.build_text_encoder_state_dict(load_tensors(_model_file(te)), dreambooth if has_te else None, loras)


def load_components(cfg: dict, *, height: int, width: int, denoising_steps_num: int, device="cuda", dreambooth_path=None,
                    lora_dict=None, few_step_model_type: str = "lcm", vae_id=None, use_tiny_vae: bool = True,
                    engine_dir: Optional[Union[str, os.PathLike]] = "engines", depth_source: str = "detector"):
    """config dict -> the `pipe` namespace `StreamAnimateDiffusionDepth` takes (unet, vae, depth_model, `_encode_prompt`, scheduler).
    `depth_source="input"`: every frame brings its own depth, so `depth_model_path` is not needed and no detector is built
    (`depth_model` is None)."""
    _check_depth_source(depth_source)
    model_dir = _need("pretrained_model_path", cfg.get("pretrained_model_path"), os.path.isdir)
    ucfg = load_unet_config(model_dir, cfg)
    unet, dreambooth, lora_sds = load_style_unet(cfg, ucfg, height // 8, width // 8, denoising_steps_num, device=device,
                                                 dreambooth_path=dreambooth_path, lora_dict=lora_dict,
                                                 few_step_model_type=few_step_model_type, engine_dir=engine_dir)
    clip_skip = (cfg.get("third_party_dict") or {}).get("clip_skip", 1)
    prompt_encoder = load_prompt_encoder(model_dir, device, clip_skip, dreambooth, lora_sds)
    if use_tiny_vae:
        from .vae_hip import HipTinyVAE
        tsd = load_taesd(vae_id or cfg.get("taesd_path"))
        vae = HipTinyVAE(tsd, device=device, width=int(tsd["encoder.layers.0.weight"].shape[0]))
    else:
        from .vae_kl_hip import HipAutoencoderKL
        has_vae = dreambooth is not None and any(k.startswith(convert.LDM_VAE_PREFIX) for k in dreambooth)
        vae = HipAutoencoderKL(convert.build_vae_state_dict(load_vae_kl(model_dir), dreambooth if has_vae else None), device=device)
    depth = None
    if depth_source == "detector":
        from .midas_hip import HipMidas
        depth = HipMidas(load_depth_state_dict(cfg.get("depth_model_path")), device=device)
    return SimpleNamespace(device=torch.device(device), vae_scale_factor=8, unet=unet, vae=vae, depth_model=depth,
                           text_encoder=prompt_encoder.encoder, tokenizer=prompt_encoder.tokenizer,
                           _encode_prompt=prompt_encoder._encode_prompt, unet_config=ucfg,
                           scheduler=SimpleNamespace(config=dict(cfg.get("noise_scheduler_kwargs") or {})))


def build_style_sets(cfg: dict, like_unet, like_text, *, dreambooth_path=None, lora_dict=None, few_step_model_type: str = "lcm",
                     engine_dir: Optional[Union[str, os.PathLike]] = "engines"):
    """The packed weight sets (UNet, text encoder) of one style, through the path `load_components` takes: `build_state_dict` and
    the packed-weight cache under the same `packed_cache_name`, `build_text_encoder_state_dict`.  They come from second, plan-less
    instances of the configuration of `like_unet` / `like_text` (plans are built lazily: such an instance costs only its weights),
    so the running instances are not disturbed."""
    from .clip_hip import HipClipTextEncoder
    unet, dreambooth, lora_sds = load_style_unet(cfg, like_unet.cfg, like_unet.h, like_unet.w, like_unet.N, device=like_unet.device,
                                                 dreambooth_path=dreambooth_path, lora_dict=lora_dict,
                                                 few_step_model_type=few_step_model_type, engine_dir=engine_dir)
    tsd = text_encoder_state_dict(cfg["pretrained_model_path"], dreambooth, lora_sds)
    text = HipClipTextEncoder(tsd, like_text.device, like_text.cfg, use_graph=False)
    return unet.packed_state(), text.packed_state()


def _check_depth_source(source) -> None:
    if source not in ("detector", "input"):
        raise ValueError(f"depth_source={source!r}: use 'detector' or 'input'")


def _is_jpeg(x) -> bool:
    return isinstance(x, (bytes, bytearray, memoryview)) and bytes(x[:2]) == b"\xff\xd8"


# ----------------------------------------------------------------------------- the wrapper
class StreamAnimateDiffusionDepthWrapper:
    jpeg_decode = "device"                  # where a JPEG input frame is decoded ("device" | "host"); `_setup` sets the instance's
    jpeg_dec = None                         # jpeg_io.HipJpegDecoder, made by the first JPEG input frame on the device
    jpeg_host_decodes = 0                   # JPEG input frames Pillow decoded on the host (no device, "host", or an unsupported file)
    _matte = None                           # the depth matte's settings (set_matte), None: off
    _matte_line = None                      # matte.MatteLine: the delayed source frames and depth planes, while a matte is set
    _matte_dev = None                       # matte.HipMatte, made by the first composited frame on the device
    _matte_skip = 0                         # frames pushed before the delay line existed: their outputs have no slot
    _lock = None                            # the colour lock's settings (set_color_lock), None: off
    _lock_dev = None                        # color_lock.HipColorLock, made by the first locked frame on the device
    _lock_state = None                      # the target state on the host route (float64 [3,2]); on the device it stays there
    _lock_ref = None                        # the moments of the reference image (mode "image")
    _lock_load = None                       # a state the device record has yet to be loaded with
    _lock_init = True                       # the next "ema" frame copies its own moments
    _lock_last = None                       # the last locked frame: what a dropped frame's repeated output reuses
    _steady = None                          # the steady mode's settings (set_steady), None: off
    _steady_dev = None                      # steady.HipSteady, made by the first steadied frame on the device
    _steady_state = None                    # (previous output, previous source bytes) on the host route; on the device it stays there
    _steady_init = True                     # the next steadied frame starts the sequence: it passes as it is
    _steady_last = None                     # the last steadied frame: what a dropped frame's repeated output reuses
    _steady_follow = None                   # the follow setting beside steady (set_steady_follow), None: the same coordinates
    _size = None                            # the output size's settings (set_output_size), None: the UNet's geometry
    _size_dev = None                        # resize.HipResize of the current size, made by the first resized frame on the device
    _size_jpeg = None                       # {(height, width): jpeg_io.HipJpegEncoder}, one per output size "jpeg" frames left at
    _matte_source = "stream"                # what the kept real part of a matted, resized frame is made of (set_matte_source)
    _camera = None                          # resize.CameraTap, while "camera", a matte and an output size are all set on the device
    _matte_up = None                        # matte.HipMatteUp of the current output size, made by the first frame that needs it
    _matte_edge = None                      # the edge-aware matte's settings (set_matte_edge), None: off
    _hold = None                            # the matte hold's settings (set_matte_hold), None: off
    _hold_dev = None                        # matte.HipMatteHold, made by the first held frame on the device
    _hold_state = None                      # (previous held plane, previous source bytes) on the host route; on the device it stays there
    _hold_init = True                       # the next held frame starts the sequence: its matte passes as it is
    _detail = None                          # the detail mode's settings (set_detail), None: off
    _detail_dev = None                      # detail.HipDetail of the current output size, made by the first frame that needs it
    _backdrop = None                        # the backdrop's settings (set_backdrop), None: the real frame stands behind the matte
    _backdrop_image = None                  # the image of an "image" backdrop, as the caller gave it
    _backdrop_dev = None                    # backdrop.HipBackdrop, made by the first frame that needs it on the device
    _backdrop_host = None                   # {(height, width, filter): uint8 frame} of the image on the host route
    _mask_input = None                      # how a mask is read (set_mask_input), None: mask_io.DEFAULTS
    _mask_tap = None                        # mask_io.HipMaskIngest (HostMaskTap on CPU tensors), made by the first mask
    _mask_sticky = None                     # the sticky mask (set_mask), as the caller gave it (an array or a tensor of its own)
    _mask_shared = None                     # ... staged for the delay line: one buffer that every frame without a mask names
    _key = None                             # the matte key's settings (set_matte_key), None: off
    _key_plate = None                       # the plate on the host, planar uint8 [3,H,W]: of an image, or captured on the host route
    _key_capture = False                    # the next composited output's source frame becomes the plate
    _key_dev = None                         # matte_key.HipMatteKey, made by the first keyed frame on the device
    _key_adapt = None                       # the adaptive plate's settings beside the key (set_matte_key_adapt), None: the plate stays
    _key_gain = None                        # the plate gain's settings beside the key (set_matte_key_gain), None: no gain is measured
    _key_gain_last = None                   # (g, n) of the last frame keyed on the host route
    _key_state = None                       # the adaptive plate on the host route, uint16 [3,H,W]; None: it starts from the plate
    _cut_settings = None                    # the cut detector's settings (set_cut_detect), None: off
    _auto_rewarm = False                    # re-warm by itself behind a cut (set_auto_rewarm)
    _rewarm_due = None                      # the count of frames entered at which the automatic re-warm runs, None: none is pending
    auto_rewarms = 0                        # automatic re-warms since `prepare`
    last_cut_record = None                  # the newest collected record, `cut.record_dict`'s dict
    depth_source = "detector"               # "input": every frame brings its own depth and no detector was built (`_setup` sets it)

    def __init__(self, config_path: str, few_step_model_type: str, num_inference_steps: int,
                 t_index_list: Optional[List[int]] = None, strength: Optional[float] = None,
                 dreambooth_path: Optional[str] = None, lora_dict: Optional[Dict[str, float]] = None, output_type: str = "pil",
                 vae_id: Optional[str] = None, device="cuda", dtype: torch.dtype = torch.float16, frame_buffer_size: int = 1,
                 width: int = 512, height: int = 512, acceleration: str = "hip", do_add_noise: bool = True,
                 device_ids: Optional[List[int]] = None, use_tiny_vae: bool = True, enable_similar_image_filter: bool = False,
                 similar_image_filter_threshold: float = 0.98, similar_image_filter_max_skip_frame: int = 10,
                 use_denoising_batch: bool = True, cfg_type: str = "none", seed: int = 42,
                 engine_dir: Optional[Union[str, Path]] = "engines", opt_unet: bool = False, frame_pipelining: bool = False,
                 jpeg_quality: int = 75, jpeg_decode: str = "device", output_size: Optional[Tuple[int, int]] = None,
                 output_resample: str = "lanczos", matte_source: str = "stream", steady: Optional[dict] = None,
                 matte_edge: Optional[dict] = None, detail: Optional[dict] = None, depth_input: Optional[dict] = None,
                 depth_source: str = "detector", backdrop: Optional[dict] = None, steady_follow: Optional[dict] = None,
                 matte_hold: Optional[dict] = None, mask_input: Optional[dict] = None, matte_key: Optional[dict] = None,
                 matte_key_adapt: Optional[dict] = None, matte_key_gain: Optional[dict] = None, keep_recent: bool = False):
        _check_depth_source(depth_source)
        self._check_keywords(few_step_model_type=few_step_model_type, acceleration=acceleration, cfg_type=cfg_type,
                             use_denoising_batch=use_denoising_batch, frame_buffer_size=frame_buffer_size, device_ids=device_ids,
                             opt_unet=opt_unet, output_type=output_type, dtype=dtype, jpeg_quality=jpeg_quality, jpeg_decode=jpeg_decode)
        cfg = load_config(config_path)
        if t_index_list is None and strength is None:
            t_index_list = cfg.get("t_index_list")
        window, sink, _ = stream_sizes(cfg)
        n = len(t_index_list) if strength is None else min(int(num_inference_steps * strength), num_inference_steps)
        pipe = load_components(cfg, height=height, width=width, denoising_steps_num=n, device=device,
                               dreambooth_path=dreambooth_path, lora_dict=lora_dict, few_step_model_type=few_step_model_type,
                               vae_id=vae_id, use_tiny_vae=use_tiny_vae, engine_dir=engine_dir, depth_source=depth_source)
        self._style_src = dict(cfg=cfg, few_step_model_type=few_step_model_type, engine_dir=engine_dir)    # what add_style builds from
        self._setup(pipe, num_inference_steps=num_inference_steps, t_index_list=t_index_list, strength=strength,
                    output_type=output_type, device=device, dtype=dtype, width=width, height=height, do_add_noise=do_add_noise,
                    seed=seed, clip_skip=(cfg.get("third_party_dict") or {}).get("clip_skip", 1), warmup_frames=sink,
                    window_size=window, frame_pipelining=frame_pipelining, enable_similar_image_filter=enable_similar_image_filter,
                    similar_image_filter_threshold=similar_image_filter_threshold,
                    similar_image_filter_max_skip_frame=similar_image_filter_max_skip_frame, jpeg_quality=jpeg_quality,
                    jpeg_decode=jpeg_decode, output_size=output_size, output_resample=output_resample, matte_source=matte_source,
                    steady=steady, matte_edge=matte_edge, detail=detail, depth_input=depth_input, depth_source=depth_source,
                    backdrop=backdrop, steady_follow=steady_follow, matte_hold=matte_hold, mask_input=mask_input, matte_key=matte_key,
                    matte_key_adapt=matte_key_adapt, matte_key_gain=matte_key_gain, keep_recent=keep_recent)

    @classmethod
    def from_components(cls, pipe, *, num_inference_steps: int, t_index_list: Optional[List[int]] = None,
                        strength: Optional[float] = None, **kw):
        """The wrapper around an already assembled `pipe` namespace (tests, synthetic weights).  Keywords: those of the
        constructor that do not name files (`jpeg_quality`, `jpeg_decode`, `output_size`, `output_resample`, `matte_source`, `steady`, `steady_follow`, `matte_edge`, `matte_hold`, `detail`, `backdrop`, `depth_input`, `mask_input`, `matte_key`, `matte_key_adapt`, `matte_key_gain`, `keep_recent` and `depth_source` among them; with `depth_source="input"` the namespace needs no `depth_model`), plus `clip_skip`, `warmup_frames`, `window_size`, `scheduler_kwargs`."""
        self = cls.__new__(cls)
        cls._check_keywords(**{k: kw.pop(k) for k in ("acceleration", "cfg_type", "use_denoising_batch", "frame_buffer_size",
                                                      "device_ids", "opt_unet", "few_step_model_type") if k in kw},
                            output_type=kw.get("output_type", "pil"), dtype=kw.get("dtype", torch.float16),
                            jpeg_quality=kw.get("jpeg_quality", 75), jpeg_decode=kw.get("jpeg_decode", "device"))
        self._setup(pipe, num_inference_steps=num_inference_steps, t_index_list=t_index_list, strength=strength, **kw)
        return self

    @staticmethod
    def _check_keywords(few_step_model_type="lcm", acceleration="hip", cfg_type="none", use_denoising_batch=True,
                        frame_buffer_size=1, device_ids=None, opt_unet=False, output_type="pil", dtype=torch.float16, jpeg_quality=75,
                        jpeg_decode="device"):
        def no(keyword, value, supported):
            raise ValueError(f"{keyword}={value!r} is not supported by the HIP backend: use {keyword}={supported}")
        if str(few_step_model_type).upper() != "LCM":
            no("few_step_model_type", few_step_model_type, "'lcm'")
        if acceleration != "hip":
            no("acceleration", acceleration, "'hip'")
        if cfg_type != "none":
            no("cfg_type", cfg_type, "'none'")
        if not use_denoising_batch:
            no("use_denoising_batch", use_denoising_batch, "True")
        if frame_buffer_size != 1:
            no("frame_buffer_size", frame_buffer_size, "1")
        if device_ids is not None:
            no("device_ids", device_ids, "None")
        if opt_unet:
            no("opt_unet", opt_unet, "False")
        if output_type not in OUTPUT_TYPES:
            no("output_type", output_type, " | ".join(repr(t) for t in OUTPUT_TYPES))
        if isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, int) or not 1 <= jpeg_quality <= 100:
            raise ValueError(f"jpeg_quality={jpeg_quality!r}: use an integer from 1 to 100")
        if jpeg_decode not in ("device", "host"):
            raise ValueError(f"jpeg_decode={jpeg_decode!r}: use 'device' or 'host'")

    def _setup(self, pipe, *, num_inference_steps, t_index_list, strength, output_type="pil", device=None, dtype=torch.float16,
               width=512, height=512, do_add_noise=True, seed=42, clip_skip=1, warmup_frames=8, window_size=16,
               scheduler_kwargs=None, frame_pipelining=False, enable_similar_image_filter=False,
               similar_image_filter_threshold=0.98, similar_image_filter_max_skip_frame=10, jpeg_quality=75, jpeg_decode="device",
               output_size=None, output_resample="lanczos", matte_source="stream", steady=None, matte_edge=None, detail=None,
               depth_input=None, depth_source="detector", backdrop=None, steady_follow=None, matte_hold=None, mask_input=None, matte_key=None,
               matte_key_adapt=None, matte_key_gain=None, keep_recent=False):
        self._check_matte_source(matte_source)
        if matte_key_gain is not None and not isinstance(matte_key_gain, dict):
            raise ValueError(f"matte_key_gain={matte_key_gain!r}: use a dict of set_matte_key_gain's keywords, or None")
        if matte_key_adapt is not None and not isinstance(matte_key_adapt, dict):
            raise ValueError(f"matte_key_adapt={matte_key_adapt!r}: use a dict of set_matte_key_adapt's keywords, or None")
        if matte_key is not None and not isinstance(matte_key, dict):
            raise ValueError(f"matte_key={matte_key!r}: use a dict of set_matte_key's keywords (with `to`), or None")
        if mask_input is not None and not isinstance(mask_input, dict):
            raise ValueError(f"mask_input={mask_input!r}: use a dict of set_mask_input's keywords, or None")
        if matte_hold is not None and not isinstance(matte_hold, dict):
            raise ValueError(f"matte_hold={matte_hold!r}: use a dict of set_matte_hold's keywords, or None")
        if backdrop is not None and not isinstance(backdrop, dict):
            raise ValueError(f"backdrop={backdrop!r}: use a dict of set_backdrop's keywords, or None")
        _check_depth_source(depth_source)
        if depth_input is not None and not isinstance(depth_input, dict):
            raise ValueError(f"depth_input={depth_input!r}: use a dict of set_depth_input's keywords, or None")
        if steady is not None and not isinstance(steady, dict):
            raise ValueError(f"steady={steady!r}: use a dict of set_steady's keywords, or None")
        if steady_follow is not None and not isinstance(steady_follow, dict):
            raise ValueError(f"steady_follow={steady_follow!r}: use a dict of set_steady_follow's keywords, or None")
        if matte_edge is not None and not isinstance(matte_edge, dict):
            raise ValueError(f"matte_edge={matte_edge!r}: use a dict of set_matte_edge's keywords, or None")
        if detail is not None and not isinstance(detail, dict):
            raise ValueError(f"detail={detail!r}: use a dict of set_detail's keywords, or None")
        self.sd_turbo = False
        self.device = pipe.device if device is None else device
        self.dtype, self.width, self.height = dtype, width, height
        self.output_type = output_type
        self.jpeg_quality = jpeg_quality
        self.jpeg = None                    # jpeg_io.HipJpegEncoder, made by the first "jpeg" frame on the device
        self.jpeg_decode = jpeg_decode
        if output_type == "jpeg":
            from . import jpeg
            jpeg._check(height, width, jpeg_quality)       # a size that is no multiple of 16 is refused here, not at the first frame
        if output_size is not None:                        # (and an output size nobody serves, likewise)
            if not isinstance(output_size, (tuple, list)) or len(output_size) != 2:
                raise ValueError(f"output_size={output_size!r}: use (height, width) or None")
            self.set_output_size(*output_size, resample=output_resample)
        self.frame_buffer_size = 1
        self.use_denoising_batch = True
        self.seed = seed
        self.frame_pipelining = frame_pipelining
        self.stream = StreamAnimateDiffusionDepth(pipe, num_inference_steps=num_inference_steps, t_index_list=t_index_list,
                                                  strength=strength, torch_dtype=dtype, width=width, height=height,
                                                  do_add_noise=do_add_noise, frame_buffer_size=1, use_denoising_batch=True,
                                                  cfg_type="none", clip_skip=clip_skip, warmup_frames=warmup_frames,
                                                  window_size=window_size, scheduler_kwargs=scheduler_kwargs,
                                                  keep_recent=keep_recent)
        self.batch_size = len(self.stream.t_list)
        self.stream.load_warmup_unet(None)
        self.stream.prepare_cache(height=height, width=width, denoising_steps_num=self.batch_size)
        if enable_similar_image_filter:
            self.stream.enable_similar_image_filter(similar_image_filter_threshold, similar_image_filter_max_skip_frame)
        self.io = None
        if torch.device(self.device).type == "cuda" and not ops.DRY_RUN:
            from .frame_io import FrameProcessor, HipFrameIO
            self.io = HipFrameIO(height, width, device=pipe.device)
            self.stream.image_processor = FrameProcessor(self.io)
        self._init_styles(pipe)
        self._init_cut_detect()
        self.set_matte_source(matte_source)
        if steady is not None:
            self.set_steady(**steady)
        if steady_follow is not None:
            self.set_steady_follow(**steady_follow)
        if matte_edge is not None:
            self.set_matte_edge(**matte_edge)
        if matte_hold is not None:
            self.set_matte_hold(**matte_hold)
        if detail is not None:
            self.set_detail(**detail)
        if backdrop is not None:
            self.set_backdrop(**backdrop)
        self.depth_source = depth_source
        if depth_source == "input":
            self.stream.depth_detector = None      # (a `pipe` that brought one: it is never called)
        if depth_input is not None:
            self.set_depth_input(**depth_input)
        if mask_input is not None:
            self.set_mask_input(**mask_input)
        if matte_key is not None:
            if "to" not in matte_key:
                raise ValueError(f"matte_key={matte_key!r}: the dict needs `to` (a colour, an image or 'capture')")
            self._set_matte_key(**matte_key, needs_matte=False)      # (no matte can be set yet: the key waits for the first set_matte)
        if matte_key_adapt is not None:
            self.set_matte_key_adapt(**matte_key_adapt)
        if matte_key_gain is not None:
            self.set_matte_key_gain(**matte_key_gain)

    # ------------------------------------------------------------------ depth from the caller (depth_io.py)
    @property
    def depth_input(self) -> dict:
        """how a `depth=` frame is read, as {kind, invalid, range}"""
        return dict(self.stream.depth_input)

    def set_depth_input(self, kind: str = "distance", invalid=0, range=None) -> None:
        """How the depth frames handed in with `depth=` are read.  `kind="distance"`: metric samples, larger = farther (an RGB-D
        camera's millimetres); `kind="inverse"`: MiDaS's convention, larger = nearer (another monocular estimator's output).
        `invalid`: the sample value that marks a hole (0 for most depth cameras), or None: every value counts; non-finite
        floats, and distances that are not positive, are holes always.  Holes smaller than the resampling filter's footprint
        are filled by their valid neighbours; larger ones count as the farthest.  `range=None`: every frame (and the warm-up
        batch of `prepare`, jointly) is normalised by its own nearest and farthest pixel, as the detector's map is;
        `range=(near, far)` for "distance" -- `far` may be inf -- or `(lo, hi)` for "inverse", in the units of the samples: a
        fixed range, so the map does not pump when something walks into view.  Without a range a frame whose own range is within
        2^-14 of its nearest value counts as flat (all farthest: that is rounding noise of the resampling, not depth); a fixed
        range is taken at its word however narrow.  May be called before or after `prepare` and
        between any two frames: the settings apply from the next frame."""
        from .depth_io import check_settings
        self.stream.depth_input = check_settings(kind, invalid, range)

    def _depth_arg(self, depth, where: str = "depth"):
        """a `depth=` argument as the pipeline takes it: arrays and tensors pass (host or device), a PIL image of mode "I;16", "I",
        "F" or "L" -- or a path to one -- becomes its uint16 / float32 array.  None under `depth_source="input"` raises."""
        if depth is None:
            if self.depth_source == "input":
                raise ValueError(f"{where}: this wrapper was built with depth_source='input': every frame needs its depth")
            return None
        if isinstance(depth, (str, os.PathLike)):
            from PIL import Image
            depth = Image.open(depth)
        if hasattr(depth, "mode") and hasattr(depth, "convert"):
            if depth.mode not in ("I;16", "I;16L", "I;16B", "I", "F", "L"):
                raise ValueError(f"{where}: a depth image must have mode 'I;16', 'I', 'F' or 'L', got {depth.mode!r}")
            arr = np.array(depth)
            if depth.mode == "I":              # (how some Pillow versions open a 16-bit PNG)
                if arr.min() < 0 or arr.max() > 65535:
                    raise ValueError(f"{where}: a mode 'I' depth image must hold 16-bit samples, 0..65535 (got {int(arr.min())}.."
                                     f"{int(arr.max())}): hand wider data in as a float32 array")
                arr = arr.astype(np.uint16)
            elif arr.dtype not in (np.uint8, np.float32):
                arr = arr.astype(np.uint16)
            return arr
        return depth

    # ------------------------------------------------------------------ the matte from the caller (mask_io.py)
    @property
    def mask_input(self) -> dict:
        """how a mask is read, as {combine, invert}"""
        from .mask_io import DEFAULTS
        return dict(self._mask_input or DEFAULTS)

    def set_mask_input(self, combine: str = "replace", invert: bool = False) -> None:
        """How the masks handed in with `mask=` (and the sticky mask of `set_mask`) cut the frame.  `combine="replace"`: the mask
        alone is the raw matte, and the matte's `lo`, `hi` and `keep` are not read; "and": the smaller of the depth ramp and
        the mask (the person, but only in front of the wall); "or": the larger.  `invert` flips the mask first.  Read when a
        frame is composited: it applies from the next output on.  May be called before or after `set_matte` and `prepare` and
        between any two frames."""
        from .mask_io import check_settings
        self._mask_input = check_settings(combine, invert)
        self._hold_init = True             # (a held matte starts again from the new raw matte)

    @property
    def mask(self) -> bool:
        """is a sticky mask set (`set_mask`)?"""
        return self._mask_sticky is not None

    def set_mask(self, mask) -> None:
        """A sticky mask: the mask of every frame that brings none of its own -- a fixed region ("only the window").  What
        `img2img`'s `mask=` takes; needs a matte (`set_matte`), and is kept as a copy of the caller's.  It joins each frame as
        the frame enters, so it reaches the output with that frame, N - 1 frames on."""
        from . import mask_io
        if self._matte is None:
            raise ValueError("set_mask: a mask needs a matte: call set_matte first (its feather, show and keep act on the mask)")
        if self._key is not None:
            raise ValueError("set_mask: a mask and a matte key exclude each other: call clear_matte_key first")
        m = mask_io.load(mask, "set_mask")
        m = mask_io._torch_mask(m).clone() if torch.is_tensor(m) and m.is_cuda else mask_io._as_mask(m).copy()
        mask_io.tables(m.shape[0], m.shape[1], self.height, self.width)
        self._mask_sticky, self._mask_shared = m, None

    def clear_mask(self) -> None:
        """No sticky mask: a frame that brings no mask is cut by the depth ramp alone again (frames already in the stream keep
        the mask they entered with)."""
        self._mask_sticky = self._mask_shared = None

    def _mask_begin(self, mask, where: str = "mask") -> None:
        """In front of every frame, beside `_camera_begin`: a raw mask nobody claimed belongs to no later frame; the frame's own
        mask, or the sticky one, is copied into a pooled device buffer on the caller's stream and offered to the delay line,
        whose tap moves it into the frame's slot."""
        tap = self._mask_tap
        if tap is not None:
            tap.begin()
        if mask is not None and self._matte is None:
            raise ValueError(f"{where}: a mask needs a matte: call set_matte first (its feather, show and keep act on the mask)")
        if mask is not None and self._key is not None:
            raise ValueError(f"{where}: a mask and a matte key exclude each other: call clear_matte_key first")
        sticky = mask is None
        if sticky:
            mask = self._mask_sticky
        if mask is None or self._matte is None:
            return
        from . import mask_io
        if tap is None:
            tap = (mask_io.HipMaskIngest(self.height, self.width, device=self.io.device) if self.io is not None
                   else mask_io.HostMaskTap(self.height, self.width))
            self._mask_tap = self._matte_line.mask_source = tap
        if not sticky:
            tap.offer(mask_io.load(mask, where))
        elif isinstance(tap, mask_io.HostMaskTap):
            tap.pending = self._mask_sticky
        else:
            if self._mask_shared is None:
                self._mask_shared = tap.stage(self._mask_sticky, shared=True)
            tap.offer(self._mask_shared)

    def _mask_front(self, slot):
        """`(record, keep, plane)` of L2D_OP_MASK_INGEST for the slot's mask under the settings of this moment, or None"""
        if slot is None or getattr(slot, "mask", None) is None or self._mask_tap is None:
            return None
        op, keep = self._mask_tap.record(slot.mask, slot.depth, self._matte, self.mask_input)
        return op, keep, self._mask_tap.plane

    def _mask_plane(self, slot) -> Optional[np.ndarray]:
        """the raw matte of the slot's mask on the host route, fp32 [H,W]: `mask_io.raw_ref` where op 58 would run; or None"""
        if slot is None or getattr(slot, "mask", None) is None:
            return None
        from .mask_io import raw_ref
        return raw_ref(slot.mask, slot.depth[None], self._matte, self.mask_input, self.height, self.width)


    # ------------------------------------------------------------------ matte key (matte_key.py)
    @property
    def matte_key(self) -> Optional[dict]:
        """the current matte key as {to, lo, hi, luma, radius, combine, invert}, or None; `to` is the (r, g, b) of a colour key,
        "plate" (an image, or a captured frame) or "capture" (until the capture has happened)"""
        if self._key is None:
            return None
        return dict(self._key, to="capture" if self._key_capture else self._key["to"])

    def set_matte_key(self, to, *, lo=None, hi=None, luma=None, radius: int = 1, combine: str = "replace", invert: bool = False) -> None:
        """Cut the frame by a colour or by a clean plate: the third source of a matte beside the depth ramp and a caller's mask.
        Every pixel of the frame's source is compared, on the bytes a viewer would see, with the key (`matte_key.key_ref`);
        where it differs is the subject, which the matte stylises (`keep` is not read under "replace"; `invert` flips the key).
        `to`: an `(r, g, b)` triple of bytes -- a green or blue screen; an image (a uint8 [H,W,3] array, a PIL image or a
        path, decoded here: a file that is no image raises ValueError now) -- a picture of the empty room taken by a camera
        that does not move, cropped and resampled to the stream's size with the output size's filter
        (`matte_key.plate_ref`); or "capture": the source frame of the next composited output becomes the plate -- what the
        viewer sees at that moment --, and `matte_key["to"]` reads "plate" from then on (that one frame is keyed against
        itself).  `lo`, `hi` (0..1024, byte levels of the colour distance averaged over a (2 `radius` + 1)^2 window, `radius`
        0..4): at or below `lo` a pixel is the key's, at or above `hi` the subject's, a smoothstep between; `luma` (0..1):
        how much a difference in brightness counts -- 0 ignores it, so a shadow on the screen stays screen.  None takes the
        defaults, lo=40, hi=90, luma=0 for a colour and 0.25 for a plate: a guess, not tuned on camera footage.  `combine`:
        "replace" (the key alone; depth is not read), "and" (the smaller of the depth ramp and the key: the screen, but only
        what is nearer than the wall), "or" (the larger).

        A setting beside the matte, like `set_matte_edge`: it needs a matte (`set_matte`), acts on its output types, and
        `clear_matte` clears it.  The key is formed of the frame's own source out of the delay line, so it reaches the output
        with its frame; edge refit, hold, feather, backdrop, `show` and `set_matte_source("camera")` act on it as on the ramp.
        One more launch on the device at the head of the composite's list (two on a capturing frame), no synchronisation.  A
        frame the near-duplicate filter repeats is keyed again from the same slot.  A key and a caller's mask exclude each
        other.  May be called between any two frames; the change applies from the next output and restarts a matte hold.  The
        constructor's `matte_key=` (a dict of these keywords, `to` among them) is set before any matte can be: it waits for
        the first `set_matte`.  A plate is a frozen picture: `set_matte_key_adapt` lets it follow drifting light (and then
        refuses a colour here)."""
        self._set_matte_key(to, lo=lo, hi=hi, luma=luma, radius=radius, combine=combine, invert=invert)

    def _set_matte_key(self, to, lo=None, hi=None, luma=None, radius=1, combine="replace", invert=False, needs_matte=True) -> None:
        from . import matte_key as MK
        if needs_matte and self._matte is None:
            raise ValueError("set_matte_key: a key needs a matte: call set_matte first (its feather, show and keep act on the key)")
        if self._mask_sticky is not None:
            raise ValueError("set_matte_key: a matte key and a mask (set_mask) exclude each other: call clear_mask first")
        capture = isinstance(to, str) and to == "capture"
        color = MK.is_color(to)
        if isinstance(to, (tuple, list)) and not color:
            MK.check_color(to)
        if color and self._key_adapt is not None:
            raise ValueError(f"set_matte_key: to={to!r}: the adaptive plate (set_matte_key_adapt) needs a plate, not a colour: call "
                             "clear_matte_key_adapt first")
        if color and self._key_gain is not None:
            raise ValueError(f"set_matte_key: to={to!r}: the plate gain (set_matte_key_gain) needs a plate, not a colour: call "
                             "clear_matte_key_gain first")
        settings = MK.check_settings(lo, hi, luma, radius, combine, invert, plate=not color)
        plate = None
        if color:
            settings["to"] = MK.check_color(to)
        else:
            settings["to"] = "plate"
            if not capture:
                if to is None or isinstance(to, (bool, int, float)):
                    raise ValueError(f"matte key: to={to!r}: use an (r, g, b) triple, an image (an array, a PIL image or a path) or 'capture'")
                if torch.is_tensor(to):
                    to = to.detach().cpu().numpy()
                plate = MK.plate_ref(to, self.height, self.width, self._backdrop_filter())        # (decoded now: a bad file is refused here)
        self._key, self._key_capture, self._key_plate = settings, capture, plate
        if self._key_dev is not None and plate is not None:
            self._key_dev.set_plate(plate)
        self._restart_key_state()          # (a new image or a new capture: the adaptive plate starts from it)
        self._hold_init = True             # (a held matte starts again from the new raw matte)

    def capture_matte_plate(self) -> None:
        """Take the plate again: the source frame of the next composited output becomes it; the key's other settings stay."""
        if self._key is None:
            raise ValueError("capture_matte_plate: no matte key is set: call set_matte_key('capture') first")
        self._key = dict(self._key, to="plate")          # (a colour key becomes a plate key; its lo, hi and luma are kept as they are)
        self._key_capture, self._key_plate = True, None
        self._hold_init = True

    def clear_matte_key(self) -> None:
        """No key: the frame is cut by the depth ramp alone again; no launch or buffer of the key is left in the frame's path.
        The adaptive plate (`set_matte_key_adapt`) and the plate gain (`set_matte_key_gain`) go with it."""
        self._key = self._key_plate = self._key_dev = None
        self._key_adapt = self._key_state = None
        self._key_gain = self._key_gain_last = None
        self._key_capture = False
        self._hold_init = True

    # ------------------------------------------------------------------ the adaptive plate (matte_key.py)
    @property
    def matte_key_adapt(self) -> Optional[dict]:
        """the adaptive plate's settings as {rate, absorb}, or None"""
        return None if self._key_adapt is None else dict(self._key_adapt)

    def set_matte_key_adapt(self, rate: float = 1.0 / 32.0, absorb: float = 0.0) -> None:
        """Let the plate of a matte key follow drifting light.  A plate is a frozen picture of the empty room: a cloud, a lamp
        warming up or a camera's exposure settling moves every background pixel off it, and once the distance passes `lo` the
        whole wall turns into subject.  With this setting the plate moves after every keyed frame towards that frame's source
        (`matte_key.key_adapt_ref`): by `rate` of the way where the key says background, by `absorb` of the way where it says
        subject, in between under a soft key.  Both lie in [0, 0.5].  `absorb=0` never takes the subject into the plate, and
        something that is put down and left there stays subject for good; a small `absorb` lets it sink into the background
        in about 1 / `absorb` frames -- and a person who sits still with it.  The defaults, 1 / 32 and 0, are a guess, not
        tuned on camera footage.  The plate is kept in 8.8 fixed point, so that a slow rate does move it.

        A setting beside the key, like `set_steady_follow` beside `set_steady`: it needs a key against a plate
        (`set_matte_key` with an image or "capture"), a colour key refuses it, and `clear_matte_key` and `clear_matte` clear
        it.  On the device one launch (L2D_OP_MATTE_KEY_ADAPT) takes the key's place in the composite's list; it writes the
        key's plane as before, so everything behind it is unchanged.  A frame the near-duplicate filter repeats is keyed again
        but does not move the plate.  A new image or a new capture starts the plate again; a change of the rates does not.
        `matte_key_plate()` returns the plate of this moment.  May be called between any two frames; the change applies from
        the next output and restarts a matte hold."""
        from .matte_key import check_adapt
        settings = check_adapt(rate, absorb)
        if self._key is None:
            raise ValueError("set_matte_key_adapt: the adaptive plate needs a matte key against a plate: call set_matte_key with an image "
                             "or 'capture' first")
        if not isinstance(self._key["to"], str):
            raise ValueError(f"set_matte_key_adapt: the key is the colour {self._key['to']!r}: adaptation needs a plate (set_matte_key with "
                             "an image or 'capture')")
        if self._key_adapt is None:
            self._restart_key_state()      # (switched on: the plate of the key, not what an earlier run left)
        self._key_adapt = settings
        self._hold_init = True

    def clear_matte_key_adapt(self) -> None:
        """The plate stays as it was set or captured again: the key's own launch, and no buffer of the adaptive plate in the
        frame's path."""
        self._key_adapt = None
        self._restart_key_state()
        self._hold_init = True

    def _restart_key_state(self) -> None:
        self._key_state = None
        if self._key_dev is not None:
            self._key_dev.restart()

    def matte_key_plate(self) -> np.ndarray:
        """The plate of this moment as uint8 [H,W,3]: the adaptive plate's bytes (`matte_key.plate_bytes` of its state) while
        one runs, else the plate as it was set or captured.  On the device a copy to the host that waits for the stream.
        ValueError without a plate: no key, a colour key, or a capture that has not happened yet."""
        if self._key is None or not isinstance(self._key["to"], str):
            raise ValueError("matte_key_plate: no matte key against a plate is set")
        if self._key_dev is not None and self._key_dev.has_plate and not self._key_capture:
            return self._key_dev.current_plate()
        if self._key_state is not None:
            from .matte_key import plate_bytes
            return np.ascontiguousarray(plate_bytes(self._key_state).transpose(1, 2, 0))
        if self._key_plate is None or self._key_capture:
            raise ValueError("matte_key_plate: no plate yet: the capture waits for the next composited output")
        return np.ascontiguousarray(np.asarray(self._key_plate).transpose(1, 2, 0))

    # ------------------------------------------------------------------ the plate gain (matte_key.py)
    @property
    def matte_key_gain(self) -> Optional[dict]:
        """the plate gain's settings as {limit, min_share}, or None"""
        return None if self._key_gain is None else dict(self._key_gain)

    def set_matte_key_gain(self, limit: float = 2.0, min_share: float = 1.0 / 16.0) -> None:
        """Let the key against a plate follow a sudden exposure or white-balance step.  A person walks in and the camera's
        auto-exposure and auto-white-balance move every background pixel at once; the plate is wrong everywhere, and the
        adaptive plate follows only at its `rate` (and with `absorb=0` not at all where the wall has already turned subject).
        With this setting every keyed frame first measures one gain per channel between the plate and the frame's source --
        the lower median of the per-pixel ratios, in units of 1 / 128 (`matte_key.gain_hist_ref`, `gain_of`) -- and is keyed
        against the plate times that gain (`gain_plate`).  `limit` in [1, 3.99] bounds the gain to [1 / limit, limit];
        a channel with fewer valid samples (neither clipped nor near black) than `min_share` of the frame's pixels keeps a
        gain of 1.  The median holds while the subject covers less than half of the valid samples: past that the gains are
        the subject's, and the key is wrong.  The defaults are a guess, not tuned on camera footage.

        A setting beside the key, like `set_matte_key_adapt`, with or without it: it needs a key against a plate, a colour
        key refuses it, and `clear_matte_key` and `clear_matte` clear it.  Under the adaptive plate the plate still moves
        towards the frame's own bytes, so it absorbs the new exposure at `rate` and the measured gain walks back to 1.  On
        the device two launches (L2D_OP_MATTE_KEY_GAIN_HIST, L2D_OP_MATTE_KEY_GAIN) stand in front of the key's, which reads
        their record; nothing is carried from frame to frame.  `matte_key_gain_measured()` returns the last measurement.
        May be called between any two frames; the change applies from the next output and restarts a matte hold."""
        from .matte_key import check_gain
        settings = check_gain(limit, min_share)
        if self._key is None:
            raise ValueError("set_matte_key_gain: the plate gain needs a matte key against a plate: call set_matte_key with an image or "
                             "'capture' first")
        if not isinstance(self._key["to"], str):
            raise ValueError(f"set_matte_key_gain: the key is the colour {self._key['to']!r}: a gain needs a plate (set_matte_key with an "
                             "image or 'capture')")
        self._key_gain = settings
        self._hold_init = True

    def clear_matte_key_gain(self) -> None:
        """No gain is measured: the key's own launch against the plate as it is, and no buffer of the gain in the frame's path."""
        self._key_gain = self._key_gain_last = None
        if self._key_dev is not None:
            self._key_dev.has_gain = False
        self._hold_init = True

    def matte_key_gain_measured(self):
        """The last keyed frame's measurement as `((g_r, g_g, g_b), (n_r, n_g, n_b))`: the gains as factors (g / 128) and the
        valid samples as shares of the frame's pixels (n / H W).  On the device a copy to the host that waits for the stream.
        ValueError while nothing has been measured."""
        if self._key_gain is None:
            raise ValueError("matte_key_gain_measured: no plate gain is set (set_matte_key_gain)")
        if self._key_dev is not None and self._key_dev.has_gain:
            g, n = self._key_dev.current_gain()
        elif self._key_gain_last is not None:
            g, n = self._key_gain_last
        else:
            raise ValueError("matte_key_gain_measured: no frame has been keyed yet")
        hw = float(self.height * self.width)
        return tuple(float(v) / 128.0 for v in g), tuple(float(v) / hw for v in n)

    def _key_front(self, slot, device, repeated: bool = False):
        """`(records, keep, plane)` of L2D_OP_MATTE_KEY for the slot's source under the settings of this moment (on a capturing
        frame L2D_OP_FRAME_PLANAR_BYTES in front of it), or None; with an adaptive plate L2D_OP_MATTE_KEY_ADAPT in its place"""
        if slot is None or self._key is None or self._matte is None:
            return None
        if self._key_dev is None:
            from .matte_key import HipMatteKey
            self._key_dev = HipMatteKey(self.height, self.width, device=device)
            if self._key_plate is not None:
                self._key_dev.set_plate(self._key_plate)
        capture, self._key_capture = self._key_capture, False
        more = {} if self._key_gain is None else dict(gain=self._key_gain)     # (the keyword only with a gain)
        if self._key_adapt is None:
            return self._key_dev.record(slot, self._matte, self._key, capture=capture, **more)        # (the parent's call)
        return self._key_dev.record(slot, self._matte, self._key, capture=capture, adapt=self._key_adapt, repeated=repeated, **more)

    def _key_plane(self, slot, repeated: bool = False) -> Optional[np.ndarray]:
        """the raw matte of the key on the host route, fp32 [H,W]: `matte_key.raw_ref` where op 59 would run (`raw_adapt_ref`
        where op 61 would, on a uint16 state kept here); or None"""
        if slot is None or self._key is None or self._matte is None:
            return None
        from .matte_key import raw_ref
        from .steady import source_bytes
        if self._key_capture:
            self._key_capture, self._key_plate = False, source_bytes(slot.source)
            self._key_state = None
        more = {}                           # (the keyword only with a gain: without one the calls are the parent's)
        if self._key_gain is not None:
            from .matte_key import gain_params, measure_gain, plate_bytes
            if self._key_plate is None:
                raise ValueError("matte key: no plate is set")
            k = self._key_plate if self._key_adapt is None or self._key_state is None else plate_bytes(self._key_state)
            self._key_gain_last = measure_gain(source_bytes(slot.source), k, *gain_params(self._key_gain["limit"], self._key_gain["min_share"],
                                                                                         self.height, self.width))
            more["gain"] = self._key_gain_last[0]
        if self._key_adapt is not None:
            from .matte_key import raw_adapt_ref, state_of
            if self._key_plate is None:
                raise ValueError("matte key: no plate is set")
            state = state_of(self._key_plate) if self._key_state is None else self._key_state
            raw, self._key_state = raw_adapt_ref(slot.source, state, slot.depth[None], self._matte, self._key,
                                                 dict(rate=0.0, absorb=0.0) if repeated else self._key_adapt, **more)
            return raw
        key = self._key["to"]
        if isinstance(key, str):
            if self._key_plate is None:
                raise ValueError("matte key: no plate is set")
            key = self._key_plate
        return raw_ref(slot.source, key, slot.depth[None], self._matte, self._key, **more)

    # ------------------------------------------------------------------ depth matte (matte.py)
    @property
    def matte(self) -> Optional[dict]:
        """the current matte as {lo, hi, keep, feather, show}, or None"""
        return None if self._matte is None else dict(self._matte)

    def set_matte(self, lo: float, hi: float, *, keep: str = "near", feather: int = 0, show: bool = False) -> None:
        """Stylise one side of a depth ramp only: the output frame becomes `source + m (styled - source)` with m a smoothstep of
        the frame's own normalised inverse depth (0 = the farthest point of the frame, 1 = the nearest) from `lo` to `hi`;
        `keep="near"` stylises the near side and keeps the real far side, `keep="far"` the other way round; `feather` (0..8) is
        the radius of a box blur of the matte in pixels; `show=True` returns the matte itself as a grey frame (to choose `lo`
        and `hi` by eye).  One launch on the device in place of the egress launch ("u8", "pil"), or in front of the JPEG
        encoder ("jpeg"); the float output types are not served.  May be called before or after `prepare` and between any two
        frames: settings change with the next output; turning the matte on mid-stream starts the delay line (matte.MatteLine)
        with the next frame, and outputs of frames it has not seen are composited with the oldest frame it has.  The frames
        `prepare` returns are not composited.  The kept real part is the stream-sized source frame, also under an output size;
        `set_matte_source("camera")` keeps the camera's own pixels there instead."""
        from .matte import SERVED_OUTPUT_TYPES, check_settings
        self._check_served(SERVED_OUTPUT_TYPES, "composited", "clear_matte")
        settings = check_settings(lo, hi, keep=keep, feather=feather, show=show)
        self._need_line()
        self._matte = settings
        self._hold_init = True             # (a new ramp or a `keep` flip must not linger in a held matte)
        self._sync_camera()

    def clear_matte(self) -> None:
        """Back to the plain output route: no launch, copy or buffer of the matte is left in the frame's path, the camera
        buffers of `set_matte_source("camera")` included.  (A colour lock to "source" keeps the delay line it shares with the
        matte.)"""
        self._matte = self._matte_dev = self._matte_up = None
        self._hold_dev = self._hold_state = None
        self._hold_init = True
        self._mask_tap = self._mask_sticky = self._mask_shared = None      # (a mask needs a matte: none outlives it)
        self.clear_matte_key()                                             # (and so does a key)
        if self._matte_line is not None:
            self._matte_line.mask_source = None
            self._matte_line.drop_masks()
        self._release_line()
        self._sync_camera()

    # ------------------------------------------------------------------ matte at the output size
    @property
    def matte_source(self) -> str:
        """"stream" or "camera": what the kept real part of a matted frame is made of under an output size"""
        return self._matte_source

    @staticmethod
    def _check_matte_source(source) -> None:
        if source not in ("stream", "camera"):
            raise ValueError(f"matte_source={source!r}: use 'stream' or 'camera'")

    def set_matte_source(self, source: str) -> None:
        """What a matte keeps real when an output size is set.  "stream" (the default): the stream-sized source frame, composited
        at the stream's size and resampled with the rest of the picture.  "camera": the camera frame's own pixels -- the window
        of the uint8 frame the ingest looks at (`resize.camera_box`, rounded to whole source pixels), resampled to the output
        size with the output size's filter as the frame is ingested, and composited there with the matte sampled bilinearly
        (`matte.composite_up_ref`); with `keep="far"` and a 1080-line camera the person is the camera's person, not 512 lines
        scaled up.  The order on a frame stays colour lock, matte, size: the two stages become the resize of the styled frame and
        one composite launch at the output size.

        "camera" acts on an output frame only when a matte and an output size are both set, the frame runs on the device
        route, and the frame it is paired with came in as a uint8 frame or a JPEG file while all that held (the delay line's
        slot then carries its pixels).  Every other frame takes the "stream" route unchanged -- float tensors, PIL images and
        paths (they reach the stream at its own size: there is no camera frame), frames that entered before the mode, the matte
        or the current output size was set, and the host route without a device.  That is the behaviour, not an error.  A camera
        geometry whose window the output size does not serve (a ratio outside 1/2 .. 8) raises ValueError from the frame that
        first meets it.  May be called before or after `prepare` and between any two frames."""
        self._check_matte_source(source)
        self._matte_source = source
        self._sync_camera()

    # ------------------------------------------------------------------ edge-aware matte
    @property
    def matte_edge(self) -> Optional[dict]:
        """the current edge setting as {radius, eps}, or None"""
        return None if self._matte_edge is None else dict(self._matte_edge)

    def set_matte_edge(self, radius: int = 4, eps: float = 10.0) -> None:
        """Refine the matte by the frame it cuts.  The depth map is soft and its edges sit a few pixels beside the object's;
        with this setting the matte (ramp and `keep` applied, in front of the feather) is re-fitted in every (2 radius + 1)^2
        window as a linear function of the source frame's luma -- a guided filter, `matte.edge_ref` --, so that its edges land
        where the frame's own edges are.  `radius` 1..8 pixels: how far an edge may move; `eps` >= 1 in byte levels: the
        contrast of the frame below which a window counts as flat and the matte is only smoothed there.  An all-near or
        all-far matte stays exactly that.  A setting beside the matte, like `set_matte_source`: it acts only while a matte is
        set, on its output types, and `matte` keeps its five keys.  One more launch on the device in front of the composite's,
        no synchronisation; `feather` and `show` apply to the refined matte; with `set_matte_source("camera")` the matte is
        refined at the stream's size by the stream-sized source frame and then sampled at the output size as before.  A frame
        the near-duplicate filter repeats is refined again from the same slot: the same bytes.  May be called before or after
        `prepare` and between any two frames; the change applies from the next output."""
        from .matte import check_edge
        self._matte_edge = check_edge(radius, eps)
        self._hold_init = True             # (a held matte starts again from the refined one)

    def clear_matte_edge(self) -> None:
        """Back to the matte as the depth map gives it: no launch or buffer of the refinement is left in the frame's path."""
        self._matte_edge = None
        self._hold_init = True
        for dev in (self._matte_dev, self._matte_up):
            if dev is not None:
                dev.edge = None

    # ------------------------------------------------------------------ matte hold
    @property
    def matte_hold(self) -> Optional[dict]:
        """the current matte hold as {lo, hi, strength, radius, search, bias}, or None"""
        return None if self._hold is None else dict(self._hold)

    def set_matte_hold(self, lo: float = 2.0, hi: float = 10.0, *, strength: float = 0.8, radius: int = 2, search: int = 0,
                       bias: int = 256) -> None:
        """Keep the matte still where the camera is still.  The matte is a fresh draw in every frame -- a smoothstep over that
        frame's depth map, normalised on that frame alone --, so the silhouette between the real and the styled part crawls by
        a few pixels while nothing moves.  With this setting the matte in front of the feather (ramp and `keep` applied, refined
        by `set_matte_edge` when that is set) is blended per pixel with the previous held matte by steady's measure of where
        the source moved (`matte.hold_ref`): `lo`, `hi` (byte levels of the source's motion averaged over a (2 `radius` + 1)^2
        window, `radius` 0..8) and `strength` (0..1) mean what they mean in `set_steady`; where the source moved, and on a
        hard cut, the frame's own matte passes untouched.  `search` 1..8 lets it look where each 8 x 8 block of the source came
        from (`set_steady_follow`'s search, with `bias`), so that it also holds under a moving camera; 0 compares the same
        coordinates.  The defaults are steady's: nobody has tuned them on camera footage.

        A setting beside the matte, like `set_matte_edge`: it acts only while a matte is set, on its output types, and `matte`
        keeps its five keys.  The order on a frame is ramp or edge, hold, then feather and composite; `show` shows the held
        matte, `set_matte_source("camera")` samples the held plane as it samples the edge plane, and the backdrop's blur
        keeps weighing by the raw matte of the frame.  One more launch on the device in front of the composite's (two with
        `search`), in the same run, no synchronisation.  The hold advances once per composited frame, in output order; a frame
        the near-duplicate filter repeats is composited with the last held matte and moves nothing.  `prepare`, every
        `set_matte` call, `set_matte_edge` and `clear_matte_edge` start the sequence again with the next frame; changing
        these settings mid-stream does not.  With `search` it runs its own motion search against its own previous frame
        (steady's field is not shared: the two sequences may have started at different frames).  May be called before or
        after `set_matte` and `prepare` and between any two frames."""
        from .matte import check_hold
        settings = check_hold(lo, hi, strength, radius, search, bias)
        if self._hold is None:
            self._hold_init = True
        self._hold = settings

    def clear_matte_hold(self) -> None:
        """Back to the matte of each frame alone: no launch or buffer of the hold is left in the frame's path."""
        self._hold = self._hold_dev = self._hold_state = None
        self._hold_init = True

    def _hold_step(self, device, repeated: bool):
        """the `hold=` of the device composites for this frame (`matte.HoldStep`); the sequence has started behind it"""
        from .matte import HipMatteHold, HoldStep
        if self._hold_dev is None:
            self._hold_dev = HipMatteHold(self.height, self.width, device=device)
            self._hold_init = True
        step = HoldStep(self._hold_dev, self._hold, self._hold_init, repeated and not self._hold_init)
        self._hold_init = False
        return step

    def _held_plane(self, slot, repeated: bool, raw: Optional[np.ndarray] = None) -> np.ndarray:
        """the held matte of this frame on the host route, fp32 [1,H,W]: `hold_ref` where op 57 would run.  `raw`: the raw matte
        of the slot's mask in place of the ramp (`_mask_plane`)."""
        from .matte import edge_ref, hold_ref, matte_ref
        if repeated and not self._hold_init and self._hold_state is not None:
            return self._hold_state[0][None]
        mt = self._matte
        if raw is not None:
            m0 = raw if self._matte_edge is None else edge_ref(raw, slot.source, **self._matte_edge)
        else:
            m0 = matte_ref(slot.depth[None], mt["lo"], mt["hi"], 0, mt["keep"], edge=self._matte_edge,
                           source=slot.source[None] if self._matte_edge is not None else None)[0]
        init = self._hold_init or self._hold_state is None
        h, self._hold_state, _ = hold_ref(m0, slot.source, self._hold_state, **self._hold, init=init)
        self._hold_init = False
        return h[None]

    # ------------------------------------------------------------------ backdrop (backdrop.py)
    @property
    def backdrop(self) -> Optional[dict]:
        """the current backdrop as {to: "blur" | "color" | "image", radius, passes, color}, or None"""
        return None if self._backdrop is None else dict(self._backdrop)

    def set_backdrop(self, to="blur", *, radius: int = 6, passes: int = 3, color=None) -> None:
        """What stands behind the matte, in place of the real frame.  `to="blur"`: the room blurred ("portrait mode") -- the
        frame's own source, blurred `passes` (1..3) times by a (2 `radius` + 1)^2 box (1..8) in which the matte's subject
        counts 1/256 of a background pixel, so its colours do not bleed into the room around the silhouette
        (`backdrop.blur_ref`); an `(r, g, b)` triple of bytes: that colour, for a chroma key further down (also
        `to="color", color=(r, g, b)`, the form the `backdrop` property has); an image -- a uint8 [H,W,3] array, a PIL image or a
        path, decoded here (a file that is no image raises ValueError now, not at a frame): its largest centred window of
        the frame's aspect ratio, resampled with the output size's filter (`backdrop.image_ref`), prepared once per size; a
        device uint8 tensor of the frame's size ([Ho,Wo,3] where the matte composites at the output size, else [H,W,3], or
        fp16 [3,H,W]) is used in place, so a caller can change its content between frames at no host cost.  Such a tensor is
        checked here against the stream's size and the output size set at this moment (`backdrop.check_tensor`); which of
        the two sizes a frame needs is known only when it leaves -- a frame without a camera buffer, such as the first
        N - 1 outputs, takes the stream-sized composite even under `set_matte_source("camera")` -- and a tensor of the other
        size raises ValueError at that frame.  A uint8 tensor on the host is copied like an array.  A setting beside the matte, like `set_matte_edge`: it acts only while a matte is set,
        on its output types; `show=True` is unaffected; feather and edge refinement shape the composite as before, and the
        edge refinement keeps reading the real source frame.  The route of a frame does not change: where it takes the
        composite at the output size the backdrop at that size goes in as the kept part (a blur runs at the stream's size
        and is resampled), otherwise the stream-sized backdrop goes into the stream-sized composite.  On the device a blur is
        one more launch in front of the composite's (two at an output size), no synchronisation.  A frame the
        near-duplicate filter repeats is made again from the same slot: the same bytes.  May be called before or after
        `prepare` and between any two frames; the change applies from the next output."""
        from .backdrop import check_settings
        if isinstance(to, str) and to == "color":
            if color is None:
                raise ValueError("backdrop: to='color' needs color=(r, g, b)")
            to = tuple(color)
        elif color is not None:
            raise ValueError(f"backdrop: color={color!r} goes with to='color'")
        if isinstance(to, str) and to == "image":
            raise ValueError("backdrop: to='image': pass the image itself (an array, a PIL image, a path or a device tensor)")
        settings = check_settings(to, radius, passes)
        image = None
        if settings["to"] == "image":
            from .backdrop import check_tensor, load_image
            on_device = getattr(self, "io", None) is not None
            if torch.is_tensor(to) and (to.is_cuda or to.dtype == torch.float16):
                size = self._size
                check_tensor(to, self.height, self.width, None if size is None else (size["height"], size["width"]), on_device)
                image = to
            else:
                image = load_image(to)           # (decoded now: a bad file is refused here)
        if image is not self._backdrop_image:
            self._backdrop_host = None
        self._backdrop, self._backdrop_image = settings, image

    def clear_backdrop(self) -> None:
        """Back to the real frame behind the matte: no launch or buffer of the backdrop is left in the frame's path."""
        self._backdrop = self._backdrop_image = self._backdrop_dev = self._backdrop_host = None

    def _backdrop_filter(self) -> str:
        return self._size["resample"] if self._size is not None else "lanczos"

    def _backdrop_op(self, device):
        """`backdrop.HipBackdrop` of the stream's size, made on first use"""
        if self._backdrop_dev is None:
            from .backdrop import HipBackdrop
            self._backdrop_dev = HipBackdrop(self.height, self.width, device=device)
        return self._backdrop_dev

    def _backdrop_image_host(self):
        """the image of an "image" backdrop for the host route's oracles: as given, or the prepared frame of (size, filter)"""
        image = self._backdrop_image
        if image is None or torch.is_tensor(image):
            return image
        key = (self.height, self.width, self._backdrop_filter())
        if self._backdrop_host is None or key not in self._backdrop_host:
            from .backdrop import image_ref
            self._backdrop_host = {key: image_ref(image, *key)}
        return self._backdrop_host[key]

    def _sync_camera(self) -> None:
        """Install the camera tap (`HipFrameIO.camera_tap`, `MatteLine.camera_source`) while an output size is set on the device
        route and either "camera" with a matte or the detail mode wants it, rebuilt when the size or the filter changed;
        otherwise take it out and drop every camera buffer, so that nothing of the two features stays in the frame's path."""
        io, line, size = getattr(self, "io", None), self._matte_line, self._size
        want = (((self._matte_source == "camera" and self._matte is not None) or self._detail is not None)
                and size is not None and io is not None and line is not None)
        key = (size["height"], size["width"], size["resample"]) if want else None
        if want and self._camera is not None and self._camera.key == key:
            tap = self._camera
        else:
            if line is not None:
                line.drop_cameras()
            self._matte_up = self._detail_dev = None
            tap = None
            if want:
                from .resize import CameraTap
                tap = CameraTap(self.height, self.width, *key, device=io.device)
            self._camera = tap
        if io is not None:
            io.camera_tap = tap
        if line is not None:
            line.camera_source = tap

    def _camera_begin(self, image) -> None:
        """In front of every frame: a camera buffer nobody claimed belongs to no later frame, and the tap sits out the ingest
        of a frame that has no camera frame -- a path or a PIL image is resized on the host and reaches the ingest at the
        stream's own size, as a uint8 array that the tap would otherwise take for a camera's."""
        tap = self._camera
        if tap is not None:
            tap.begin()
            host_sized = isinstance(image, (str, os.PathLike)) or (hasattr(image, "convert") and hasattr(image, "resize"))
            self.io.camera_tap = None if host_sized else tap

    def _camera_slot(self, slot, image_tensor) -> bool:
        """does this output frame take the composite at the output size?"""
        tap = self._camera
        return (tap is not None and self._matte_source == "camera" and self._matte is not None and slot is not None
                and slot.camera is not None and slot.camera.key == tap.key
                and self.io is not None and torch.is_tensor(image_tensor) and image_tensor.is_cuda)

    def _need_line(self) -> None:
        """The delay line of source frames and depth planes, shared by the matte, the colour lock to "source", the steady mode
        and the detail mode: made by whichever needs it first.  Outputs of frames pushed before it existed have no slot (`_matte_skip`)."""
        if self._matte_line is None:
            from .matte import MatteLine
            self._matte_line = MatteLine(self.batch_size, self.height, self.width, device=self.stream.device)
            self.stream.matte_tap = self._matte_line
            self._matte_line.mask_source = self._mask_tap
            self._matte_skip = len(getattr(self.stream, "_pending", None) or ())

    def _release_line(self) -> None:
        """drop the delay line when neither the matte, a colour lock to "source", the steady mode nor the detail mode needs it"""
        if (self._matte is None and self._steady is None and self._detail is None
                and (self._lock is None or self._lock["mode"] != "source")):
            self._matte_line = None
            self._matte_skip = 0
            self.stream.matte_tap = None

    # ------------------------------------------------------------------ colour lock (color_lock.py)
    @property
    def color_lock(self) -> Optional[dict]:
        """the current colour lock as {to, strength, rate} (`to`: "source", "ema" or "image"), or None"""
        return None if self._lock is None else dict(to=self._lock["mode"], strength=self._lock["strength"], rate=self._lock["rate"])

    def set_color_lock(self, to="source", strength: float = 1.0, rate: float = 0.1) -> None:
        """Hold the output's colour statistics: per channel, the mean and the standard deviation of the bytes the frame leaves
        as are moved to a target by one gain (kept inside [1/4, 4]) and one offset.  `to="source"`: the frame's own source frame,
        so the stream follows the room's lighting; `to="ema"`: a running average of the styled frames themselves,
        t <- t + rate (c - t), so brightness and colour cast stop wandering (`prepare`, and this call, restart it from the next
        frame); `to=` an image (a path, a PIL image, a uint8 frame, a JPEG file, a float [3,H,W] tensor in [0, 1]): that
        image's statistics, measured once through the wrapper's own preprocessing and then frozen.  `strength` in [0, 1]
        scales the correction (0: the frame as it is), `rate` in (0, 1] is the average's step.  Two small launches on the
        device in front of the egress launch, the matte or the JPEG encoder; under a matte the styled frame is locked before
        the composite, so the real part of the picture stays untouched.  Every output type but "latent" is served.  May be
        called before or after `prepare` and between any two frames; the frames `prepare` returns are not locked, and a frame
        the near-duplicate filter dropped repeats the last locked frame without moving the average (with no locked frame to
        repeat, a drop directly behind this call, the repeated frame is locked as a frame of its own).  With `to="source"` the
        output of a frame that entered the stream before the delay line existed is locked to the oldest entry the line has, as
        the matte composites it with that entry; the mode keeps no state, so no later frame inherits anything from it (an
        output with no slot at all, in push / pop mode, passes unlocked)."""
        from .color_lock import SERVED_OUTPUT_TYPES, check_settings
        self._check_served(SERVED_OUTPUT_TYPES, "locked", "clear_color_lock")
        settings = check_settings(to, strength, rate)
        ref = self._reference_moments(to) if settings["mode"] == "image" else None
        self._lock = settings
        self._lock_ref = self._lock_state = self._lock_load = ref
        self._lock_init, self._lock_last = True, None
        if settings["mode"] == "source":
            self._need_line()
        else:
            self._release_line()

    def clear_color_lock(self) -> None:
        """Back to the unlocked output: no launch, copy or buffer of the lock is left in the frame's path.  (A matte keeps the
        delay line it shares with a lock to "source".)"""
        self._lock = self._lock_dev = self._lock_ref = self._lock_state = self._lock_load = self._lock_last = None
        self._lock_init = True
        self._release_line()

    def _reference_moments(self, image) -> np.ndarray:
        """the moments of a reference image, through the preprocessing a frame of the stream gets"""
        from .color_lock import moments_ref
        x = self.preprocess_image(image)
        dt = getattr(x, "dtype", None)
        if self.io is not None and (dt == torch.uint8 or dt == np.uint8):
            from .frame_io import HipFrameIO              # (an instance of its own: the stream's ingest slots are not disturbed)
            x = HipFrameIO(self.height, self.width, device=self.io.device).ingest(x)
            self._check_jpeg()
        else:
            x = self.stream.image_processor.preprocess(x, self.height, self.width)
        return moments_ref(x[-1] if x.ndim == 4 else x)

    def _locked(self, image_tensor: torch.Tensor, slot, repeated: bool) -> torch.Tensor:
        """the frame under the colour lock, fp16 [1,3,H,W]: ops 44 + 45 on the device, `lock_ref` without one.  `repeated`: the
        near-duplicate filter dropped the frame and `image_tensor` is the output of the one before; its locked frame is reused."""
        lock = self._lock
        if repeated and self._lock_last is not None:
            return self._lock_last
        source = None
        if lock["mode"] == "source":
            if slot is None:               # (an output of a frame the delay line has not seen)
                return image_tensor
            source = slot.source
        if self.io is not None and image_tensor.is_cuda:
            if self._lock_dev is None:
                from .color_lock import HipColorLock
                self._lock_dev = HipColorLock(self.height, self.width, device=image_tensor.device)
            if self._lock_load is not None:
                self._lock_dev.load_state(self._lock_load)
                self._lock_load = None
            out = self._lock_dev.lock(image_tensor[0], source, lock, init=self._lock_init)
        else:
            from .color_lock import lock_ref
            out, self._lock_state = lock_ref(image_tensor[:1], self._lock_state, mode=lock["mode"], strength=lock["strength"],
                                             rate=lock["rate"], init=self._lock_init, source=source)
            out = torch.from_numpy(out)
        self._lock_init = False
        self._lock_last = out
        return out

    # ------------------------------------------------------------------ steady (steady.py)
    @property
    def steady(self) -> Optional[dict]:
        """the current steady mode as {lo, hi, strength, radius, show}, or None"""
        return None if self._steady is None else dict(self._steady)

    def set_steady(self, lo: float = 2.0, hi: float = 10.0, *, strength: float = 0.8, radius: int = 2, show: bool = False) -> None:
        """Hold still what the camera holds still.  Per pixel the motion of the frame's SOURCE since the source of the output
        before is measured on the bytes a viewer would see (the largest change over the three channels, averaged over a
        (2 radius + 1)^2 window, `radius` 0..8): at or below `lo` byte levels a pixel counts as still and the previous output
        pixel is held, `out = prev + (1 - strength) (styled - prev)`; at or above `hi` it counts as moving and the new styled
        pixel passes untouched, bit for bit; a smoothstep in between.  A hard cut moves everything and passes by itself.
        `strength` in [0, 1] is how firmly a still pixel is held (0: the frame as it is, 1: frozen).  `show=True` returns the
        weight itself as a grey frame (white = moving), to choose `lo` and `hi` by eye.  The defaults are a starting point
        chosen for a sensor noise of about one byte level; they are not tuned on footage.  One small launch on the device
        behind the colour lock and in front of the egress launch, the matte, the resize or the JPEG encoder; under a matte
        the styled frame is steadied before the composite, so the real part of the picture stays untouched.  Every output
        type but "latent" is served.  May be called before or after `prepare` and between any two frames; this call and
        `prepare` restart the sequence (the next frame passes as it is), the frames `prepare` returns are not touched, a frame
        the near-duplicate filter dropped repeats the last steadied frame without moving the state, and the output of a
        frame that entered the stream before the delay line existed passes unchanged: the delay line has no slot of its own
        for it (the matte composites it with the oldest entry the line has, another frame's), so the sequence has not started
        yet -- the first output with a slot of its own is the init frame, and the state never holds another frame's source.
        (A repeated frame with no steadied frame to repeat, a drop directly behind this call, is treated as a frame of its
        own with the slot of the output before.)"""
        from .steady import SERVED_OUTPUT_TYPES, check_settings
        self._check_served(SERVED_OUTPUT_TYPES, "held steady", "clear_steady")
        settings = check_settings(lo, hi, strength, radius, show)
        self._need_line()
        self._steady = settings
        self._steady_state = self._steady_last = None
        self._steady_init = True

    def clear_steady(self) -> None:
        """Back to the plain output: no launch, copy or buffer of the steady mode is left in the frame's path.  (A matte and a
        colour lock to "source" keep the delay line they share with it.)"""
        self._steady = self._steady_dev = self._steady_state = self._steady_last = None
        self._steady_init = True
        self._release_line()

    # ------------------------------------------------------------------ follow (steady.py)
    @property
    def steady_follow(self) -> Optional[dict]:
        """the current follow setting as {search, bias}, or None"""
        return None if self._steady_follow is None else dict(self._steady_follow)

    def set_steady_follow(self, search: int = 4, bias: int = 256) -> None:
        """Let steady follow the source's motion.  Steady compares the source at the same coordinates, so under a hand-held
        camera, a slow pan or a person walking through the frame it holds nothing.  With this setting every 8 x 8 block of the
        frame's source is matched against the source of the output before, over displacements of up to `search` pixels (1..8)
        on either axis, on the bytes a viewer would see; the previous output and the previous source are then read where the
        block came from, and steady's arithmetic runs on them unchanged: what moved rigidly counts as still and is held along
        its path, what changed passes.  `bias` (0..4096, in summed byte levels over the block's 16 x 16 window per pixel of
        displacement) keeps sensor noise in flat areas from producing vectors; the default was chosen on synthetic noise, not
        on footage.  A setting beside steady, like `set_matte_edge` beside the matte: it acts only while steady is set, on
        its output types, and `steady` keeps its five keys; `show` shows the weight along the vectors.  One more launch on
        the device in front of steady's, no synchronisation.  The state is steady's own, so a change applies from the next
        output and does not restart the sequence; the init frame, repeated frames and `prepare` behave as under `set_steady`.
        May be called before or after `prepare` and between any two frames."""
        from .steady import check_follow
        self._steady_follow = check_follow(search, bias)

    def clear_steady_follow(self) -> None:
        """Back to steady at the same coordinates; the sequence goes on."""
        self._steady_follow = None

    def _steadied(self, image_tensor: torch.Tensor, slot, repeated: bool) -> torch.Tensor:
        """the frame under the steady mode, fp16 [1,3,H,W]: op 48 (with follow: ops 55 and 56) on the device, `steady_ref`
        (`follow_ref`) without one.  `repeated`: the near-duplicate filter dropped the frame and `image_tensor` is the output of
        the one before; its steadied frame is reused and the state does not move."""
        st = self._steady
        if repeated and self._steady_last is not None:
            return self._steady_last
        line = self._matte_line
        if slot is None or (line is not None and line.last is slot and not line.last_own):
            # an output of a frame the delay line has not seen -- no slot, or the oldest entry in its place, another frame's:
            # the sequence starts behind it, and the state never holds a source that is not the output's own
            self._steady_init, self._steady_last = True, None
            return image_tensor
        if self.io is not None and image_tensor.is_cuda:
            if self._steady_dev is None:
                from .steady import HipSteady
                self._steady_dev = HipSteady(self.height, self.width, device=image_tensor.device)
            out = self._steady_dev.steady(image_tensor[0], slot.source, st, init=self._steady_init, follow=self._steady_follow)
        elif self._steady_follow is not None:
            from .steady import follow_ref
            out, self._steady_state, _ = follow_ref(image_tensor[:1], slot.source, self._steady_state, **self._steady_follow, **st,
                                                    init=self._steady_init)
            out = torch.from_numpy(out)
        else:
            from .steady import steady_ref
            out, self._steady_state = steady_ref(image_tensor[:1], slot.source, self._steady_state, lo=st["lo"], hi=st["hi"],
                                                 strength=st["strength"], radius=st["radius"], show=st["show"],
                                                 init=self._steady_init)
            out = torch.from_numpy(out)
        self._steady_init = False
        self._steady_last = out
        return out

    def _check_served(self, served, noun: str, clear: str, what: Optional[str] = None) -> None:
        """ValueError where `output_type` is none a feature serves.  `noun`: what the feature does to a frame ("composited");
        `clear`: the method that turns it off; `what` ("a matte"): the check of a frame, while the feature is set -- without it
        the check of the feature's `set_...` call"""
        if self.output_type not in served:
            head, tail = (f"set_{clear[len('clear_'):]}:", "") if what is None else (f"{what} is set and", f", or {clear}()")
            raise ValueError(f"{head} output_type={self.output_type!r} is not {noun}: use one of "
                             + ", ".join(repr(t) for t in served) + tail)

    def _finish(self, image_tensor, slot, repeated: bool = False):
        """`postprocess_image` of a frame while a colour lock, the steady mode, a matte or an output size is set: the lock
        first, then steady, then the rest of the chain (`_route`) on that frame.  A frame that is no tensor is neither locked
        nor steadied and raises there."""
        from . import color_lock, detail, matte, resize, steady
        if self._lock is not None and torch.is_tensor(image_tensor):
            self._check_served(color_lock.SERVED_OUTPUT_TYPES, "locked", "clear_color_lock", "a colour lock")
            image_tensor = self._locked(image_tensor, slot, repeated)
        if self._steady is not None and torch.is_tensor(image_tensor):
            self._check_served(steady.SERVED_OUTPUT_TYPES, "held steady", "clear_steady", "the steady mode")
            image_tensor = self._steadied(image_tensor, slot, repeated)
        if self._size is not None:
            self._check_served(resize.SERVED_OUTPUT_TYPES, "resampled", "clear_output_size", "an output size")
        if self._matte is not None:
            self._check_served(matte.SERVED_OUTPUT_TYPES, "composited", "clear_matte", "a matte")
        if self._detail is not None:
            self._check_served(detail.SERVED_OUTPUT_TYPES, "given detail", "clear_detail", "the detail mode")
        if not torch.is_tensor(image_tensor):
            return self.postprocess_image(image_tensor, output_type=self.output_type)
        if self._size is not None and self.output_type == "jpeg":      # (callers assign `output_type` between frames)
            resize.check_jpeg_size(self._size["height"], self._size["width"])
        detail_slot = slot if self._detail_slot(slot, image_tensor) else None
        slot = slot if self._matte is not None else None
        return self._route(image_tensor, self.output_type, slot, self._size, camera=self._camera_slot(slot, image_tensor),
                           detail_slot=detail_slot, repeated=repeated)

    # ------------------------------------------------------------------ detail mode (detail.py)
    @property
    def detail(self) -> Optional[dict]:
        """the current detail mode as {radius, eps, strength, limit, show}, or None"""
        return None if self._detail is None else dict(self._detail)

    def set_detail(self, radius: int = 2, eps: float = 2.0, strength: float = 1.0, limit: float = 64.0, show: bool = False) -> None:
        """Bring the camera's fine detail into the frame at the output size.  The resize gives 1080 lines made of the stream's
        512; the camera frame at the output size holds what the stream-size bottleneck lost: d = luma(camera) - luma(source
        frame through the same resize).  Per channel, d is added to the resized styled frame times a gain: the local
        regression slope of the styled frame on the source frame's luma in every (2 radius + 1)^2 window of the stream's frame
        (`radius` 1..8; `eps` >= 1 in byte levels: the contrast of the source below which a window counts as flat), averaged
        over the window and sampled bilinearly at the output size (`detail.detail_ref`).  Where the style follows the camera's
        structure its sub-pixel edges and texture come back in the style's own colours and polarity; where the style is flat
        nothing is added.  `strength` in [0, 4] scales the injected term (0: the frame as it is), `limit` in [0, 255] bounds it
        in byte levels, `show=True` returns 128 + the injected term (to choose `eps` by eye).  Three small launches on the
        device behind the resize: the order on a frame is colour lock, steady, matte on the "stream" route, resize, detail,
        the matte composite at the output size on the "camera" route, then the JPEG encoder or the copy to the host -- the
        gains are always fitted on the bytes the resize reads.

        The mode acts on an output frame only when an output size is set, the frame runs on the device route, and the frame
        it is paired with came in as a uint8 frame or a JPEG file while the mode and the current output size were set (the
        delay line's slot then carries its pixels).  Every other frame leaves exactly as without the mode -- float tensors,
        PIL images and paths, frames from before the mode or the size was set, the frames `prepare` returns, and the host
        route without a device.  That is the behaviour, not an error.  A frame the near-duplicate filter repeats is computed
        again from the same slot: the same bytes.  May be called before or after `prepare` and between any two frames."""
        from .detail import SERVED_OUTPUT_TYPES, check_settings
        self._check_served(SERVED_OUTPUT_TYPES, "given detail", "clear_detail")
        settings = check_settings(radius, eps, strength, limit, show)
        self._need_line()
        self._detail = settings
        self._sync_camera()

    def clear_detail(self) -> None:
        """Back to the plain resize: no launch, buffer or camera tap of the mode is left in the frame's path.  (A matte with
        `set_matte_source("camera")` keeps the tap, and the other users of the delay line keep the line.)"""
        self._detail = self._detail_dev = None
        self._release_line()
        self._sync_camera()

    def _detail_slot(self, slot, image_tensor) -> bool:
        """does this output frame get the camera's detail?"""
        tap, line = self._camera, self._matte_line
        return (self._detail is not None and self._size is not None and tap is not None and slot is not None
                and line is not None and line.last is slot and line.last_own      # (the slot of the output's own frame)
                and slot.camera is not None and slot.camera.key == tap.key
                and self.io is not None and torch.is_tensor(image_tensor) and image_tensor.is_cuda)

    # ------------------------------------------------------------------ output size (resize.py)
    @property
    def output_size(self) -> Optional[dict]:
        """the current output size as {height, width, resample}, or None: frames leave at the UNet's size"""
        return None if self._size is None else dict(self._size)

    def set_output_size(self, height: int, width: int, resample: str = "lanczos") -> None:
        """Give frames back at `height` x `width` instead of the UNet's size: Pillow's `Image.resize` on the uint8 frame
        (`resample`: "lanczos", "bicubic" or "bilinear"), byte for byte, in one launch on the device.  Per axis the size may lie
        between half and 8 times the UNet's, up to 4096; for "jpeg" it must also be a multiple of 16 and no wider than 1920, which
        is checked here.  The order on a frame is colour lock, matte, resize, then the JPEG encoder ("jpeg", one encoder per
        size; no raw frame reaches the host) or the copy to the host ("u8", "pil"); the float output types are not served.
        Without a matte the launch takes the fp16 frame and replaces the egress launch; with one it takes the matte's uint8
        frame.  Resampling the composite is the whole feature: under a matte the kept real part of the picture is the
        UNet-sized source frame scaled up, not the camera's own pixels (`set_matte_source("camera")` keeps those instead), and
        nothing is sharpened (`set_detail` brings the camera's fine detail into the resized frame).  May be called before or after
        `prepare` and between any two frames: the change applies from the next output.  The frames `prepare` returns are not
        resized; a frame the near-duplicate filter dropped yields the bytes of the frame before it."""
        from .resize import SERVED_OUTPUT_TYPES, check_filter, check_jpeg_size, check_size
        self._check_served(SERVED_OUTPUT_TYPES, "resampled", "clear_output_size")
        ho, wo = check_size(self.height, self.width, height, width)
        check_filter(resample)
        if self.output_type == "jpeg":
            check_jpeg_size(ho, wo)
        self._size = dict(height=ho, width=wo, resample=resample)
        self._sync_camera()

    def clear_output_size(self) -> None:
        """Back to the UNet's size: no launch, copy or buffer of the resize is left in the frame's path, the camera buffers of
        `set_matte_source("camera")` included."""
        self._size = self._size_dev = self._size_jpeg = None
        self._sync_camera()

    # ------------------------------------------------------------------ styles (style_bank.py)
    def _init_styles(self, pipe) -> None:
        """The style the wrapper was built with becomes "default", as a copy: the active weights are scratch that the next switch
        overwrites.  Needs the native UNet and text encoder; with other components the bank stays empty and `set_style` refuses."""
        from .clip_hip import HipClipTextEncoder
        from .style_bank import StyleBank, clone_set
        from .unet_hip import HipStreamingUNet
        self._bank = StyleBank()
        self._prompt = None
        text = getattr(pipe, "text_encoder", None)
        if text is None:
            text = getattr(getattr(getattr(pipe, "_encode_prompt", None), "__self__", None), "encoder", None)
        self._text_encoder = text if isinstance(text, HipClipTextEncoder) else None
        if isinstance(self.stream.unet, HipStreamingUNet) and self._text_encoder is not None:
            self._bank.add("default", clone_set(self.stream.unet.packed_state()), clone_set(self._text_encoder.packed_state()))
            self._bank.current = {"default": 1.0}

    def _need_bank(self):
        if not self._bank.sets:
            raise ValueError("styles need the native UNet and text encoder (HipStreamingUNet, HipClipTextEncoder)")
        return self._bank

    @property
    def styles(self) -> List[str]:
        """names of the registered styles"""
        return self._bank.names

    @property
    def style(self) -> Dict[str, float]:
        """the current mix as {name: weight}"""
        return dict(self._bank.current)

    def add_style(self, name: str, dreambooth_path: Optional[str] = None, lora_dict: Optional[Dict[str, float]] = None, *,
                  unet_state_dict=None, text_state_dict=None) -> None:
        """Register a style and keep its packed UNet and text-encoder sets resident.  From files: the path `load_components` takes
        (`build_state_dict`, the packed-weight cache under the same name, `build_text_encoder_state_dict`).  From state dicts
        (`from_components` callers): `unet_state_dict` in the reference's key names, `text_state_dict` in transformers'.  Either
        way the sets come from second, plan-less instances; the running stream is not touched.  With `use_tiny_vae=False` a style
        that carries its own VAE keeps the constructor's VAE."""
        from .clip_hip import HipClipTextEncoder
        from .unet_hip import HipStreamingUNet
        bank = self._need_bank()
        if not isinstance(name, str) or not name:
            raise ValueError(f"style name {name!r}: use a non-empty string")
        if name in bank.sets:
            raise ValueError(f"style {name!r} is registered already: remove_style it first")
        unet, text = self.stream.unet, self._text_encoder
        from_sd = unet_state_dict is not None or text_state_dict is not None
        if from_sd:
            if dreambooth_path is not None or lora_dict is not None:
                raise ValueError("add_style: give files (dreambooth_path / lora_dict) or state dicts, not both")
            if unet_state_dict is None or text_state_dict is None:
                raise ValueError("add_style: unet_state_dict and text_state_dict go together")
            usrc = HipStreamingUNet(unet_state_dict, unet.cfg, unet.h, unet.w, unet.N, device=unet.device)
            tsrc = HipClipTextEncoder(text_state_dict, text.device, text.cfg, use_graph=False)
            sets = (usrc.packed_state(), tsrc.packed_state())
        else:
            src = getattr(self, "_style_src", None)
            if src is None:
                raise ValueError("add_style: this wrapper was made from components, not from a config: pass unet_state_dict and "
                                 "text_state_dict")
            sets = build_style_sets(src["cfg"], unet, text, dreambooth_path=dreambooth_path, lora_dict=lora_dict,
                                    few_step_model_type=src["few_step_model_type"], engine_dir=src["engine_dir"])
        bank.add(name, *sets)

    def remove_style(self, name: str) -> None:
        """Forget a style and free its sets; a style that is part of the current mix is refused."""
        bank = self._need_bank()
        sets = bank.sets.get(name)
        bank.remove(name)
        for inst, ps in zip((self.stream.unet, self._text_encoder), sets):
            if inst._blender is not None:
                inst._blender.forget(ps.W)             # (a blend table keeps the sets it reads alive)

    def set_style(self, style, rewarm=False) -> None:
        """Switch to a registered style (a name) or to an affine mix of up to four ({name: weight}, weights summing to 1) between
        two frames: one blend launch each over the UNet's and the text encoder's packed weights on the current stream, then the
        current prompt re-encoded by the new text encoder and handed to the stream like `update_prompt` does.  No plan or graph is
        rebuilt; the VAE, the depth detector, the KV caches, the stream batch, the ring state and the noise counter are not
        touched.  Takes effect with the next frame, in `__call__` and in push / pop mode (the side stream of `push` never touches
        these weights).  K / V of earlier frames were projected by the old weights: window slots age out within `window_size`
        frames -- that is the cross-fade -- and the sink slots written by `prepare` keep the old projections until they are
        re-warmed: `rewarm=True` does it right here on the window `prepare` was given, `rewarm="recent"` on the last frames
        (`rewarm(...)`, behind the mix and the re-encoded prompt); False, the default, leaves them."""
        from .style_bank import drop_zero_terms, parse_style
        if rewarm not in (False, True, "warmup", "recent"):
            raise ValueError(f"rewarm={rewarm!r}: use False, True (the window of prepare) or 'recent'")
        if rewarm == "recent" and not self.stream.keep_recent:
            raise ValueError("rewarm='recent' needs a wrapper built with keep_recent=True")
        bank = self._need_bank()
        mix = parse_style(style, bank.sets)
        names, weights = drop_zero_terms(list(mix), list(mix.values()))
        self.stream.unet.load_mix([bank.sets[n][0] for n in names], weights)
        self._text_encoder.load_mix([bank.sets[n][1] for n in names], weights)
        bank.current = dict(zip(names, weights))
        if self._prompt is not None:
            self.stream.update_prompt(self._prompt)
        if rewarm:
            self.rewarm("recent" if rewarm == "recent" else "warmup")

    # ------------------------------------------------------------------ re-warm
    @property
    def rewarms(self) -> int:
        """completed re-warms since `prepare`"""
        return self.stream.rewarms

    def rewarm(self, source="warmup", *, depths=None) -> None:
        """Refresh the sink slots of every temporal layer under the weights and the prompt the stream has now, without a new
        `prepare` (`StreamAnimateDiffusionDepth.rewarm`).  source: "warmup", the window `prepare` was given; "recent", the last F
        frames that entered the stream (`keep_recent=True`); or frames -- anything `prepare` takes as `warmup_frames`, encoded as
        `prepare` encodes them (the detector, or `depths` as `prepare`'s `warmup_depths`) but without the matte tap.  It restarts
        nothing: the matte's delay line, the colour lock, steady, the matte hold, the key's plate and the output size carry on.
        Legal with frames pushed and not yet popped: it runs on the caller's stream and their UNet steps run behind it.
        A pending automatic re-warm (`set_auto_rewarm`) is cancelled once this one has succeeded: it has done its work."""
        self._rewarm(source, depths)
        self._rewarm_due = None

    def _rewarm(self, source, depths) -> None:
        if isinstance(source, str):
            if source not in ("warmup", "recent"):
                raise ValueError(f"source={source!r}: use 'warmup', 'recent' or a window of frames")
            if depths is not None:
                raise ValueError(f"depths= goes with frames, not with source={source!r}: that window's depth is already encoded")
            if source == "recent":
                if not self.stream.keep_recent:
                    raise ValueError("source='recent' needs a wrapper built with keep_recent=True")
                if self.stream._warm_window is None:
                    raise RuntimeError("rewarm() needs prepare() first: there is no stream to re-warm")
                self.stream.rewarm(*self.stream.recent_window())
            else:
                self.stream.rewarm()
            return
        if isinstance(depths, (list, tuple)):
            items = [self._depth_arg(d, "depths") for d in depths]
            depths = torch.stack(items) if torch.is_tensor(items[0]) else np.stack(items)
        depths = self._depth_arg(depths, "depths")
        side = getattr(self.stream, "_pre_stream", None)
        if side is not None and getattr(self.stream, "_pending", None):
            # the encodes below use the plan buffers (TAESD encoder, depth detector) the pushed frames' side-stream work may still hold
            torch.cuda.current_stream().wait_stream(side)
        gen = self.stream.rewarm_generator()              # one generator: the encode's draws, then the noise between rows
        x, d = self._on_window(source, lambda frames: self.stream.encode_window(frames, depths, generator=gen))
        self.stream.rewarm(x, d, generator=gen)

    def _on_window(self, warmup_frames, run):
        """`run(frames)` on a warm-up window as `prepare` takes it: a list of JPEG files is decoded, a uint8 batch goes through one
        batched ingest launch, float frames pass as they are"""
        if isinstance(warmup_frames, (list, tuple)) and warmup_frames and all(_is_jpeg(f) for f in warmup_frames):
            # (a device frame is a view of one of the decoder's two static slots: it is copied before the slot's next turn)
            decoded = [d.clone() if torch.is_tensor(d) else torch.from_numpy(d).to(self.io.device) if self.io is not None else d
                       for d in map(self._decode_jpeg, warmup_frames)]
            warmup_frames = torch.stack(decoded) if torch.is_tensor(decoded[0]) else np.stack(decoded)
            self._check_jpeg()
        dt = getattr(warmup_frames, "dtype", None)
        if dt == torch.uint8 or dt == np.uint8:
            from .frame_io import _PassThrough
            if self.io is None:
                raise ValueError("uint8 warm-up frames need the device-side frame I/O (a cuda device)")
            x = self.io.ingest(warmup_frames)
            # the pipeline preprocesses frame by frame and only then concatenates: through a static ingest slot all rows would be
            # views of the last frame, and a normalised frame must never reach a [0, 1]-or-[-1, 1] probe
            keep, self.stream.image_processor = self.stream.image_processor, _PassThrough()
            try:
                return run(x)
            finally:
                self.stream.image_processor = keep
        return run(warmup_frames)

    # ------------------------------------------------------------------ cut detection and the automatic re-warm
    CUTS_KEPT = 256

    def _init_cut_detect(self) -> None:
        import collections
        self.cuts = collections.deque(maxlen=self.CUTS_KEPT)     # the frame indices, since `prepare`, of the cuts reported

    @property
    def cut_detect(self) -> Optional[dict]:
        """the cut detector's settings as {thumb, hist, ratio, gap}, or None"""
        return None if self._cut_settings is None else dict(self._cut_settings)

    @cut_detect.setter
    def cut_detect(self, settings: Optional[dict]) -> None:
        if settings is None:
            self.clear_cut_detect()
        elif isinstance(settings, dict):
            self.set_cut_detect(**settings)
        else:
            raise ValueError(f"cut_detect={settings!r}: use a dict of set_cut_detect's keywords, or None")

    def set_cut_detect(self, thumb=20.0, hist=0.35, ratio=3.0, gap=8) -> None:
        """Measure every frame that enters the stream against the one before, on the device (`cut.HipCutDetect`: two small
        launches and one asynchronous 32-byte copy per frame, no synchronisation added), and report scene cuts in `cuts` /
        `last_cut_record`.  A frame is a cut when its block-luma thumbnail moved by `thumb` byte levels on average AND `hist` of
        its pixels changed histogram bin AND (`ratio` > 0) the thumbnail moved `ratio` times the running level of the frames
        before; `gap` frames behind a cut none is reported.  The defaults are a guess, untuned on footage.  May be called before
        or after `prepare` and between any two frames; on a running detector only the thresholds change."""
        from . import cut
        settings = cut.check_settings(thumb, hist, ratio, gap)
        det = self.stream.cut_detector
        if det is None:
            self.stream.cut_detector = cut.HipCutDetect(self.height, self.width, settings, device=self.device)
        else:
            det.configure(settings)
        self._cut_settings = settings

    def clear_cut_detect(self) -> None:
        """No detector: every launch of a frame is again what it was without one.  A pending automatic re-warm is dropped and
        `auto_rewarm` goes off with it; `cuts` stays as a record of what was found."""
        self.stream.cut_detector = None
        self.stream.cut_records.clear()
        self._cut_settings, self._auto_rewarm, self._rewarm_due = None, False, None

    @property
    def auto_rewarm(self) -> bool:
        return self._auto_rewarm

    @auto_rewarm.setter
    def auto_rewarm(self, on) -> None:
        self.set_auto_rewarm(on)

    def set_auto_rewarm(self, on=True) -> None:
        """Re-warm the sinks by themselves behind a cut: a cut at frame n makes `rewarm("recent")` due once the recent window holds
        frames n .. n + F - 1, all of the new scene; it runs at the head of the next `img2img` / `pop`, in front of that frame's
        UNet step.  A further cut before that moves the due point (it does not stack); a manual `rewarm` or `set_style(...,
        rewarm=...)` in between cancels it.  Needs `keep_recent=True` and a cut detector."""
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"auto_rewarm={on!r}: use True or False")
        if on and not self.stream.keep_recent:
            raise ValueError("auto_rewarm needs a wrapper built with keep_recent=True")
        if on and self._cut_settings is None:
            raise ValueError("auto_rewarm needs a cut detector: call set_cut_detect first")
        self._auto_rewarm = bool(on)
        if not on:
            self._rewarm_due = None

    def _cut_head(self) -> None:
        """the head of a frame: the automatic re-warm, when one is due"""
        due = self._rewarm_due
        if due is not None and self.stream._recent_seen >= due:
            self._rewarm_due = None               # (first: one that raises is not tried again at every frame)
            self.rewarm("recent")
            self.auto_rewarms += 1

    def _cut_tail(self) -> None:
        """behind a frame: the records the pipeline collected at its synchronisation"""
        records = self.stream.cut_records
        if not records:
            return
        from .cut import record_dict
        while records:
            rec = record_dict(records.popleft())
            self.last_cut_record = rec
            if rec["cut"]:
                self.cuts.append(rec["n"])
                if self._auto_rewarm:
                    self._rewarm_due = rec["n"] + self.stream.warmup_frames

    # ------------------------------------------------------------------ prepare
    def prepare(self, warmup_frames, prompt: str, negative_prompt: str = "", guidance_scale: float = 1.2, delta: float = 1.0,
                warmup_depths=None, warmup_masks=None) -> torch.Tensor:
        """warmup_frames: float [F,3,H,W] in [0, 1] as in the reference, uint8 [F,Hs,Ws,3] (one batched ingest launch), or a list
        of JPEG files of one size (decoded like `img2img`'s, then the uint8 route).  warmup_depths: the frames' own depth, a batch
        [F,Hd,Wd] (or a list of what `img2img` takes as `depth`, of one size), normalised jointly; None: the detector.
        warmup_masks: one mask per warm-up frame, a batch [F,Hm,Wm] or a list of what `img2img` takes as `mask`; the last one
        cuts the N - 1 primed positions of the delay line; None: those positions have no mask of their own (a sticky mask
        applies to them as to any frame).  Needs a matte.
        Returns the generated warm-up frames, [F,H,W,3] in [0, 1] (wrapper.py:197-199)."""
        kw = dict(prompt=prompt, negative_prompt=negative_prompt, guidance_scale=guidance_scale, delta=delta, seed=self.seed)
        if isinstance(warmup_depths, (list, tuple)):
            items = [self._depth_arg(d, "warmup_depths") for d in warmup_depths]
            warmup_depths = torch.stack(items) if torch.is_tensor(items[0]) else np.stack(items)
        warmup_depths = self._depth_arg(warmup_depths, "warmup_depths")
        if warmup_depths is not None:
            kw["warmup_depths"] = warmup_depths
        last_mask = None
        if warmup_masks is not None:
            if self._matte is None:
                raise ValueError("warmup_masks: a mask needs a matte: call set_matte first")
            if self._key is not None:
                raise ValueError("warmup_masks: a mask and a matte key exclude each other: call clear_matte_key first")
            n_frames = len(warmup_frames) if hasattr(warmup_frames, "__len__") else None
            if not hasattr(warmup_masks, "__len__") or len(warmup_masks) == 0 or (n_frames is not None and len(warmup_masks) != n_frames):
                raise ValueError(f"warmup_masks: expected one mask per warm-up frame ({n_frames}), a batch [F,Hm,Wm] or a list")
            last_mask = warmup_masks[-1]
        self._mask_begin(last_mask, "warmup_masks")        # (claimed by the line's `prime`; with N = 1 by nobody)
        self._prompt = prompt
        self._matte_skip = 0               # (`stream.prepare` primes the matte's delay line through the tap, when one is set)
        self._lock_init, self._lock_last = True, None      # an "ema" colour lock starts again; a reference image's state stays
        if self._lock is not None and self._lock["mode"] != "image":
            self._lock_state = None
        self._steady_init, self._steady_last, self._steady_state = True, None, None      # the steady mode starts again too
        self._hold_init, self._hold_state = True, None                                   # and the matte hold
        self.cuts.clear()                                                                # and the cut detector's count (the pipeline restarts it)
        self.last_cut_record, self._rewarm_due, self.auto_rewarms = None, None, 0
        frames = self._on_window(warmup_frames, lambda x: self.stream.prepare(warmup_frames=x, **kw))
        from .unet_hip import HipStreamingUNet
        if isinstance(self.stream.unet, HipStreamingUNet):
            self.stream.enable_device_step(seed=self.seed)
            if self.frame_pipelining:
                self.stream.enable_frame_pipelining()
        frames = frames.permute(0, 2, 3, 1)
        return (frames.clip(-1, 1) + 1) / 2

    # ------------------------------------------------------------------ frames
    def __call__(self, image=None, prompt: Optional[str] = None, depth=None, mask=None):
        return self.img2img(image, prompt, depth, mask)

    def img2img(self, image, prompt: Optional[str] = None, depth=None, mask=None):
        """image: a path, a PIL image (resized to (width, height) on the host like the reference, :264-267), a uint8 HWC array /
        tensor of any size (resize + centre crop on the device), a JPEG file as `bytes` / `bytearray` / `memoryview` (decoded on the
        device, then treated as that uint8 frame; a damaged scan raises ValueError where the output is fetched), or a float
        [3,H,W] tensor in [0, 1] (the reference's input).  depth: the frame's own depth frame in place of the detector's -- a uint16
        or float32 [Hd,Wd] array or tensor of any size, on the host or on the device, a PIL image of mode "I;16", "I", "F" or "L",
        or a path to one -- read as `set_depth_input` says; frames with and without it may alternate (not under
        `depth_source="input"`, where a frame without raises ValueError).  A frame the near-duplicate filter drops ignores it.
        mask: the frame's own matte in place of (or combined with, `set_mask_input`) the depth ramp -- a uint8, uint16, bool or
        float32 [Hm,Wm] array or tensor of any size, on the host or on the device, a PIL image of mode "L", "1", "I;16" or "F",
        or a path to one --, covering the camera frame's field of view; it needs a matte, is delayed with its frame and cuts
        that frame's output N - 1 frames on.  Frames with and without one may alternate; a dropped frame ignores it."""
        depth = self._depth_arg(depth)
        dk = {} if depth is None else {"depth": depth}
        if prompt is not None:
            self._update_prompt(prompt)
        self._camera_begin(image)
        self._mask_begin(mask)
        if self._cut_settings is not None:
            return self._img2img_cut(image, dk)
        return self._img2img(image, dk)

    def _img2img_cut(self, image, dk):
        """`_img2img` with a cut detector: a due re-warm at the head, the frame's record behind it"""
        self._cut_head()
        try:
            return self._img2img(image, dk)
        finally:
            self._cut_tail()

    def _img2img(self, image, dk):
        line = self._matte_line
        if line is None and self._lock is None and self._size is None:
            return self.postprocess_image(self.stream(self.preprocess_image(image), **dk), output_type=self.output_type)
        if line is None:
            # a frame the near-duplicate filter dropped comes back as the very tensor of the output before
            before = getattr(self.stream, "prev_image_result", None)
            out = self.stream(self.preprocess_image(image), **dk)
            return self._finish(out, None, repeated=before is not None and out is before)
        seen = line.tapped
        out = self.stream(self.preprocess_image(image), **dk)
        # a frame the near-duplicate filter dropped never reached the tap: the repeated output keeps its slot
        fresh = line.tapped > seen
        return self._finish(out, line.take() if fresh else line.last, repeated=not fresh)

    def push(self, image, prompt: Optional[str] = None, depth=None, mask=None) -> None:
        """pipelined mode (`frame_pipelining=True`): start a frame's encode / depth path; `pop()` returns the oldest frame's output.
        `depth`: as `img2img`'s; its ingest runs on the side stream with the rest of the depth path.  `mask`: as `img2img`'s; its
        copy runs here, on the caller's stream, and its ingest with the composite in `pop`."""
        depth = self._depth_arg(depth)
        if prompt is not None:
            self._update_prompt(prompt)
        self._camera_begin(image)
        self._mask_begin(mask)
        self.stream.push(self.preprocess_image(image), **({} if depth is None else {"depth": depth}))
        if self.io is not None and self.io.last_view is not None:
            # push() ran the ingest on this stream before ordering the side stream behind it; the side stream reads the slot
            # until the event push recorded behind its two encodes
            self.io.release(self.io.last_view, self.stream._pending[-1][2])

    def pop(self):
        if self._cut_settings is not None:
            self._cut_head()
        out = self.stream.pop()
        if self._cut_settings is not None:
            self._cut_tail()
        if self._matte_line is None and self._lock is None and self._size is None:
            return self.postprocess_image(out, output_type=self.output_type)
        slot = None
        if self._matte_line is not None:
            if self._matte_skip:
                self._matte_skip -= 1
            else:
                slot = self._matte_line.take()
        return self._finish(out, slot)

    def _update_prompt(self, prompt: str) -> None:
        self.stream.update_prompt(prompt)
        self._prompt = prompt              # (what set_style re-encodes with the new text encoder)

    def _decode_jpeg(self, data):
        """a JPEG file -> its uint8 [Hs,Ws,3] frame: a device tensor (a view of a static slot of `jpeg_io.HipJpegDecoder`), or Pillow's
        array where there is no device, `jpeg_decode="host"`, or the file is outside the device's subset (progressive, greyscale...)"""
        if self.io is not None and self.jpeg_decode == "device":
            from .jpeg import JpegUnsupported
            if self.jpeg_dec is None:
                from .jpeg_io import HipJpegDecoder
                self.jpeg_dec = HipJpegDecoder(device=self.io.device)
            try:
                return self.jpeg_dec.decode(data)
            except JpegUnsupported:
                pass
        import io

        from PIL import Image
        self.jpeg_host_decodes += 1
        return np.array(Image.open(io.BytesIO(data)).convert("RGB"))

    def _check_jpeg(self) -> None:
        if self.jpeg_dec is not None:
            self.jpeg_dec.check()

    def preprocess_image(self, image):
        """path / PIL image -> uint8 [height, width, 3] (host resize, as the reference); arrays and tensors pass through: the
        pipeline's `image_processor` (frame_io.FrameProcessor) ingests them, so a normalised tensor never meets a range probe"""
        if isinstance(image, (bytes, bytearray, memoryview)):
            if not _is_jpeg(image):
                raise ValueError("a bytes frame must be a JPEG file (it does not begin with FF D8)")
            return self._decode_jpeg(image)
        if isinstance(image, (str, os.PathLike)):
            from PIL import Image
            image = Image.open(image)
        if hasattr(image, "convert") and hasattr(image, "resize"):
            arr = np.array(image.convert("RGB").resize((self.width, self.height)))
            if self.io is None:
                return torch.from_numpy(arr).permute(2, 0, 1).float() / 255.0
            return arr
        return image

    def postprocess_image(self, image_tensor: torch.Tensor, output_type: str = "pil"):
        """`image_utils.postprocess_image(x, output_type)[0]` (+ `.cpu()` for "pt" / "latent", wrapper.py:289-297); "u8" and "pil"
        through the egress kernel when the tensor is on the device; "jpeg" through the device-side encoder (no egress launch, no raw
        frame on the host), the file of `encode_ref(egress_ref(x))` either way.  A matte, a colour lock and an output size are
        not applied: this is `_route` with neither."""
        if not torch.is_tensor(image_tensor):
            raise ValueError(f"Input for postprocessing is in incorrect format: {type(image_tensor)}. We only support pytorch tensor")
        return self._route(image_tensor, output_type)

    def _route(self, image_tensor: torch.Tensor, output_type: str, slot=None, size: Optional[dict] = None, camera: bool = False,
               detail_slot=None, repeated: bool = False):
        """The one way out for a frame (fp16 [1,3,H,W] in [-1, 1], behind the colour lock and the steady mode when set): the matte's composite
        with `slot` (a `MatteLine` slot; None: no matte, or its line has seen no frame yet) or the egress bytes, resampled to
        `size` (the setting of `set_output_size`, or None), then the JPEG encoder or the copy to the host.  `camera` (the slot
        carries the camera's pixels at `size`, `_camera_slot`): the resize of the styled frame first, then the composite at the
        output size, in place of those two stages.  `detail_slot` (the frame's slot where the detail mode acts on it,
        `_detail_slot`): the detail launches behind the resize, on the frame the resize read.  `repeated` (the near-duplicate filter
        dropped the frame): a matte hold composites with the last held matte and does not advance.  On the device every
        stage is one launch that hands its static device buffer to the next and only the last one copies to the host; the
        resize takes the fp16 frame itself, and so does the encoder, so neither has an egress launch in front of it.  The float
        output types leave as the reference's do."""
        u8 = out = None
        if output_type == "latent":
            out = image_tensor[0].cpu()
        elif output_type == "pt":
            out = (image_tensor / 2 + 0.5).clamp(0, 1)[0].cpu()
        elif output_type == "np":
            out = (image_tensor / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()[0]
        elif output_type not in ("pil", "u8", "jpeg"):
            raise ValueError(f"output_type={output_type!r}: use one of {OUTPUT_TYPES}")
        elif self.io is not None and image_tensor.is_cuda:
            dev, to_host = image_tensor.device, output_type != "jpeg"
            stages = []
            give_detail = None
            if detail_slot is not None and size is not None:
                give_detail = functools.partial(self._detail_op(size, dev).apply, slot=detail_slot, settings=self._detail)
            bd = self._backdrop if slot is not None and not self._matte["show"] else None
            held = {}                       # (the keywords only with a hold or a mask: without them the calls are the parent's)
            if slot is not None and self._hold is not None:
                held["hold"] = self._hold_step(dev, repeated)
            front = self._key_front(slot, dev, repeated) if self._key is not None else self._mask_front(slot)
            bdk = {}
            if front is not None:
                held["mask"] = front
                bdk["plane"] = front[2]
            if camera:
                stages.append(self._size_op(size, dev).resize)
                if give_detail is not None:
                    stages.append(give_detail)
                more = {} if bd is None else dict(backdrop=self._backdrop_op(dev).output(
                    slot, self._matte, bd, size["height"], size["width"], self._backdrop_image, size["resample"], **bdk))
                stages.append(functools.partial(self._matte_up_op(size, dev).composite, slot=slot, settings=self._matte,
                                                edge=self._matte_edge, **more, **held))
            elif slot is not None:
                more = {} if bd is None else dict(backdrop=self._backdrop_op(dev).stream(
                    slot, self._matte, bd, self._backdrop_image, self._backdrop_filter(), **bdk))
                stages.append(functools.partial(self._matte_op(dev).composite, slot=slot, settings=self._matte, edge=self._matte_edge,
                                                **more, **held))
            if size is not None and not camera:
                stages.append(self._size_op(size, dev).resize)
                if give_detail is not None:
                    stages.append(give_detail)
            if not stages and to_host:
                stages.append(self.io.egress)
            x = before = image_tensor[0]
            for i, stage in enumerate(stages):
                last = to_host and i + 1 == len(stages)
                if stage is give_detail:   # (it also takes the frame the resize in front of it read)
                    x = stage(x, before, to_host=last)
                else:
                    before, x = x, stage(x, to_host=last)
            if to_host:
                u8 = x.copy()              # (the pinned buffer is overwritten by the next frame)
            else:
                out = self._encoder(size, dev).encode(x)
        else:
            if slot is not None:
                from .matte import composite_ref
                more = {}                   # (the keyword only with a backdrop: without one the call is the parent's)
                raw = self._key_plane(slot, repeated) if self._key is not None else self._mask_plane(slot)
                if self._backdrop is not None and not self._matte["show"]:
                    from .backdrop import stream_ref
                    more["backdrop"] = stream_ref(self._backdrop, self._backdrop_image_host(), slot.source, slot.depth, self._matte,
                                                  self._backdrop_filter(), **({} if raw is None else {"plane": raw}))[None]
                if self._hold is not None:
                    more["plane"] = self._held_plane(slot, repeated, **({} if raw is None else {"raw": raw}))
                elif raw is not None:
                    from .matte import edge_ref
                    more["plane"] = (raw if self._matte_edge is None else edge_ref(raw, slot.source, **self._matte_edge))[None]
                u8 = composite_ref(image_tensor[:1], slot.source[None], slot.depth[None], **self._matte, edge=self._matte_edge, **more)[0]
            else:
                from .frame_io import egress_ref
                u8 = egress_ref(image_tensor)[0].numpy()
            if size is not None:
                from .resize import resize_ref
                u8 = resize_ref(u8, size["height"], size["width"], size["resample"])
        self._check_jpeg()                 # behind the copy to the host every output type ends in: the status words are there too
        if u8 is None:
            return out
        if output_type == "jpeg":
            from .jpeg import encode_ref
            return encode_ref(u8, self.jpeg_quality)
        if output_type == "u8":
            return u8
        from PIL import Image
        return Image.fromarray(u8)

    def _matte_op(self, device):
        """`matte.HipMatte` of the stream's size, made on first use"""
        if self._matte_dev is None:
            from .matte import HipMatte
            self._matte_dev = HipMatte(self.height, self.width, device=device)
        return self._matte_dev

    def _matte_up_op(self, size: dict, device):
        """`matte.HipMatteUp` of an output size: rebuilt when the size changes, kept otherwise"""
        ho, wo = size["height"], size["width"]
        mu = self._matte_up
        if mu is None or (mu.out_height, mu.out_width) != (ho, wo):
            from .matte import HipMatteUp
            mu = self._matte_up = HipMatteUp(self.height, self.width, ho, wo, device=device)
        return mu

    def _detail_op(self, size: dict, device):
        """`detail.HipDetail` of an output size: rebuilt when the size or the filter changes, kept otherwise"""
        ho, wo, resample = size["height"], size["width"], size["resample"]
        dt = self._detail_dev
        if dt is None or (dt.out_height, dt.out_width, dt.resample) != (ho, wo, resample):
            from .detail import HipDetail
            dt = self._detail_dev = HipDetail(self.height, self.width, ho, wo, resample, device=device)
        return dt

    def _size_op(self, size: dict, device):
        """`resize.HipResize` of an output size: rebuilt when the size or the filter changes, kept otherwise"""
        ho, wo, resample = size["height"], size["width"], size["resample"]
        rs = self._size_dev
        if rs is None or (rs.out_height, rs.out_width, rs.resample) != (ho, wo, resample):
            from .resize import HipResize
            rs = self._size_dev = HipResize(self.height, self.width, ho, wo, resample, device=device)
        return rs

    def _encoder(self, size: Optional[dict], device):
        """`jpeg_io.HipJpegEncoder` of the size a frame leaves at, made on first use: `self.jpeg` for the UNet's own size (`size`
        None), one per output size in `_size_jpeg` (which `clear_output_size` drops)"""
        if size is None:
            hw, enc = (self.height, self.width), self.jpeg
        else:
            hw, self._size_jpeg = (size["height"], size["width"]), self._size_jpeg or {}
            enc = self._size_jpeg.get(hw)
        if enc is None:
            from .jpeg_io import HipJpegEncoder
            enc = HipJpegEncoder(*hw, self.jpeg_quality, device=device)
            if size is None:
                self.jpeg = enc
            else:
                self._size_jpeg[hw] = enc
        return enc

    @staticmethod
    def get_model_prefix(config_path: str, few_step_model_type: str, use_tiny_vae: bool, num_denoising_steps: int, height: int,
                         width: int, dreambooth: Optional[str] = None, lora_dict: Optional[dict] = None) -> str:
        """the reference's engine prefix (wrapper.py:299-332)"""
        cfg = load_config(config_path)
        db, loras = _style(cfg, dreambooth, None)
        merged = dict(lora_dict or {})
        for k, v in loras.items():
            merged.setdefault(k, v)
        prefix = f"{Path(db).stem if db else 'sd15'}--{few_step_model_type}--step{num_denoising_steps}--"
        for k, v in merged.items():
            prefix += f"{Path(k).stem}-{v}--"
        return prefix + f"tiny_vae-{use_tiny_vae}--h-{height}--w-{width}"
