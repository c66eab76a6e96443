"""Weight ingestion for the packed-weight cache: third-party style checkpoints -> the
reference-keyed UNet state dict that `HipStreamingUNet` packs (and `save_packed` caches on disk).

The reference does this on live `nn.Module`s before the accelerator is built (wrapper.py:417-466):
  * a DreamBooth checkpoint in LDM / CompVis key layout is renamed to diffusers keys and loaded over the spatial weights
    (animatediff/converter/convert.py:26-38 -> convert_from_ckpt.py:245-474 `convert_ldm_unet_checkpoint`);
  * kohya-style LoRA files are merged into the weights, `W += alpha * up @ down`
    (convert.py:72-88 -> convert_lora_safetensor_to_diffusers.py:22-101 `convert_lora_model_level`), for the streaming and
    the warm-up UNet alike (convert.py:106-134) -- which share ONE set of weights here.
This module does the same on plain state dicts (no module tree, no diffusers): key renaming from the UNet topology, and a
LoRA merge that resolves kohya's underscore-flattened module names against the state-dict keys.  Both are pinned against
the reference's own functions run in the build container (tests/golden/gen_golden_convert.py -> convert_*.json / .npz).
"""
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .config import UNetConfig

LDM_UNET_PREFIX = "model.diffusion_model."

_RESNET = (("in_layers.0", "norm1"), ("in_layers.2", "conv1"), ("emb_layers.1", "time_emb_proj"), ("out_layers.0", "norm2"),
           ("out_layers.3", "conv2"), ("skip_connection", "conv_shortcut"))


def ldm_unet_key_map(cfg: UNetConfig) -> Dict[str, str]:
    """{LDM module prefix -> diffusers module prefix} for the SD-1.x UNet topology described by `cfg`
    (what convert_from_ckpt.py:245-474 derives by scanning the checkpoint).  Prefixes, without `.weight` / `.bias`."""
    m = {"time_embed.0": "time_embedding.linear_1", "time_embed.2": "time_embedding.linear_2", "input_blocks.0.0": "conv_in",
         "out.0": "conv_norm_out", "out.2": "conv_out"}
    nl, lpb = cfg.num_levels, cfg.layers_per_block

    def resnet(old, new):
        for a, b in _RESNET:
            m[f"{old}.{a}"] = f"{new}.{b}"

    i = 1
    for lvl in range(nl):
        for j in range(lpb):
            resnet(f"input_blocks.{i}.0", f"down_blocks.{lvl}.resnets.{j}")
            if lvl != nl - 1:
                m[f"input_blocks.{i}.1"] = f"down_blocks.{lvl}.attentions.{j}"
            i += 1
        if lvl != nl - 1:
            m[f"input_blocks.{i}.0.op"] = f"down_blocks.{lvl}.downsamplers.0.conv"
            i += 1
    resnet("middle_block.0", "mid_block.resnets.0")
    m["middle_block.1"] = "mid_block.attentions.0"
    resnet("middle_block.2", "mid_block.resnets.1")
    i = 0
    for lvl in range(nl):
        for j in range(lpb + 1):
            resnet(f"output_blocks.{i}.0", f"up_blocks.{lvl}.resnets.{j}")
            has_attn = lvl != 0
            if has_attn:
                m[f"output_blocks.{i}.1"] = f"up_blocks.{lvl}.attentions.{j}"
            if j == lpb and lvl != nl - 1:
                m[f"output_blocks.{i}.{2 if has_attn else 1}.conv"] = f"up_blocks.{lvl}.upsamplers.0.conv"
            i += 1
    return m


def convert_ldm_unet_checkpoint(checkpoint: Dict[str, torch.Tensor], cfg: UNetConfig) -> Dict[str, torch.Tensor]:
    """LDM-layout checkpoint (keys `model.diffusion_model.*`; other entries ignored) -> diffusers-keyed spatial UNet weights.
    Same result as the reference's convert_ldm_unet_checkpoint for the SD-1.x topology (non-EMA weights)."""
    kmap = ldm_unet_key_map(cfg)
    prefixes = sorted(kmap, key=len, reverse=True)
    out = {}
    for k, v in checkpoint.items():
        if not k.startswith(LDM_UNET_PREFIX):
            continue
        name = k[len(LDM_UNET_PREFIX):]
        for p in prefixes:
            if name == p or name.startswith(p + "."):
                out[kmap[p] + name[len(p):]] = v
                break
        else:
            raise KeyError(f"LDM UNet key {k!r} has no place in the SD-1.x topology of this config")
    return out


def _flatten(key: str) -> str:
    return key.replace(".", "_")


def lora_pairs(lora_sd: Dict[str, torch.Tensor], prefix: str = "lora_unet") -> Iterable[Tuple[str, torch.Tensor, torch.Tensor]]:
    """(flattened module name, up, down) for every UNet LoRA pair of a kohya-style state dict; `.alpha` entries are skipped
    like the reference does (convert_lora_safetensor_to_diffusers.py:35-36: the strength is the caller's `alpha`)."""
    for k in lora_sd:
        if ".alpha" in k or "lora_down" not in k or "text" in k or not k.startswith(prefix + "_"):
            continue
        up = k.replace("lora_down", "lora_up")
        yield k.split(".")[0][len(prefix) + 1:], lora_sd[up], lora_sd[k]


def merge_lora(sd: Dict[str, torch.Tensor], lora_sd: Dict[str, torch.Tensor], alpha: float = 0.6, strict: bool = False) -> List[str]:
    """In place: sd[weight] += alpha * up @ down for every UNet pair of a kohya LoRA (reference
    convert_lora_safetensor_to_diffusers.py:22-101).  Returns the touched keys.  Pairs whose module does not exist in `sd`
    raise with strict=True, else are skipped (the reference's attribute walk would raise)."""
    flat = {_flatten(k[: -len(".weight")]): k for k in sd if k.endswith(".weight")}
    touched = []
    for name, up, down in lora_pairs(lora_sd):
        key = flat.get(name)
        if key is None:
            if strict:
                raise KeyError(f"LoRA module {name!r} not found in the UNet state dict")
            continue
        w = sd[key]
        u, d = up.to(torch.float32), down.to(torch.float32)
        if "conv_in" in name:
            # the streaming UNet's conv_in may be wider than the LoRA's 4 input channels: only the first 4 are touched (:75-81)
            delta = (u.reshape(u.shape[0], -1) @ d.reshape(d.shape[0], -1)).reshape(w.shape[0], 4, *w.shape[2:])
            w32 = w.to(torch.float32).clone()          # (never the caller's tensor: `.to` is a no-op on fp32 weights)
            w32[:, :4] += alpha * delta
        elif "conv" in name:
            delta = (u.reshape(u.shape[0], -1) @ d.reshape(d.shape[0], -1)).reshape(w.shape)
            w32 = w.to(torch.float32) + alpha * delta
        elif up.dim() == 4:
            delta = (u.squeeze(3).squeeze(2) @ d.squeeze(3).squeeze(2)).unsqueeze(2).unsqueeze(3)
            w32 = w.to(torch.float32) + alpha * delta
        else:
            w32 = w.to(torch.float32) + alpha * (u @ d)
        sd[key] = w32.to(w.dtype)
        touched.append(key)
    return touched


def merge_motion_checkpoint(sd: Dict[str, torch.Tensor], ckpt: Dict) -> List[str]:
    """In place: the `live2diff.ckpt` merge of the reference (animatediff/pipeline/pipeline_animatediff_depth.py:281-290):
    take `ckpt["state_dict"]` when present, strip `module.` from the keys, drop the `grid` buffers, load the rest over the
    UNet weights (`load_state_dict(strict=False)` + the reference's `assert len(unexpected) == 0`).  Returns the keys set."""
    state = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    state = {k.replace("module.", ""): v for k, v in state.items() if "grid" not in k and torch.is_tensor(v)}
    unexpected = [k for k in state if k not in sd]
    if unexpected:
        raise KeyError(f"Find unexpected keys ({len(unexpected)}): {unexpected[:5]}")
    for k, v in state.items():
        if tuple(v.shape) != tuple(sd[k].shape):
            raise ValueError(f"{k}: checkpoint tensor {tuple(v.shape)} != UNet parameter {tuple(sd[k].shape)}")
        sd[k] = v.to(sd[k].dtype)
    return list(state)


_DOWN_TAGS = (".lora_down.weight", ".lora.down.weight", ".lora_A.weight", "_lora.down.weight")
_UP_OF = {".lora_down.weight": ".lora_up.weight", ".lora.down.weight": ".lora.up.weight", ".lora_A.weight": ".lora_B.weight",
          "_lora.down.weight": "_lora.up.weight"}


def few_step_lora_pairs(lora_sd: Dict[str, torch.Tensor]):
    """(state-dict weight key candidate, up, down, alpha or None) for every UNet pair of a few-step (LCM) LoRA file.  The
    published `latent-consistency/lcm-lora-sdv1-5` file is kohya-keyed (`lora_unet_<flattened module>.lora_down.weight` +
    `.alpha`); diffusers 0.25.0's loader (the third-party code behind wrapper.py:451-452 -> pipeline/loader.py:12-31,
    `LoraLoaderMixin.lora_state_dict`) also accepts its own layouts, which are resolved here too:
    `unet.<module>.lora.down.weight`, `unet.<module>.lora_A.weight` (peft) and the attention-processor form
    `unet.<block>.attn1.processor.to_q_lora.down.weight`.  The first tuple element is the flattened (underscore) module
    name for kohya keys and the dotted module path otherwise."""
    for k, down in lora_sd.items():
        tag = next((t for t in _DOWN_TAGS if k.endswith(t)), None)
        if tag is None or "text" in k.split(".")[0]:
            continue
        up = lora_sd[k[: -len(tag)] + _UP_OF[tag]]
        stem = k[: -len(tag)]
        if stem.startswith("lora_unet_"):
            yield ("flat", stem[len("lora_unet_"):], up, down, lora_sd.get(stem + ".alpha"))
            continue
        if stem.startswith("lora_te"):
            continue
        if stem.startswith("unet."):
            stem = stem[len("unet."):]
        stem = stem.replace(".processor.", ".")                     # attn1.processor.to_q(_lora) -> attn1.to_q
        if stem.endswith("to_out"):
            stem += ".0"                                           # processor form names the Sequential, the weight is its [0]
        yield ("dotted", stem, up, down, lora_sd.get(k[: -len(tag)] + ".alpha"))


def merge_few_step_lora(sd: Dict[str, torch.Tensor], lora_sd: Dict[str, torch.Tensor], lora_scale: float = 1.0,
                        strict: bool = True) -> List[str]:
    """In place: `W += lora_scale * (alpha / rank) * up @ down` for every UNet pair -- the arithmetic of diffusers 0.25.0's
    `fuse_lora` (`LoRACompatibleLinear._fuse_lora` / `LoRACompatibleConv._fuse_lora`: `w + lora_scale * bmm(up, down)` with
    `network_alpha / rank` folded into `up`), which the reference calls through `stream.load_lora(few_step_lora);
    stream.fuse_lora()` (wrapper.py:451-452) BEFORE `prepare_cache` projects the positional-encoding tables (:454-459) --
    so a few-step LoRA that targets motion-module projections must be merged before `HipStreamingUNet` packs the weights,
    which is exactly where `build_state_dict` puts it.  diffusers is not in /root/reference: **parity unpinned**, checked
    against the formula (tests/test_convert.py).  Unresolved modules raise with strict=True (default), like the loader."""
    flat = {_flatten(k[: -len(".weight")]): k for k in sd if k.endswith(".weight")}
    touched = []
    for kind, name, up, down, alpha in few_step_lora_pairs(lora_sd):
        key = flat.get(name) if kind == "flat" else (name + ".weight" if name + ".weight" in sd else None)
        if key is None:
            if strict:
                raise KeyError(f"few-step LoRA module {name!r} not found in the UNet state dict")
            continue
        w = sd[key]
        u, d = up.to(torch.float32), down.to(torch.float32)
        rank = d.shape[0]
        scale = lora_scale * (float(alpha) / rank if alpha is not None else 1.0)
        delta = (u.reshape(u.shape[0], -1) @ d.reshape(d.shape[0], -1)).reshape(w.shape)
        sd[key] = (w.to(torch.float32) + scale * delta).to(w.dtype)
        touched.append(key)
    if strict and not touched:
        raise ValueError("the few-step LoRA touched no UNet weight: unknown key layout")
    return touched


def build_state_dict(base_sd: Dict[str, torch.Tensor], cfg: UNetConfig, dreambooth: Optional[Dict[str, torch.Tensor]] = None,
                     loras: Optional[List[Tuple[Dict[str, torch.Tensor], float]]] = None,
                     motion_ckpt: Optional[Dict] = None, few_step_lora: Optional[Dict[str, torch.Tensor]] = None,
                     strict_lora: bool = True) -> Dict[str, torch.Tensor]:
    """The reference's ingestion order on state dicts, from raw checkpoints alone:
      1. base SD-1.5 UNet weights inflated into the streaming topology (`from_pretrained_2d`: the caller's `base_sd`);
      2. `motion_ckpt` = live2diff.ckpt over them (pipeline_animatediff_depth.py:281-290, `merge_motion_checkpoint`);
      3. DreamBooth spatial weights (`load_third_party_checkpoints`, :303; `load_state_dict(strict=False)`: motion modules
         keep their weights);
      4. the few-step (LCM) LoRA at scale 1 (wrapper.py:451-452) -- before the PE tables are projected (:454-459), i.e. before
         packing;
      5. each user LoRA at its strength (wrapper.py:461-466; kohya files, convert.py:72-88).
    A LoRA that resolves against NO weight raises (strict_lora=False: warns) instead of silently merging nothing.
    The result is what `HipStreamingUNet(state_dict, ...)` packs and `save_packed` caches
    (cache name: `HipStreamingUNet.packed_cache_name`)."""
    sd = dict(base_sd)
    if motion_ckpt is not None:
        merge_motion_checkpoint(sd, motion_ckpt)
    if dreambooth is not None:
        conv = convert_ldm_unet_checkpoint(dreambooth, cfg)
        unknown = [k for k in conv if k not in sd]
        if unknown:
            raise KeyError(f"{len(unknown)} converted DreamBooth keys are not UNet parameters, e.g. {unknown[:3]}")
        for k, v in conv.items():
            if tuple(v.shape) != tuple(sd[k].shape):
                raise ValueError(f"{k}: DreamBooth tensor {tuple(v.shape)} != UNet parameter {tuple(sd[k].shape)}")
            sd[k] = v.to(sd[k].dtype)
    if few_step_lora is not None:
        merge_few_step_lora(sd, few_step_lora, 1.0, strict=strict_lora)
    for lora_sd, alpha in (loras or []):
        touched = merge_lora(sd, lora_sd, alpha)
        n_pairs = sum(1 for _ in lora_pairs(lora_sd))
        if len(touched) < n_pairs or not touched:
            msg = (f"LoRA merge resolved {len(touched)} of {n_pairs} UNet pairs against the state dict (a peft / diffusers-"
                   "keyed file, or another topology?)")
            if strict_lora:
                raise KeyError(msg)
            import warnings
            warnings.warn(msg)
    return sd


def load_safetensors(path: str) -> Dict[str, torch.Tensor]:
    from safetensors import safe_open
    with safe_open(path, framework="pt", device="cpu") as f:
        return {k: f.get_tensor(k) for k in f.keys()}


# ----------------------------------------------------------------------------- text encoder
LDM_CLIP_PREFIX = "cond_stage_model.transformer."


def convert_ldm_clip_checkpoint(dreambooth_sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The text-encoder half of an LDM / CompVis checkpoint: `cond_stage_model.transformer.` stripped (reference
    convert_from_ckpt.py:591-599; keys come out as transformers 4.x names, `text_model.` prefix included).  Divergence: the
    reference loads the result with `strict=False` (converter/convert.py:47-50), so a checkpoint without these keys loads nothing
    and says nothing; here a checkpoint with no text-encoder key raises."""
    out = {k[len(LDM_CLIP_PREFIX):]: v for k, v in dreambooth_sd.items() if k.startswith(LDM_CLIP_PREFIX)}
    if not out:
        raise KeyError(f"no `{LDM_CLIP_PREFIX}*` key in the checkpoint: it carries no text encoder")
    return out


def merge_text_lora(sd: Dict[str, torch.Tensor], lora_sd: Dict[str, torch.Tensor], alpha: float = 0.6) -> List[str]:
    """In place: W += alpha * up @ down for every `lora_te_*` pair of a kohya LoRA (reference
    convert_lora_safetensor_to_diffusers.py:38-41, 88-91), the flattened module name resolved against the text-encoder keys
    (with or without `text_model.`).  Per-module `.alpha` entries are skipped, as the reference does.  Returns the touched keys;
    a pair whose module is not in `sd` raises (the reference's attribute walk would)."""
    flat = {}
    for k in sd:
        if k.endswith(".weight"):
            m = k[: -len(".weight")]
            flat[_flatten(m if m.startswith("text_model.") else "text_model." + m)] = k
    touched = []
    for k in lora_sd:
        if ".alpha" in k or "lora_down" not in k or not k.startswith("lora_te_"):
            continue
        name = k.split(".")[0][len("lora_te_"):]
        key = flat.get(name)
        if key is None:
            raise KeyError(f"text LoRA module {name!r} not found in the text-encoder state dict")
        up, down = lora_sd[k.replace("lora_down", "lora_up")].to(torch.float32), lora_sd[k].to(torch.float32)
        w = sd[key]
        delta = up.reshape(up.shape[0], -1) @ down.reshape(down.shape[0], -1)
        sd[key] = (w.to(torch.float32) + alpha * delta.reshape(w.shape)).to(w.dtype)
        touched.append(key)
    return touched


def build_text_encoder_state_dict(base_sd: Dict[str, torch.Tensor], dreambooth: Optional[Dict[str, torch.Tensor]] = None,
                                  loras: Optional[List[Tuple[Dict[str, torch.Tensor], float]]] = None) -> Dict[str, torch.Tensor]:
    """The text half of a style, in the reference's order: base text encoder, the DreamBooth checkpoint's text encoder over it
    (converter/convert.py:47-50), then each LoRA's `lora_te_*` pairs at its strength (:72-88).  Keys of the result are the
    base dict's; DreamBooth keys are matched with or without the `text_model.` prefix."""
    sd = dict(base_sd)
    if dreambooth is not None:
        strip = lambda k: k[len("text_model."):] if k.startswith("text_model.") else k
        by_stem = {strip(k): k for k in sd}
        conv = convert_ldm_clip_checkpoint(dreambooth)
        n = 0
        for k, v in conv.items():
            key = by_stem.get(strip(k))
            if key is None:
                continue                  # (the reference's strict=False: e.g. position_ids)
            if tuple(v.shape) != tuple(sd[key].shape):
                raise ValueError(f"{key}: DreamBooth tensor {tuple(v.shape)} != text-encoder parameter {tuple(sd[key].shape)}")
            sd[key] = v.to(sd[key].dtype)
            n += 1
        if n == 0:
            raise KeyError("the checkpoint's text-encoder keys match no parameter of the base text encoder")
    for lora_sd, alpha in (loras or []):
        merge_text_lora(sd, lora_sd, alpha)
    return sd


# ----------------------------------------------------------------------------- the VAE half of a style (SD AutoencoderKL)
LDM_VAE_PREFIX = "first_stage_model."


def ldm_vae_key_map() -> Dict[str, str]:
    """LDM VAE key (without `first_stage_model.`) -> diffusers AutoencoderKL key, as the reference's convert_ldm_vae_checkpoint
    (convert_from_ckpt.py:476) renames them: `down.i.block.j` -> `down_blocks.i.resnets.j`, `up.(3 - i)` -> `up_blocks.i`,
    `mid.block_k` -> `mid_block.resnets.(k - 1)`, `mid.attn_1.{norm,q,k,v,proj_out}` -> `mid_block.attentions.0.{group_norm,
    to_q,to_k,to_v,to_out.0}`, `nin_shortcut` -> `conv_shortcut`, `norm_out` -> `conv_norm_out`."""
    from .vae_kl_hip import BLOCK_OUT, DEC_LAYERS, ENC_LAYERS
    m: Dict[str, str] = {}
    n = len(BLOCK_OUT)

    def wb(old, new):
        for leaf in ("weight", "bias"):
            m[f"{old}.{leaf}"] = f"{new}.{leaf}"

    def resnet(old, new, cin, cout):
        for part in ("norm1", "conv1", "norm2", "conv2"):
            wb(f"{old}.{part}", f"{new}.{part}")
        if cin != cout:
            wb(f"{old}.nin_shortcut", f"{new}.conv_shortcut")

    def mid(side):
        c = BLOCK_OUT[-1]
        for k in (1, 2):
            resnet(f"{side}.mid.block_{k}", f"{side}.mid_block.resnets.{k - 1}", c, c)
        for old, new in (("norm", "group_norm"), ("q", "to_q"), ("k", "to_k"), ("v", "to_v"), ("proj_out", "to_out.0")):
            wb(f"{side}.mid.attn_1.{old}", f"{side}.mid_block.attentions.0.{new}")

    for side in ("encoder", "decoder"):
        wb(f"{side}.conv_in", f"{side}.conv_in")
        wb(f"{side}.conv_out", f"{side}.conv_out")
        wb(f"{side}.norm_out", f"{side}.conv_norm_out")
    cin = BLOCK_OUT[0]
    for i, c in enumerate(BLOCK_OUT):
        for j in range(ENC_LAYERS):
            resnet(f"encoder.down.{i}.block.{j}", f"encoder.down_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        cin = c
        if i < n - 1:
            wb(f"encoder.down.{i}.downsample.conv", f"encoder.down_blocks.{i}.downsamplers.0.conv")
    mid("encoder")
    mid("decoder")
    cin = BLOCK_OUT[-1]
    for i, c in enumerate(reversed(BLOCK_OUT)):
        blk = n - 1 - i
        for j in range(DEC_LAYERS):
            resnet(f"decoder.up.{blk}.block.{j}", f"decoder.up_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        cin = c
        if i < n - 1:
            wb(f"decoder.up.{blk}.upsample.conv", f"decoder.up_blocks.{i}.upsamplers.0.conv")
    wb("quant_conv", "quant_conv")
    wb("post_quant_conv", "post_quant_conv")
    return m


def convert_ldm_vae_checkpoint(checkpoint: Dict[str, torch.Tensor], prefix: str = LDM_VAE_PREFIX) -> Dict[str, torch.Tensor]:
    """LDM VAE tensors (under `prefix`) -> diffusers names.  The attention projections, 1x1 convs in LDM checkpoints, come out
    as [512, 512] linear weights, as the reference's converter leaves them.  A missing key raises KeyError."""
    out = {}
    for old, new in ldm_vae_key_map().items():
        k = prefix + old
        if k not in checkpoint:
            raise KeyError(f"VAE checkpoint lacks {k}")
        t = checkpoint[k]
        if ".attentions.0.to_" in new and t.dim() == 4:
            t = t[:, :, 0, 0]
        out[new] = t
    return out


def build_vae_state_dict(base_vae_sd: Dict[str, torch.Tensor], dreambooth: Optional[Dict[str, torch.Tensor]] = None,
                         vae: Optional[Dict] = None) -> Dict[str, torch.Tensor]:
    """The VAE half of the reference's load_third_party_checkpoints (convert.py:40-45, :52-69): the base AutoencoderKL state dict
    (diffusers names), replaced by a DreamBooth checkpoint's `first_stage_model.*` tensors and then by a standalone VAE file in LDM
    layout (possibly under `state_dict`), in that order."""
    sd = dict(base_vae_sd)
    if dreambooth is not None:
        if "state_dict" in dreambooth:
            dreambooth = dreambooth["state_dict"]
        sd.update(convert_ldm_vae_checkpoint(dreambooth))
    if vae is not None:
        if "state_dict" in vae:
            vae = vae["state_dict"]
        sd.update(convert_ldm_vae_checkpoint({LDM_VAE_PREFIX + k: v for k, v in vae.items()}))
    return sd


# ----------------------------------------------------------------------------- the `from_pretrained_2d` step
def inflate_2d_unet(sd2d: Dict[str, torch.Tensor], cfg: UNetConfig, dtype=torch.float16) -> Dict[str, torch.Tensor]:
    """The state-dict form of the reference's `UNet3DConditionStreamingModel.from_pretrained_2d` (unet_depth_streaming.py; called at
    pipeline_animatediff_depth.py:273-277): every key of `weights.unet_param_spec(cfg)`, taken from the diffusers 2D UNet file
    where it has it and a ZERO placeholder of the spec's shape otherwise (motion modules, the depth mapping network) --
    `merge_motion_checkpoint` requires every key it sets to exist already.  The caller checks after `build_state_dict` that no
    placeholder (a spec key absent from `sd2d`) survived: the reference would silently keep a random init."""
    from .weights import unet_param_spec
    out = {}
    for k, shp in unet_param_spec(cfg).items():
        if k in sd2d:
            if tuple(sd2d[k].shape) != tuple(shp):
                raise ValueError(f"{k}: 2D UNet tensor {tuple(sd2d[k].shape)} != streaming UNet parameter {tuple(shp)}")
            out[k] = sd2d[k].to(dtype)
        else:
            out[k] = torch.zeros(shp, dtype=dtype)
    return out
