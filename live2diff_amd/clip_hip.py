"""HipClipTextEncoder -- the text encoder in front of the UNet's cross-attention.

Boundary (reference): `AnimationDepthPipeline._encode_prompt` (live2diff/animatediff/pipeline/pipeline_animatediff_depth.py:149-248),
which tokenizes the prompt and runs transformers' `CLIPTextModel` (SD-1.x: CLIP ViT-L/14's text tower) to the `[B, 77, 768]`
embeddings; with `clip_skip = k` it takes `hidden_states[-(k + 1)]` (the output of layer 12 - k) through the final LayerNorm.
`HipPromptEncoder._encode_prompt` has that method's signature and return convention, so it can be set as `pipe._encode_prompt`.

The network runs as one static plan per (batch, layers) on the kernels of csrc/clip.hip: an embedding gather, five launches per
layer (q|k|v with the LayerNorm in front, causal attention, out_proj + residual, fc1 with the LayerNorm in front and quick-GELU
behind, fc2 + residual) and the final LayerNorm -- 5 (12 - clip_skip) + 2 launches, nothing but the ids upload in front of them.
State-dict keys are transformers' names, with or without the `text_model.` prefix (4.x / 5.x).
"""
import json
import os
import zlib
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib, ops


@dataclass(frozen=True)
class ClipTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


SD15_CLIP = ClipTextConfig()


def tiny_clip_config() -> ClipTextConfig:
    """3 heads of 64, 3 layers, a 1000-token vocabulary: the smallest shapes the kernels take (K % 192 == 0)."""
    return ClipTextConfig(vocab_size=1000, hidden_size=192, intermediate_size=384, num_hidden_layers=3, num_attention_heads=3)


def config_from_json(d: dict) -> ClipTextConfig:
    """transformers' CLIPTextConfig (config.json of a diffusers `text_encoder/`)."""
    act = d.get("hidden_act", "quick_gelu")
    if act != "quick_gelu":
        raise ValueError(f"text encoder activation {act!r}: only SD-1.x's quick_gelu CLIP is supported")
    return ClipTextConfig(vocab_size=d["vocab_size"], hidden_size=d["hidden_size"], intermediate_size=d["intermediate_size"],
                          num_hidden_layers=d["num_hidden_layers"], num_attention_heads=d["num_attention_heads"],
                          max_position_embeddings=d["max_position_embeddings"], layer_norm_eps=d.get("layer_norm_eps", 1e-5))


def clip_text_spec(cfg: ClipTextConfig = SD15_CLIP) -> Dict[str, tuple]:
    """Parameter inventory, transformers 5.x names (CLIPTextModel.state_dict(); 4.x adds the `text_model.` prefix)."""
    C, F = cfg.hidden_size, cfg.intermediate_size
    spec = OrderedDict()
    spec["embeddings.token_embedding.weight"] = (cfg.vocab_size, C)
    spec["embeddings.position_embedding.weight"] = (cfg.max_position_embeddings, C)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            spec[p + f"self_attn.{n}.weight"] = (C, C)
            spec[p + f"self_attn.{n}.bias"] = (C,)
        spec[p + "layer_norm1.weight"] = (C,)
        spec[p + "layer_norm1.bias"] = (C,)
        spec[p + "mlp.fc1.weight"] = (F, C)
        spec[p + "mlp.fc1.bias"] = (F,)
        spec[p + "mlp.fc2.weight"] = (C, F)
        spec[p + "mlp.fc2.bias"] = (C,)
        spec[p + "layer_norm2.weight"] = (C,)
        spec[p + "layer_norm2.bias"] = (C,)
    spec["final_layer_norm.weight"] = (C,)
    spec["final_layer_norm.bias"] = (C,)
    return spec


def random_clip_text_state_dict(cfg: ClipTextConfig = SD15_CLIP, seed: int = 0, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """Key-hashed deterministic weights (generator seeded with crc32(f"clip{seed}." + key)), rounded through fp16 so that the
    fp32 restatement and the fp16 encoder see the same numbers: embeddings randn * 0.02 (position 0.01), LayerNorm gains
    1 +- 0.1, biases 0.05 * randn, weights randn * fan_in^-0.5."""
    out = OrderedDict()
    for k, shp in clip_text_spec(cfg).items():
        g = torch.Generator(device="cpu")
        g.manual_seed(zlib.crc32(f"clip{seed}.{k}".encode()) & 0x7FFFFFFF)
        x = torch.randn(shp, generator=g, dtype=torch.float32)
        if "embedding" in k:
            x = x * (0.01 if "position" in k else 0.02)
        elif k.endswith("bias"):
            x = 0.05 * x
        elif "layer_norm" in k:
            x = 1.0 + 0.1 * x
        else:
            x = x * shp[1] ** -0.5
        out[k] = x.to(torch.float16).to(dtype)
    return out


def normalize_keys(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """transformers 4.x `text_model.` prefix stripped; the `position_ids` buffer dropped."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith("text_model."):
            k = k[len("text_model."):]
        if k.endswith("position_ids"):
            continue
        out[k] = v
    return out


def clip_launches(cfg: ClipTextConfig, clip_skip: Optional[int]) -> int:
    """launches of one encode: embedding + 5 per layer run + final LayerNorm"""
    return 5 * (cfg.num_hidden_layers - (clip_skip or 0)) + 2


class HipClipTextEncoder:
    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", config: Optional[ClipTextConfig] = None,
                 use_graph: bool = True):
        self.cfg = cfg = config or SD15_CLIP
        self.device = torch.device(device)
        self.use_graph = use_graph and not ops.DRY_RUN
        sd = normalize_keys(state_dict)
        missing = [k for k in clip_text_spec(cfg) if k not in sd]
        if missing:
            raise KeyError(f"CLIP text state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
        g = lambda k: sd[k].to(self.device)
        f32 = lambda k: g(k).float().contiguous()
        self.tok = g("embeddings.token_embedding.weight").to(torch.float16).contiguous()
        self.pos = g("embeddings.position_embedding.weight").to(torch.float16).contiguous()
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            L = {}
            L["qkv.w"] = ops.pack_clip_linear(torch.cat([g(a + f"{n}_proj.weight") for n in "qkv"]))
            L["qkv.b"] = torch.cat([f32(a + f"{n}_proj.bias") for n in "qkv"]).contiguous()
            L["out.w"], L["out.b"] = ops.pack_clip_linear(g(a + "out_proj.weight")), f32(a + "out_proj.bias")
            L["fc1.w"], L["fc1.b"] = ops.pack_clip_linear(g(p + "mlp.fc1.weight")), f32(p + "mlp.fc1.bias")
            L["fc2.w"], L["fc2.b"] = ops.pack_clip_linear(g(p + "mlp.fc2.weight")), f32(p + "mlp.fc2.bias")
            for n in (1, 2):
                L[f"ln{n}.g"], L[f"ln{n}.b"] = f32(p + f"layer_norm{n}.weight"), f32(p + f"layer_norm{n}.bias")
            self.layers.append(L)
        self.ln_g, self.ln_b = f32("final_layer_norm.weight"), f32("final_layer_norm.bias")
        from .unet_hip import own_storage
        top = {"tok": self.tok, "pos": self.pos, "ln_g": self.ln_g, "ln_b": self.ln_b}
        for d in [top] + self.layers:                  # (load_mix overwrites these in place: never the caller's tensors)
            own_storage(d, sd)
        self.tok, self.pos, self.ln_g, self.ln_b = top["tok"], top["pos"], top["ln_g"], top["ln_b"]
        self.layer_weight_bytes = sum(t.numel() * t.element_size() for L in self.layers for t in L.values())
        self._plans = {}
        self._blender = None

    # ------------------------------------------------------------------ packed weights / style switch (style_bank.py)
    def _flat(self) -> Dict[str, torch.Tensor]:
        W = {"tok": self.tok, "pos": self.pos, "ln_g": self.ln_g, "ln_b": self.ln_b}
        for i, L in enumerate(self.layers):
            for k, t in L.items():
                W[f"layers.{i}.{k}"] = t
        return W

    def _packed_meta(self) -> dict:
        return dict(kind="clip_text", abi=str(_lib.ABI_VERSION), config=json.dumps(self.cfg.__dict__, sort_keys=True))

    def packed_state(self):
        """The packed weights of this instance as (tensors, metadata): `tok`, `pos`, every tensor of `layers[i]`, `ln_g`, `ln_b`."""
        from .unet_hip import PackedWeights
        return PackedWeights(self._flat(), self._packed_meta())

    def load_mix(self, sets, weights) -> None:
        """Overwrite the weights IN PLACE with sum_k weights[k] * sets[k] (each the `packed_state()` of an encoder of this
        configuration), one launch on the current stream.  Plans and captured graphs keep their pointers."""
        from .style_bank import WeightBlender
        from .unet_hip import PackedWeights
        sets, weights = list(sets), list(weights)
        own = self._packed_meta()
        flat = self._flat()
        for j, ps in enumerate(sets):
            if not isinstance(ps, PackedWeights):
                raise TypeError(f"load_mix: set {j} is {type(ps).__name__}, need PackedWeights (packed_state())")
            if dict(ps.meta) != own:
                raise ValueError(f"style set {j}: packed for text encoder {ps.meta}, this instance is {own}: re-pack from the state dict")
            if any(ps.W.get(k) is t for k, t in flat.items()):
                raise ValueError(f"load_mix: set {j} holds this instance's own tensors (the destination): blend from a copy")
        if self._blender is None:
            self._blender = WeightBlender(flat, self.device)
        self._blender.apply([ps.W for ps in sets], weights)

    # ------------------------------------------------------------------ plan
    def _layers_run(self, clip_skip: Optional[int]) -> int:
        k = 0 if clip_skip is None else int(clip_skip)
        if not 0 <= k < self.cfg.num_hidden_layers:
            raise ValueError(f"clip_skip {clip_skip} out of range for {self.cfg.num_hidden_layers} layers")
        return self.cfg.num_hidden_layers - k

    def plan(self, B: int, clip_skip: Optional[int] = None, early: Optional[tuple] = None):
        """Static plan of one encode of B prompts.  `early` = (clip_skip, first prompt): prompts from `first` on leave through the
        final LayerNorm after layer 12 - clip_skip, the others after the last layer run (one launch more; the CFG form of the
        reference, whose unconditional half never takes clip_skip)."""
        key = (B, clip_skip, early)
        if key in self._plans:
            return self._plans[key]
        cfg, dev = self.cfg, self.device
        T, C, F, H = cfg.max_position_embeddings, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
        M = B * T
        st = type("ClipPlan", (), {})()
        st.ids = torch.zeros(M, dtype=torch.int64, device=dev)
        st.x = torch.zeros(M, C, dtype=torch.float32, device=dev)           # residual stream
        st.qkv = torch.zeros(M, 3 * C, dtype=torch.float16, device=dev)
        st.attn = torch.zeros(M, C, dtype=torch.float16, device=dev)
        st.hid = torch.zeros(M, F, dtype=torch.float16, device=dev)
        st.out = torch.zeros(B, T, C, dtype=torch.float16, device=dev)
        pl = st.pl = _lib.OpList()
        add = lambda opk: pl.append(*opk)
        n_run = self._layers_run(clip_skip)
        e_layers, e_row = (None, M) if early is None else (self._layers_run(early[0]), early[1] * T)
        if early is not None and not (0 < early[1] < B and e_layers <= n_run):
            raise ValueError(f"early exit {early} does not fit B = {B}, clip_skip = {clip_skip}")
        add(ops.clip_embed(st.ids, self.tok, self.pos, st.x, rows=M, T=T, C=C, V=cfg.vocab_size, P=cfg.max_position_embeddings))
        eps = cfg.layer_norm_eps
        for i in range(n_run):
            L = self.layers[i]
            add(ops.clip_linear(st.x, L["qkv.w"], st.qkv, M=M, K=C, Nout=3 * C, ldx=C, ldo=3 * C, bias=L["qkv.b"],
                                gamma=L["ln1.g"], beta=L["ln1.b"], eps=eps))
            add(ops.clip_attn(st.qkv, st.attn, B=B, T=T, H=H, d=cfg.head_dim, ldq=3 * C, ldo=C, scale=cfg.head_dim ** -0.5))
            add(ops.clip_linear(st.attn, L["out.w"], st.x, M=M, K=C, Nout=C, ldx=C, ldo=C, bias=L["out.b"],
                                epi=ops.CLIP_EPI_RESIDUAL))
            add(ops.clip_linear(st.x, L["fc1.w"], st.hid, M=M, K=C, Nout=F, ldx=C, ldo=F, bias=L["fc1.b"],
                                gamma=L["ln2.g"], beta=L["ln2.b"], epi=ops.CLIP_EPI_QUICK_GELU, eps=eps))
            add(ops.clip_linear(st.hid, L["fc2.w"], st.x, M=M, K=F, Nout=C, ldx=F, ldo=C, bias=L["fc2.b"],
                                epi=ops.CLIP_EPI_RESIDUAL))
            if i + 1 == e_layers:
                add(ops.clip_ln(st.x, self.ln_g, self.ln_b, st.out, rows=M - e_row, C=C, ldx=C, ldo=C, eps=eps,
                                x_off=e_row * C, o_off=e_row * C))
        add(ops.clip_ln(st.x, self.ln_g, self.ln_b, st.out, rows=e_row, C=C, ldx=C, ldo=C, eps=eps))
        st.graph = None
        self._plans[key] = st
        return st

    def _check_ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        ids = input_ids if input_ids.dim() == 2 else input_ids.view(1, -1)
        T = self.cfg.max_position_embeddings
        if ids.shape[1] != T:
            raise ValueError(f"input_ids {tuple(input_ids.shape)}: expected [B, {T}] (tokenizer padding='max_length')")
        if not ids.is_cuda:
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.cfg.vocab_size:
                raise ValueError(f"token id out of range [0, {self.cfg.vocab_size}): {lo}..{hi}")
        return ids

    def run_plan(self, st, input_ids: torch.Tensor) -> torch.Tensor:
        st.ids.copy_(input_ids.reshape(-1))
        if self.use_graph:
            if st.graph is None:         # (captured on a side stream: the legacy default stream cannot be captured)
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    st.graph = _lib.Graph(st.pl, stream=int(side.cuda_stream))
                torch.cuda.current_stream().wait_stream(side)
            st.graph.launch()
        else:
            st.pl.run()
        return st.out

    @torch.no_grad()
    def encode(self, input_ids: torch.Tensor, clip_skip: Optional[int] = None) -> torch.Tensor:
        """[B, 77] token ids -> [B, 77, hidden] fp16 on the device (a fresh tensor): the last layer's output through the final
        LayerNorm, or with clip_skip = k the output of layer 12 - k through it (diffusers' hidden_states[-(k + 1)])."""
        ids = self._check_ids(input_ids)
        return self.run_plan(self.plan(ids.shape[0], clip_skip), ids).clone()

    @torch.no_grad()
    def encode_cfg(self, input_ids: torch.Tensor, clip_skip: Optional[int] = None) -> torch.Tensor:
        """Prompts [uncond..., cond...] in one launch sequence: the first half through all layers, the second half with
        clip_skip (the reference's CFG convention, pipeline_animatediff_depth.py:176-246)."""
        ids = self._check_ids(input_ids)
        B = ids.shape[0]
        if clip_skip is None:
            return self.encode(ids)
        return self.run_plan(self.plan(B, None, early=(clip_skip, B // 2)), ids).clone()


class HipPromptEncoder:
    """Tokenizer + HipClipTextEncoder behind the reference's `_encode_prompt` signature.  `default_clip_skip` is used when the
    caller omits clip_skip (the mirror's update_prompt does): a clip_skip-2 style needs default_clip_skip=2 so that prompt
    updates stay in the embedding space the stream was prepared in."""

    _UNSET = object()

    def __init__(self, encoder: HipClipTextEncoder, tokenizer, default_clip_skip: Optional[int] = None):
        self.encoder, self.tokenizer, self.default_clip_skip = encoder, tokenizer, default_clip_skip

    def _ids(self, prompts):
        return torch.tensor([self.tokenizer.encode(p) for p in prompts], dtype=torch.int64)

    @torch.no_grad()
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                       clip_skip=_UNSET):
        if clip_skip is HipPromptEncoder._UNSET:
            clip_skip = self.default_clip_skip
        prompts = list(prompt) if isinstance(prompt, (list, tuple)) else [prompt]
        bs = len(prompts)
        if do_classifier_free_guidance:
            if negative_prompt is None:
                uncond = [""] * bs
            elif type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                uncond = [negative_prompt]
            elif len(negative_prompt) != bs:
                raise ValueError(f"`negative_prompt` has batch size {len(negative_prompt)}, but `prompt` has {bs}")
            else:
                uncond = list(negative_prompt)
            emb = self.encoder.encode_cfg(self._ids(uncond + prompts), clip_skip)
            u, c = emb[:len(uncond)], emb[len(uncond):]
            T = emb.shape[1]
            u = u.repeat(1, num_videos_per_prompt, 1).view(len(uncond) * num_videos_per_prompt, T, -1)
            c = c.repeat(1, num_videos_per_prompt, 1).view(bs * num_videos_per_prompt, T, -1)
            emb = torch.cat([u, c])
        else:
            emb = self.encoder.encode(self._ids(prompts), clip_skip)
            T = emb.shape[1]
            emb = emb.repeat(1, num_videos_per_prompt, 1).view(bs * num_videos_per_prompt, T, -1)
        return emb.to(device)


def load_text_encoder(model_dir: str, device="cuda", default_clip_skip: Optional[int] = None) -> HipPromptEncoder:
    """A diffusers-layout model directory: text_encoder/config.json + model.safetensors (or pytorch_model.bin),
    tokenizer/vocab.json + merges.txt (+ special_tokens_map.json / tokenizer_config.json for the pad token)."""
    from .clip_tokenizer import ClipTokenizer

    te = os.path.join(model_dir, "text_encoder")
    with open(os.path.join(te, "config.json")) as f:
        cfg = config_from_json(json.load(f))
    st_path, bin_path = os.path.join(te, "model.safetensors"), os.path.join(te, "pytorch_model.bin")
    if os.path.exists(st_path):
        from safetensors.torch import load_file
        sd = load_file(st_path)
    elif os.path.exists(bin_path):
        sd = torch.load(bin_path, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{te}: neither model.safetensors nor pytorch_model.bin")
    tok = ClipTokenizer.from_dir(os.path.join(model_dir, "tokenizer"), max_length=cfg.max_position_embeddings)
    return HipPromptEncoder(HipClipTextEncoder(sd, device, cfg), tok, default_clip_skip)
