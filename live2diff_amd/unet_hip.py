"""HipStreamingUNet -- the object that occupies the reference's `stream.unet` slot.

Boundary (reference): `StreamAnimateDiffusionDepth.unet`, called at
live2diff/pipeline_stream_animation_depth.py:456-466 with the signature of
`UNet3DConditionStreamingModel.forward` (unet_depth_streaming.py:429-448) /
`UNet2DConditionModelDepthEngine.__call__` (acceleration/tensorrt/engine.py:142-153); the warm-up twin
(`unet_warmup`, unet_depth_warmup.py:407-590, called at pipeline :320-328) is `HipStreamingUNet.warmup`.

Design (MI355X-first, not a module-by-module translation):
  * one channels-last fp16 activation layout `[B*T, C]` end to end; the only layout conversions of a step
    are on the 4-channel latents at the boundary;
  * weights are ingested once from a reference-keyed `state_dict` and re-packed for the kernels
    (3x3 taps-major, q|k fused, q|k|v fused for the temporal layers, GEGLU value/gate interleaved, all
    time_emb_proj / all text K,V projections concatenated into single GEMMs);
  * a UNet step is a static *plan* -- an array of `l2d_op` records, built once per (H, W, N, L) -- that the
    native executor replays (`l2d_run_ops`, or a captured hipGraph): ~650 kernels, no Python in the loop;
  * the KV-cache stays in the reference interchange layout `[N,2,T,L,C]` and is updated IN PLACE, so the
    caller's `kv_cache_list` semantics (pipeline :468-469) hold and nothing cache-sized is ever copied.
No torch compute ops are used on the path (torch provides HBM allocations, the stream, and the tiny
host-to-static-buffer input copies).
"""
from types import SimpleNamespace
from typing import List, Optional

import os
import torch

from . import _lib, ops
from .config import UNetConfig, motion_module_layout
from .unet_plan import TEXT_PAD, UNetPlan
from .unet_pack import own_storage, pack_unet, sinusoid_pe  # noqa: F401  (own_storage / sinusoid_pe: re-exported, clip_hip.py imports the former from here)


class UNetOutput(dict):
    """`out["sample"]`, `out["kv_cache"]`, `out.sample`, `out.kv_cache`, `out[0]`
    (reference UNet3DConditionStreamingOutput, unet_depth_streaming.py:29-32)."""

    def __init__(self, sample, kv_cache):
        super().__init__(sample=sample, kv_cache=kv_cache)
        self.sample, self.kv_cache = sample, kv_cache

    def __getitem__(self, k):
        if isinstance(k, int):
            return (self.sample, self.kv_cache)[k]
        return dict.__getitem__(self, k)


class PackedWeights:
    """Packed weights outside an instance: `W` (name -> device tensor, what `_pack_weights` produced) + `meta` (the strings a
    packed-weight file carries).  Produced by `HipStreamingUNet.packed_state()`, accepted by the constructor -- the unit of the
    multi-GPU weight replication (parallel.replicate_packed_weights: rank 0 packs once, every rank receives the packed tensors)."""
    __slots__ = ("W", "meta")

    def __init__(self, W, meta):
        self.W, self.meta = W, meta


class HipStreamingUNet:
    def __init__(self, state_dict, cfg: UNetConfig, height: int, width: int,
                 denoising_steps_num: int, device="cuda", warmup_frames: Optional[int] = None, use_graph: bool = False,
                 tattn_variant: int = 0, text_len: int = 77, fresh_output: bool = False):
        """height/width are LATENT sizes (image / 8). `state_dict` uses the reference key names; it may also be the
        path of a packed-weight file written by `save_packed`, or ANOTHER HipStreamingUNet of the same
        configuration and latent size whose packed weights this instance then shares (read-only replicas are per GPU, not per
        stream: several independent frame streams on one GPU -- each with its own plan buffers and KV caches, each on its own
        HIP stream -- fill each other's launch gaps)."""
        assert cfg.num_heads == 8 and cfg.temporal_heads == 8
        assert height % 8 == 0 and width % 8 == 0, "latent size must be divisible by 8 (3 down-samplings, T%4==0)"
        self.cfg, self.h, self.w, self.N = cfg, height, width, denoising_steps_num
        self.device = torch.device(device)
        self.F = cfg.sink_size if warmup_frames is None else warmup_frames
        self.use_graph = use_graph
        self.fresh_output = fresh_output   # True: return a private copy of the prediction (the reference's PyTorch path returns a
        #                                    fresh tensor); False (default): a view of the static output buffer, like a TensorRT binding
        self.tattn_variant = tattn_variant
        self.cond_cache = True           # False: re-run the conditioning launches every call (tests)
        assert 1 <= text_len <= TEXT_PAD
        self.text_len = text_len           # static number of text tokens (77 for CLIP)
        self.dtype = torch.float16
        self.config = SimpleNamespace(in_channels=cfg.in_channels)      # read by the reference wrapper (:524)
        self.device_name = "dry-run" if ops.DRY_RUN else _lib.device_name()   # raises unless a gfx950 is present
        self.mm_layout = motion_module_layout(cfg, height, width)
        # levels whose stream batch is small enough for the weight-streaming GEMM (wsgemm.hip): N * T tokens <= L2D_WSGEMM_MAX_M and
        # samples made of whole 32-token tiles.  Decides the PACKING of those levels' layers (and with it the plan's kernels); levels of
        # up to 1280 tokens take it by default, larger ones -- up to this bound -- per measured shape (ops.wsgemm_wanted)
        o = ops.overrides()
        self.ws_levels = [o.wsgemm and denoising_steps_num * (height >> l) * (width >> l) <= o.wsgemm_max_m
                          and ((height >> l) * (width >> l)) % 32 == 0 for l in range(cfg.num_levels)]
        if isinstance(state_dict, HipStreamingUNet):
            o = state_dict
            if (o.cfg, o.h, o.w, o.device) != (cfg, self.h, self.w, self.device):
                raise ValueError("shared packed weights need the same configuration, latent size and device")
            if (o.N, o.ws_levels) != (self.N, self.ws_levels):
                # the packing depends on the stream batch too (which levels take the weight-streaming form, the per-shape skip
                # list keyed by M = N T): forms chosen for another N would be missing / forced here (as _load_packed checks)
                raise ValueError(f"shared packed weights were packed for denoising_steps_num = {o.N} (weight-streaming levels "
                                 f"{o.ws_levels}), this instance has {self.N} ({self.ws_levels}): re-pack")
            self.W, self.temb_offsets, self.text_offsets = o.W, o.temb_offsets, o.text_offsets
            self._w_gen = o._w_gen           # (shared together with W: a blend through any sharer makes every sharer's conditioning stale)
            self.n_map_blocks, self.temb_total, self.text_total, self.text_kp = o.n_map_blocks, o.temb_total, o.text_total, o.text_kp
        elif isinstance(state_dict, (str, os.PathLike)):
            self._load_packed(state_dict)          # a file written by save_packed(): skips the packing pass
        elif isinstance(state_dict, PackedWeights):
            self._adopt_packed(state_dict.W, state_dict.meta, "packed weights")     # received from another rank
        else:
            self._pack_weights(state_dict)
            own_storage(self.W, state_dict)
        self._plans = {}
        self._graph = {}
        if not hasattr(self, "_w_gen"):
            self._w_gen = [0]                # generation of the contents of W: bumped by load_mix
        self._blender = None

    # ------------------------------------------------------------------ reference-compatible surface
    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def forward(self, *a, **k):
        return self(*a, **k)

    def set_info_for_attn(self, height: int, width: int, *a, **k):
        assert (height, width) == (self.h, self.w), "static shapes per instance (TensorRT precedent: models.py:289-291)"

    def prepare_cache(self, denoising_steps_num: int) -> List[torch.Tensor]:
        """Zero KV caches [N,2,h*w,L,C] fp16 in motion_module_idx order
        (reference unet_depth_streaming.py:283-302 + stream_motion_module.py:57-77)."""
        return [torch.zeros(denoising_steps_num, 2, hh * ww, self.cfg.window_size, c, dtype=torch.float16,
                            device=self.device) for (c, hh, ww, _l) in self.mm_layout]

    # ------------------------------------------------------------------ weights
    def _pack_weights(self, sd):
        """the packing pass (unet_pack.py): `W` and the scalars that describe it"""
        packed = pack_unet(sd, self.cfg, self.h, self.w, self.N, self.ws_levels, self.device)
        for k, v in packed._asdict().items():
            setattr(self, k, v)

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.W.values())

    # ------------------------------------------------------------------ packed-weight cache
    PACK_FORMAT = 4      # bump when _pack_weights changes layout (packed conv / GEGLU order, fused projections, ...)

    def save_packed(self, path) -> None:
        """Write the packed weights (what `_pack_weights` produced from the reference-keyed state dict: merged
        DreamBooth / LoRA weights, permuted, fused and padded for the kernels, PE tables pre-projected) as one
        safetensors file.  The analogue of the reference's TensorRT engine cache (wrapper.py:300-332, :505-560): a style
        switch that was seen before skips the conversion.  Packed weights depend on the weights, on the window length and on
        WHICH KERNEL serves each layer: the levels with few stream tokens (`ws_levels`: denoising steps x latent size) hold the
        weight-streaming forms, levels whose samples are not whole 32-token tiles the implicit-GEMM forms, and the L2D_WSGEMM*
        overrides move layers between kernels.  The file records all of that; `_load_packed` refuses a file packed for another layout
        with a "re-pack" error instead of failing on a missing tensor later."""
        from safetensors.torch import save_file
        save_file({k: v.detach().cpu().contiguous() for k, v in self.W.items()}, str(path), metadata=self._packed_meta())

    def _packed_meta(self) -> dict:
        import json
        return dict(format=str(self.PACK_FORMAT), abi=str(_lib.ABI_VERSION), window=str(self.cfg.window_size),
                    block_out_channels=json.dumps(list(self.cfg.block_out_channels)),
                    temb_offsets=json.dumps(self.temb_offsets), text_offsets=json.dumps(self.text_offsets),
                    n_map_blocks=str(self.n_map_blocks), layout=json.dumps(self._pack_layout()))

    def packed_state(self) -> "PackedWeights":
        """The packed weights of this instance as (tensors, metadata) -- what a packed-weight file holds, without the file."""
        return PackedWeights(self.W, self._packed_meta())

    def load_mix(self, sets, weights) -> None:
        """Overwrite the packed weights IN PLACE with sum_k weights[k] * sets[k] (each a `PackedWeights` of this configuration, stream
        shape and kernel layout), one launch on the current stream (style_bank.WeightBlender).  Plans and captured graphs keep
        their pointers and are not rebuilt; everything derived from weights at run time (time-embedding rows, text K / V^T) is
        recomputed before the next frame of EVERY instance that shares this W.  The sets must not be this instance's own W."""
        from .style_bank import WeightBlender
        sets, weights = list(sets), list(weights)
        own = self._packed_meta()
        for j, ps in enumerate(sets):
            if not isinstance(ps, PackedWeights):
                raise TypeError(f"load_mix: set {j} is {type(ps).__name__}, need PackedWeights (packed_state())")
            self._check_packed_meta(ps.meta, f"style set {j}")
            for k in ("temb_offsets", "text_offsets", "n_map_blocks"):
                if ps.meta.get(k) != own[k]:
                    raise ValueError(f"style set {j}: {k} = {ps.meta.get(k)}, this instance has {own[k]}: re-pack from the state dict")
            if ps.W is self.W:
                raise ValueError(f"load_mix: set {j} is this instance's own W (the destination): blend from a copy")
        if self._blender is None:
            self._blender = WeightBlender(self.W, self.device)
        self._blender.apply([ps.W for ps in sets], weights)
        self._w_gen[0] += 1

    def _cond_fresh(self, st) -> None:
        """the conditioning launches read W: stale after a blend through any instance that shares it"""
        if getattr(st, "w_gen", None) != self._w_gen[0]:
            st.cond_key, st.w_gen = None, self._w_gen[0]

    def _load_packed(self, path) -> None:
        import json

        from safetensors import safe_open
        with safe_open(str(path), framework="pt", device="cpu") as f:
            meta = f.metadata() or {}
            self._check_packed_meta(meta, path)
            # (a copy in every case: on the CPU -- dry-run plans of the test-suite -- get_tensor() returns a view into the file buffer
            #  whose address need not be 16-byte aligned, which the launch validation requires of every pointer)
            W = {k: (f.get_tensor(k).to(self.device) if torch.device(self.device).type != "cpu" else f.get_tensor(k).clone())
                 for k in f.keys()}
        self._adopt_packed(W, meta, path, checked=True)

    def _check_packed_meta(self, meta, path) -> None:
        import json
        if int(meta.get("format", -1)) != self.PACK_FORMAT or int(meta.get("abi", -1)) != _lib.ABI_VERSION:
            raise ValueError(f"{path}: packed-weight format {meta.get('format')} / ABI {meta.get('abi')} does not match "
                             f"this build ({self.PACK_FORMAT} / {_lib.ABI_VERSION}): re-pack from the state dict")
        if json.loads(meta.get("layout", "null")) != self._pack_layout():
            raise ValueError(f"{path}: packed for kernel layout {meta.get('layout')}, this instance needs {json.dumps(self._pack_layout())} "
                             "(latent size / denoising steps / L2D_WSGEMM* differ): re-pack from the state dict")
        if int(meta["window"]) != self.cfg.window_size or json.loads(meta["block_out_channels"]) != list(self.cfg.block_out_channels):
            raise ValueError(f"{path}: packed for window {meta['window']} / widths {meta['block_out_channels']}, "
                             f"this instance is window {self.cfg.window_size} / {list(self.cfg.block_out_channels)}")

    def _adopt_packed(self, W, meta, path, checked: bool = False) -> None:
        import json
        if not checked:
            self._check_packed_meta(meta, path)
        self.W = W
        self.temb_offsets = {k: int(v) for k, v in json.loads(meta["temb_offsets"]).items()}
        self.text_offsets = {k: int(v) for k, v in json.loads(meta["text_offsets"]).items()}
        self.n_map_blocks = int(meta["n_map_blocks"])
        self.temb_total = self.W["temb_all.w"].shape[0]
        self.text_total, self.text_kp = self.W["text_k.w"].shape

    def _pack_layout(self) -> dict:
        """what decides which packed form each layer has (besides the weights themselves)"""
        nl = self.cfg.num_levels
        o = ops.overrides()
        t = ops.wsgemm_table(o)
        return dict(ws_levels=[bool(v) for v in self.ws_levels],
                    old_levels=[((self.h >> l) * (self.w >> l)) % 32 != 0 for l in range(nl)],
                    ws_skip=sorted(t.get("skip", [])), ws_large=sorted(t.get("large", [])),
                    ws_tokens=[self.N * (self.h >> l) * (self.w >> l) if self.ws_levels[l] else 0 for l in range(nl)],
                    wsgemm=o.wsgemm, ws_max_m=o.wsgemm_max_m, ws_large_all=o.wsgemm_large_all,
                    # the fallback rules decide packed forms too (which layers take the weight-streaming form at token counts the tuner
                    # never saw; from how many blocks a level packs the chain kernel's weights)
                    rowchain_min_blocks=ops.ROWCHAIN_MIN_BLOCKS)

    @staticmethod
    def packed_cache_name(model_name: str, few_step_model_type: str, window_size: int, lora_dict: Optional[dict] = None,
                          height: int = 0, width: int = 0, denoising_steps_num: int = 0) -> str:
        """File stem for a packed-weight cache entry, in the spirit of the reference's engine prefix (wrapper.py:300-332).  Since
        round 4 the packed forms depend on the stream shape (which levels take the weight-streaming kernel), so the LATENT size
        and the number of denoising steps are part of the name like they are in the reference's prefix; the tiny-VAE is not."""
        stem = f"{model_name}--{few_step_model_type}--"
        for k, v in (lora_dict or {}).items():
            stem += f"{os.path.splitext(os.path.basename(str(k)))[0]}-{v}--"
        shape = f"{height}x{width}x{denoising_steps_num}--" if height and width and denoising_steps_num else ""
        return stem + shape + f"L{window_size}--l2dpack{HipStreamingUNet.PACK_FORMAT}"

    # ------------------------------------------------------------------ plan construction
    def _build_plan(self, mode: str, kv_cache: List[torch.Tensor]):
        """the static launch plan of one step, `mode` "stream" or "warmup" (unet_plan.py)"""
        return UNetPlan(self.cfg, self.W, self.h, self.w, self.N, self.F, self.device, temb_offsets=self.temb_offsets,
                        text_offsets=self.text_offsets, n_map_blocks=self.n_map_blocks, text_len=self.text_len,
                        tattn_variant=self.tattn_variant, mode=mode, kv_cache=kv_cache).build()

    def _plan(self, mode, kv_cache):
        st = self._plans.get(mode)
        if st is None:
            st = self._build_plan(mode, kv_cache)
            self._plans[mode] = st
        return st

    def _bind_caches(self, st, kv_cache, row: Optional[int] = None):
        """Re-point the temporal-attention ops at the caller's cache tensors (they normally never change:
        the pipeline owns one `kv_cache_list` for the stream's lifetime)."""
        changed = False
        for tag, idx in st.tattn_ops:
            c = kv_cache[idx]
            assert c.dtype == torch.float16 and c.is_contiguous(), "kv_cache must be contiguous fp16 [N,2,T,L,C]"
            ptr = c.data_ptr() if row is None else c.data_ptr() + row * c.stride(0) * 2
            op = st.pl[tag]
            if op.p[1] != ptr:
                op.p[1] = ptr
                changed = True
        if changed:
            st.pl._arr = None
            self._graph.pop(st.mode, None)

    def invalidate_text_cache(self):
        """Force the conditioning launches (time embedding, text K / V^T) to re-run on the next call: for callers that
        rewrite the plan's static `in_enc` / `in_t` buffers themselves (HipStreamStep.set_prompt)."""
        for st in self._plans.values():
            st.cond_key = None

    def _load_cond(self, st, timestep, encoder_hidden_states):
        """Conditioning inputs -> static buffers + the `cond_pl` launches, only when they changed.  "Changed" is decided
        on the host without a sync: the SAME tensor objects as last call (held here, so their storage cannot be recycled
        for other data) with unchanged in-place version counters.  The reference pipeline passes `self.prompt_embeds`
        (re-bound only by update_prompt) and one `sub_timesteps_tensor` for the whole stream; a caller that builds fresh
        tensors every call simply gets the launches every call."""
        cfg = self.cfg
        self._cond_fresh(st)
        key = (timestep, encoder_hidden_states, timestep._version, encoder_hidden_states._version)
        old = st.cond_key
        if (self.cond_cache and old is not None and len(old) == 4 and old[0] is key[0] and old[1] is key[1]
                and old[2:] == key[2:]):
            return
        st.in_t.copy_(timestep.reshape(-1)[:1] if st.Bt == 1 else timestep.reshape(-1).expand(st.Bt))
        st.in_enc[:, : st.text_len, : cfg.cross_attention_dim].copy_(encoder_hidden_states[: st.Bt])
        st.cond_pl.run()
        st.cond_key = key

    def _ensure_cond(self, st):
        """For callers that own the static inputs (HipStreamStep): run the conditioning launches if they are stale."""
        self._cond_fresh(st)
        if st.cond_key is None:
            st.cond_pl.run()
            st.cond_key = ("external",)

    def _run(self, st):
        if self.use_graph and st.warm:      # the first call runs directly: the launchers' one-time kernel-attribute /
            g = self._graph.get(st.mode)    # device queries are not allowed inside a stream capture
            if g is None:
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    g = _lib.Graph(st.pl, stream=int(side.cuda_stream))
                torch.cuda.current_stream().wait_stream(side)
                self._graph[st.mode] = g
            g.launch()
        else:
            st.pl.run()
            st.warm = True

    # ------------------------------------------------------------------ the boundary call
    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, temporal_attention_mask=None, depth_sample=None,
                 kv_cache=None, pe_idx=None, update_idx=None, return_dict: bool = True, **kwargs):
        N, cfg = self.N, self.cfg
        if tuple(sample.shape) != (N, cfg.in_channels, 1, self.h, self.w):
            raise ValueError(f"sample shape {tuple(sample.shape)} != static {(N, cfg.in_channels, 1, self.h, self.w)}")
        if kv_cache is None or len(kv_cache) != len(self.mm_layout):
            raise ValueError(f"kv_cache must be the list of {len(self.mm_layout)} caches from prepare_cache()")
        st = self._plan("stream", kv_cache)
        self._bind_caches(st, kv_cache)
        st.text_len_rt = encoder_hidden_states.shape[1]
        if st.text_len_rt != st.text_len:
            raise ValueError(f"text length {st.text_len_rt} != static {st.text_len}")
        st.in_sample.copy_(sample.reshape(N, cfg.in_channels, -1))
        st.in_depth.copy_(depth_sample.reshape(N, cfg.in_channels, -1))
        self._load_cond(st, timestep, encoder_hidden_states)
        st.in_bias.copy_(temporal_attention_mask)
        st.in_pe_idx.copy_(pe_idx)
        st.in_upd.copy_(update_idx)
        self._run(st)
        if self.fresh_output:
            out = st.out_sample.clone().view(N, cfg.out_channels, 1, self.h, self.w)
            return UNetOutput(out, kv_cache) if return_dict else (out, kv_cache)
        out = st.out_sample.view(N, cfg.out_channels, 1, self.h, self.w)    # a view of the plan's static output buffer (like
        if not return_dict:                                                  # the TensorRT engine's output binding): the next call overwrites it
            return (out, kv_cache)
        return UNetOutput(out, kv_cache)

    @torch.no_grad()
    def warmup(self, sample, timestep, encoder_hidden_states=None, depth_sample=None, kv_cache=None, row: int = 0,
               return_dict: bool = True, **kwargs):
        """Warm-up UNet pass over F frames that fills cache row `row` (slots 0..F-1) of every layer.
        sample/depth [1,4,F,h,w]; timestep [1]; encoder_hidden_states [1,77,D]; kv_cache = the FULL cache list
        (the reference passes `[cache[idx] for cache in kv_cache_list]`, pipeline :326)."""
        F_, cfg = self.F, self.cfg
        if tuple(sample.shape) != (1, cfg.in_channels, F_, self.h, self.w):
            raise ValueError(f"warm-up sample shape {tuple(sample.shape)} != {(1, cfg.in_channels, F_, self.h, self.w)}")
        st = self._plan("warmup", kv_cache)
        self._bind_caches(st, kv_cache, row=row)
        st.in_sample.copy_(sample[0].transpose(0, 1).reshape(F_, cfg.in_channels, -1))
        st.in_depth.copy_(depth_sample[0].transpose(0, 1).reshape(F_, cfg.in_channels, -1))
        self._load_cond(st, timestep, encoder_hidden_states)
        self._run(st)
        out = st.out_sample.view(F_, cfg.out_channels, self.h, self.w).transpose(0, 1).unsqueeze(0)
        if not return_dict:
            return (out,)
        return UNetOutput(out, kv_cache)

    # ------------------------------------------------------------------ introspection for bench / tests
    def plan_summary(self, mode="stream"):
        st = self._plans[mode]
        return dict(st.summary(), n_cond_ops=len(st.cond_pl), weight_bytes=self.weight_bytes())
