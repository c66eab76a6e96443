"""The UNet's packing pass: a reference-keyed `state_dict` -> `W`, the tensors the kernels read (3x3 taps-major, q|k fused, q|k|v
fused for the temporal layers, GEGLU value/gate interleaved, all time_emb_proj / all text K,V projections concatenated into single
GEMMs).  The packer decides WHICH KERNEL takes a layer and writes the decision as the key suffix: `.ww` / `.ww1` weight-streaming
(wsgemm.hip), `.rw` / `.rw1` token-row (rowgemm.hip), `.cw` cconv, `.chw` chain (rowchain.hip), `.w` / `.w1` implicit GEMM.  The
suffixes are the packed-file format (HipStreamingUNet.PACK_FORMAT); unet_plan.UNetPlan.form reads them back.
"""
import math
from typing import NamedTuple

import torch

from . import ops
from .config import UNetConfig, unet_blocks


def sinusoid_pe(max_len: int, dim: int, device) -> torch.Tensor:
    """reference positional_encoding.py:12-16"""
    pos = torch.arange(max_len, dtype=torch.float32, device=device).unsqueeze(1)
    div = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32, device=device) * (-math.log(10000.0) / dim))
    pe = torch.zeros(max_len, dim, device=device)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def own_storage(W: dict, state_dict) -> None:
    """Packed tensors that are the state dict's own tensors or views of them (a state dict already on the device in the packed
    dtype: `.to()`, `.contiguous()` and `reshape` copy nothing) are replaced by copies, in place in `W`.  `load_mix` overwrites
    the packed tensors; it must reach neither the caller's state dict nor another instance packed from the same one."""
    theirs = {v.untyped_storage().data_ptr() for v in state_dict.values() if torch.is_tensor(v) and v.numel()}
    for k, t in W.items():
        if torch.is_tensor(t) and t.numel() and t.untyped_storage().data_ptr() in theirs:
            W[k] = t.clone()


class PackedUNet(NamedTuple):
    """what the packing pass leaves on a HipStreamingUNet"""
    W: dict
    temb_offsets: dict      # resnet name -> first row of its time_emb_proj in "temb_all"
    text_offsets: dict      # spatial block name -> first row of its cross-attention K / V projection in "text_k" / "text_v"
    n_map_blocks: int
    temb_total: int
    text_total: int
    text_kp: int
    pe_tables: dict


def pack_unet(sd, cfg: UNetConfig, h: int, w: int, N: int, ws_levels, device) -> PackedUNet:
    """h, w: latent size; N: denoising steps (the stream batch); ws_levels: the levels whose layers take the weight-streaming GEMM"""
    return _Packer(sd, cfg, h, w, N, ws_levels, device).pack()


class _Packer:
    def __init__(self, sd, cfg, h, w, N, ws_levels, device):
        self.sd, self.cfg, self.h, self.w, self.N, self.ws_levels, self.dev = sd, cfg, h, w, N, ws_levels, device
        self.W, self.temb_offsets, self.text_offsets, self.pe_tables = {}, {}, {}, {}
        self.temb_w, self.temb_b, self.text_k, self.text_v = [], [], [], []

    def g(self, k):
        return self.sd[k].to(device=self.dev)

    def conv3(self, name):
        self.W[name + ".w"] = ops.pack_conv3x3(self.g(name + ".weight"))
        self.W[name + ".b"] = ops.f32(self.g(name + ".bias"))

    def norm(self, name):
        self.W[name + ".g"] = self.g(name + ".weight").to(torch.float16).contiguous()
        self.W[name + ".beta"] = self.g(name + ".bias").to(torch.float16).contiguous()

    def plain(self, name):
        """fp16 row-major weight + fp32 bias (the skinny GEMMs of the time embedding)"""
        self.W[name + ".w"] = self.g(name + ".weight").to(torch.float16).contiguous()
        self.W[name + ".b"] = ops.f32(self.g(name + ".bias"))

    def rg_ok(self, wname):
        n, k = self.sd[wname].shape[0], self.sd[wname][0].numel()
        return ops.rowgemm_ok(n, k)

    def ws_ok(self, wname, lvl, n_mul=1, epi=0, pro=0, ntr=0, taps=1):
        """the weight-streaming GEMM (wsgemm.hip) takes this layer: a level of few tokens, 32-row weight tiles, 64-column chunks,
        and the in-frame tuner did not find the round-3 kernel faster for the shape (ops.wsgemm_wanted); n_mul: q | k | v"""
        n, k = self.sd[wname].shape[0] * n_mul, self.sd[wname][0].numel()
        if lvl is None or not self.ws_levels[lvl] or n % 32 or (k // taps) % 64:
            return False
        M_ = self.N * (self.h >> lvl) * (self.w >> lvl)
        return ops.wsgemm_wanted(taps, M_, k, n, ntr, epi, pro)

    def lin(self, name, bias=True, norm=None, old=False, lvl=None, gnorm=False):
        """Linear layer `name`; `norm` = the LayerNorm (or, `gnorm`, GroupNorm) whose output feeds it.  At the few-token levels
        (`lvl` in ws_levels) the weight-streaming packing (wsgemm.hip: fragment order, a LayerNorm folded into weight,
        bias and column sums) -- except behind a GroupNorm, whose per-group scale cannot move to the accumulator side.
        Else token-row GEMM packing (rowgemm.hip: fragment order, the norm's affine folded into weight and bias) when the shape
        allows, else -- and with `old` in addition -- the implicit-GEMM packing with the norm applied by its own launch."""
        W, g, sd = self.W, self.g, self.sd
        fold = (g(name + ".weight"), g(name + ".bias") if bias else None, g(norm + ".weight") if norm else None, g(norm + ".bias") if norm else None)
        if not gnorm and self.ws_ok(name + ".weight", lvl, pro=(1 if norm else 0)):
            W[name + ".ww"], wb, wcs = ops.pack_wsgemm(*fold)
            if wb is not None:
                W[name + ".wb"] = wb
            if wcs is not None:
                W[name + ".wcs"] = wcs
            return
        # Row GEMM where it fuses a norm, and for the narrow levels (K <= 640).  A plain Linear at K = 1280 stays on the
        # implicit-GEMM kernel: with 32-token row tiles every block ingests its whole weight band (80 KB per 32-row tile), and
        # the probe (profiles/round3_b_rowgemm_block_phases_before.txt) shows those launches bound by ~30 B/clk of ingest per CU.
        rg = self.rg_ok(name + ".weight") and (norm is not None or sd[name + ".weight"][0].numel() <= ops.ROWGEMM_PLAIN_MAX_K)
        if rg:
            W[name + ".rw"], rb = ops.pack_rowgemm(*fold)
            if rb is not None:
                W[name + ".rb"] = rb
        if not rg or old:
            W[name + ".w"] = ops.pack_linear(fold[0])
            if bias:
                W[name + ".b"] = ops.f32(fold[1])

    def ff(self, name, norm, old=False, lvl=None):
        W, g, sd = self.W, self.g, self.sd
        pw, pb = name + ".net.0.proj.weight", name + ".net.0.proj.bias"
        fold = lambda: (g(pw), g(pb), g(norm + ".weight"), g(norm + ".bias"))
        rg = self.rg_ok(pw) and sd[pw].shape[0] % 64 == 0 and sd[pw][0].numel() <= ops.ROWGEMM_FF1_MAX_K
        if self.ws_ok(pw, lvl, epi=1, pro=1) and sd[pw].shape[0] % 64 == 0:
            W[name + ".ww1"], W[name + ".wb1"], W[name + ".wcs1"] = ops.pack_wsgemm(*fold(), geglu=True)
        elif rg:
            W[name + ".rw1"], W[name + ".rb1"] = ops.pack_rowgemm(*fold(), geglu=True)
            if sd[pw][0].numel() == ops.ROWCHAIN_C:
                # the token-resident block tail (rowchain.hip) streams FF2 in the row GEMM's fragment order too (K = 4 C).  Its own
                # keys (".chw" / ".chb"): the plan picks the row GEMM for a layer by the presence of ".rw", and a plain K = 1280
                # Linear must stay on the implicit-GEMM kernel wherever the chain does not run (round-5 advisor finding)
                W[name + ".net.2.chw"], W[name + ".net.2.chb"] = ops.pack_rowgemm(g(name + ".net.2.weight"), g(name + ".net.2.bias"))
        if (name + ".ww1") not in W and (not rg or old):
            W[name + ".w1"], W[name + ".b1"] = ops.pack_geglu(g(pw), g(pb))
        self.lin(name + ".net.2", old=old, lvl=lvl)

    def conv3cc(self, name, lvl_out, ups=0) -> bool:
        """3x3 stride-1 conv whose OUTPUT lives at level `lvl_out`: the patch-resident / register-streamed packing of cconv.hip
        where the plan wants that kernel (ops.cconv_wanted: measured per shape class); the K-group count of the packing is the
        stream plan's (ops.cconv_schedule on the stream batch), the warm-up plan re-uses it"""
        cw = self.sd[name + ".weight"]
        Ho, Wo = self.h >> lvl_out, self.w >> lvl_out
        if cw.shape[1] % 64 or not ops.cconv_wanted(self.N, Ho, Wo, cw.shape[1], cw.shape[0], ups):
            return False
        kg = ops.cconv_schedule(self.N, Ho, Wo, cw.shape[0], cw.shape[1])[1]
        self.W[name + ".cw"] = ops.pack_cconv(self.g(name + ".weight"), kg)
        self.W[name + ".b"] = ops.f32(self.g(name + ".bias"))
        return True

    def conv3ws(self, name, lvl):
        """resnet 3x3 conv: cconv packing where that kernel is wanted, weight-streaming packing at the few-token levels, else the
        implicit-GEMM / patch-conv packing"""
        cw = self.sd[name + ".weight"]
        if self.conv3cc(name, lvl):
            return
        # (the kernel's loader walks 8 NL pixels per DMA instruction with at most two row wraps: W >= 8, wsgemm.hip; narrower
        # levels -- tall / narrow latents such as 64 x 32 -- stay on the implicit-GEMM / patch kernels like in round 3)
        if (self.w >> lvl) >= 8 and cw.shape[0] % 32 == 0 and cw.shape[1] % 64 == 0 and self.ws_ok(name + ".weight", lvl, taps=9):
            self.W[name + ".ww"] = ops.pack_wsgemm_conv3x3(self.g(name + ".weight"))
            self.W[name + ".b"] = ops.f32(self.g(name + ".bias"))
        else:
            self.conv3(name)

    def concat_parts_ok(self, name, c1):
        """wsgemm takes whole 64-channel chunks from EACH input of a two-pointer concat (up blocks: hidden | skip); c1: the
        channels of the first input (a resnet with one input: all of them)"""
        return c1 % 64 == 0 and (self.sd[name + ".conv_shortcut.weight"].shape[1] - c1) % 64 == 0

    def resnet(self, name, lvl, c1):
        self.norm(name + ".norm1"); self.conv3ws(name + ".conv1", lvl); self.norm(name + ".norm2"); self.conv3ws(name + ".conv2", lvl)
        sc = name + ".conv_shortcut"
        if (sc + ".weight") in self.sd:                   # (two-input concat GEMM)
            if self.ws_ok(sc + ".weight", lvl) and self.concat_parts_ok(name, c1):
                self.lin(sc, lvl=lvl)
            else:
                self.W[sc + ".w"] = ops.pack_linear(self.g(sc + ".weight"))
                self.W[sc + ".b"] = ops.f32(self.g(sc + ".bias"))
        self.temb_offsets[name] = sum(t.shape[0] for t in self.temb_w)
        self.temb_w.append(self.g(name + ".time_emb_proj.weight").to(torch.float16))
        self.temb_b.append(self.g(name + ".time_emb_proj.bias").float())

    def spatial(self, name, lvl):
        # the mid block sits at the lowest resolution, where T = h w / 64 need not be a multiple of the row GEMM's 32-token
        # tile (its transposed V output and GroupNorm prologue need that): it keeps the implicit-GEMM packing as well
        # (likewise any level of THIS instance where T % 32 != 0: small test latents; a packed-weight file written there
        # holds both forms, one written at an SD resolution holds the second form for the mid block only)
        W, g, lin = self.W, self.g, self.lin
        Tl = (self.h >> lvl) * (self.w >> lvl)
        old = name.startswith("mid_block") or Tl % 32 != 0
        b = name + ".transformer_blocks.0"
        self.norm(name + ".norm"); lin(name + ".proj_in", norm=name + ".norm", old=old, gnorm=True); lin(name + ".proj_out", old=old, lvl=lvl)
        for n in ("norm1", "norm2", "norm3"):
            self.norm(b + "." + n)
        wq, wk, wv = (g(b + f".attn1.to_{c}.weight") for c in "qkv")
        fold = (torch.cat([wq, wk, wv], 0), None, g(b + ".norm1.weight"), g(b + ".norm1.bias"))
        rg = self.rg_ok(b + ".attn1.to_q.weight")
        if Tl % 128 == 0 and self.ws_ok(b + ".attn1.to_q.weight", lvl, n_mul=3, pro=1, ntr=wq.shape[0]):
            # q | k | v in one weight-streaming launch behind norm1 (V leaves transposed: a sample is whole 128-token tiles)
            W[b + ".attn1.qkv.ww"], W[b + ".attn1.qkv.wb"], W[b + ".attn1.qkv.wcs"] = ops.pack_wsgemm(*fold)
        elif rg:
            # q | k | v in one launch behind norm1 (V leaves transposed): rowgemm.hip
            W[b + ".attn1.qkv.rw"], W[b + ".attn1.qkv.rb"] = ops.pack_rowgemm(*fold)
        if (b + ".attn1.qkv.ww") not in W and (not rg or old):
            W[b + ".attn1.qk"] = ops.pack_linear(torch.cat([wq, wk], 0))
            W[b + ".attn1.v"] = ops.pack_linear(wv)
        lin(b + ".attn1.to_out.0", old=old, lvl=lvl)
        lin(b + ".attn2.to_q", bias=False, norm=b + ".norm2", old=old, lvl=lvl)
        self.text_offsets[name] = sum(t.shape[0] for t in self.text_k)
        self.text_k.append(g(b + ".attn2.to_k.weight").to(torch.float16))
        self.text_v.append(g(b + ".attn2.to_v.weight").to(torch.float16))
        lin(b + ".attn2.to_out.0", old=old, lvl=lvl)
        self.ff(b + ".ff", b + ".norm3", old=old, lvl=lvl)

    def motion(self, name, lvl, C):
        W, g, lin = self.W, self.g, self.lin
        t = name + ".temporal_transformer"
        self.norm(t + ".norm"); lin(t + ".proj_in", norm=t + ".norm", gnorm=True); lin(t + ".proj_out", lvl=lvl)
        b = t + ".transformer_blocks.0"
        L = self.cfg.window_size
        if C not in self.pe_tables:
            self.pe_tables[C] = sinusoid_pe(max(self.cfg.temporal_max_len, L), C, self.dev)
        pe = self.pe_tables[C][:L]
        for j in range(2):
            a = b + f".attention_blocks.{j}"
            wq, wk, wv = g(a + ".to_q.weight"), g(a + ".to_k.weight"), g(a + ".to_v.weight")
            fold = (torch.cat([wq, wk, wv], 0), None, g(b + f".norms.{j}.weight"), g(b + f".norms.{j}.bias"))
            if self.ws_ok(a + ".to_q.weight", lvl, n_mul=3, pro=1):
                W[a + ".qkv.ww"], W[a + ".qkv.wb"], W[a + ".qkv.wcs"] = ops.pack_wsgemm(*fold)
            elif self.rg_ok(a + ".to_q.weight"):
                W[a + ".qkv.rw"], W[a + ".qkv.rb"] = ops.pack_rowgemm(*fold)
            else:
                W[a + ".qkv"] = ops.pack_linear(fold[0])
            # pre-projected positional encodings (reference prepare_pe_buffer, stream_motion_module.py:79-97)
            for nm, w_ in (("q_pe", wq), ("k_pe", wk), ("v_pe", wv)):
                W[a + "." + nm] = (pe @ w_.float().t()).to(torch.float16).contiguous()
            lin(a + ".to_out.0", lvl=lvl)
            self.norm(b + f".norms.{j}")
        self.norm(b + ".ff_norm")
        self.ff(b + ".ff", b + ".ff_norm", lvl=lvl)

    def pack(self) -> PackedUNet:
        W, sd = self.W, self.sd
        self.conv3("conv_in")
        self.conv3("flow_conv_in.conv_in")
        n_map_blocks = 0
        while f"flow_conv_in.blocks.{n_map_blocks}.weight" in sd:
            self.conv3(f"flow_conv_in.blocks.{n_map_blocks}")
            n_map_blocks += 1
        self.conv3("flow_conv_in.conv_out")
        self.plain("time_embedding.linear_1"); self.plain("time_embedding.linear_2")
        c = self.cfg.block_out_channels[0]                # channels that enter the block
        for blk in unet_blocks(self.cfg):
            if blk.kind == "resnet":
                self.resnet(blk.name, blk.level, c)
            elif blk.kind == "spatial":
                self.spatial(blk.name, blk.level)
            elif blk.kind == "motion":
                self.motion(blk.name, blk.level, blk.channels)
            elif blk.kind == "down" or not self.conv3cc(blk.name, blk.level - 1, ups=1):       # (up-sampler output: one level up)
                self.conv3(blk.name)
            c = blk.channels
        self.norm("conv_norm_out"); self.conv3("conv_out")
        W["temb_all.w"] = torch.cat(self.temb_w, 0).contiguous()          # [sum Cout, 4*c0]
        W["temb_all.b"] = torch.cat(self.temb_b, 0).contiguous()
        W["text_k.w"] = ops.pack_linear(torch.cat(self.text_k, 0))        # [sum C, Kp(text)]
        W["text_v.w"] = ops.pack_linear(torch.cat(self.text_v, 0))
        return PackedUNet(W, self.temb_offsets, self.text_offsets, n_map_blocks, W["temb_all.w"].shape[0], *W["text_k.w"].shape, self.pe_tables)
