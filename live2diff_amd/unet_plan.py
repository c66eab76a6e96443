"""The UNet's static launch plan: `UNetPlan(...).build()` walks the topology once (config.unet_blocks) and emits the `l2d_op` records
of one step -- stream (batch = denoising steps) or warm-up (batch = frames) -- on the shared PlanBuilder.  The object is also the
plan's state: static input / output buffers, the conditioning launches (`cond_pl`) and what the runtime patches per call.

Which kernel takes a layer was decided by the packer (unet_pack.py) and is read back in ONE place, `form`.  The order in which ops
are appended and arena buffers are taken and given back is part of the plan (tests/test_plan_fingerprints.py).
"""
from typing import List, Optional, Tuple

import torch

from . import _lib, ops
from .config import UNetConfig, unet_blocks
from .ops import round_up
from .plan import Act, PlanBuilder

TEXT_PAD = 80   # 77 CLIP tokens padded to a multiple of 4 (igemm stores 4 channels per lane)
LN_EPS = 1e-5   # nn.LayerNorm default, as ops.layernorm


def _res(a: Optional[Act]) -> dict:
    """the residual operand of a GEMM / conv launch"""
    return dict(res=a.buf, ldr=a.C) if a is not None else dict(res=None, ldr=0)


def _x2(a: Optional[Act]) -> dict:
    """the second input of a two-pointer concat (up blocks: hidden | skip)"""
    return dict(x2=a.buf, C2=a.C, ldx2=a.C) if a is not None else dict(x2=None, C2=0, ldx2=0)


class UNetPlan(PlanBuilder):
    def __init__(self, cfg: UNetConfig, W: dict, h: int, w: int, N: int, F: int, device, *, temb_offsets: dict, text_offsets: dict,
                 n_map_blocks: int, text_len: int, tattn_variant: int, mode: str, kv_cache: List[torch.Tensor]):
        """W, temb_offsets, text_offsets, n_map_blocks: the packing pass's (unet_pack.PackedUNet); h, w: latent size; N / F: denoising
        steps / warm-up frames -- the batch axis of the "stream" / "warmup" `mode`; kv_cache: prepare_cache()'s list."""
        B = N if mode == "stream" else F                    # frames processed as the batch axis
        super().__init__(device, B, sk_counters=1 << 20, gn_layers=96, G=cfg.norm_num_groups)
        self.cfg, self.W, self.h, self.w, self.N, self.mode, self.kv_cache = cfg, W, h, w, N, mode, kv_cache
        self.temb_offsets, self.text_offsets, self.n_map_blocks = temb_offsets, text_offsets, n_map_blocks
        self.text_len, self.tattn_variant = text_len, tattn_variant
        self.temb_total, (self.text_total, self.text_kp) = W["temb_all.w"].shape[0], W["text_k.w"].shape
        Bt = self.Bt = N if mode == "stream" else 1         # rows of timestep / text inputs
        # `cond_pl`: the launches that depend on (timestep, text) only -- time-embedding MLP + every resnet's
        # time_emb_proj, and the K / V^T text projections of all 16 cross-attention layers (frame-invariant).
        # They run when the conditioning changes (first frame, update_prompt, a new warm-up row), not every frame.
        # `pl` starts with the zeroing of the GroupNorm statistics accumulators, once per frame.
        self.cond_pl, self.cond_key, self.warm = _lib.OpList(), None, False
        self.tattn_ops: List[Tuple[int, int]] = []          # (tag in `pl`, index into kv_cache) of every temporal attention
        self.ident = {}                                     # channels -> (ones, zeros): the affine part of a normalise-only GroupNorm
        z = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype, device=device)
        # ---- static inputs / outputs, and what the conditioning launches leave for the frame's
        self.in_sample, self.in_depth = z(B, cfg.in_channels, h * w), z(B, cfg.in_channels, h * w)
        self.in_t = z(Bt, dtype=torch.int64)
        self.in_enc = z(Bt, TEXT_PAD, self.text_kp)
        if mode == "stream":
            L = cfg.window_size
            self.in_bias, self.in_pe_idx, self.in_upd = z(B, L), z(B, L, dtype=torch.int64), z(B, dtype=torch.int64)
        self.out_sample = z(B, cfg.out_channels, h * w)
        self.temb_all = z(Bt, self.temb_total, dtype=torch.float32)
        self.text_k, self.text_vt = z(Bt * TEXT_PAD, self.text_total), z(Bt, self.text_total, TEXT_PAD)

    # ------------------------------------------------------------------ which kernel takes a layer
    def form(self, name: str, T: Optional[int] = None, sfx: str = "") -> str:
        """The packed form the plan uses for layer `name`: "cconv" (.cw), "ws" (weight-streaming, .ww: exists only at the
        weight-streaming levels), "row" (token-row, .rw: only where the row GEMM takes the shape) or "igemm".  sfx: "1" for the
        first layer of a feed-forward (.ww1 / .rw1 / .w1).  T: tokens per sample, given by the spatial blocks, whose row-GEMM
        launches (GroupNorm prologue, transposed V) need samples of whole 32-token tiles and which hold the implicit-GEMM form
        as well where that fails (mid block, small latents)."""
        if (name + ".cw") in self.W:
            return "cconv"
        if (name + ".ww" + sfx) in self.W:
            return "ws"
        if (name + ".rw" + sfx) in self.W and (T is None or T % 32 == 0):
            return "row"
        return "igemm"

    def temb_rows(self, off: Optional[int], T: int) -> dict:
        """launch arguments that add a resnet's time_emb_proj (columns from `off` of the conditioning GEMM's output) per sample"""
        if off is None:
            return {}
        return dict(rowbias=self.temb_all[:, off:], ldrb=self.temb_total, rows_per_bias=(T if self.mode == "stream" else self.B * T))

    # ------------------------------------------------------------------ single launches
    def linear_raw(self, xbuf, M, K, ldx, wt, outbuf, ldo, **kw):
        return self.gemm(xbuf, wt, outbuf, M=M, Nout=wt.shape[0], C1=K, ldx1=ldx, CinP=wt.shape[1], ldo=ldo, **kw)

    def rowlin(self, xbuf, M, K, wkey, bkey, outbuf, ldo, **kw):
        """one token-row GEMM launch (rowgemm.hip) on weights packed by ops.pack_rowgemm"""
        wt = self.W[wkey]
        kw.setdefault("T", M // self.B)          # tokens per sample: 64-token tiles only when a sample is a whole number of them
        return self.add(ops.rowgemm(xbuf, wt, outbuf, M=M, K=K, Nout=wt.numel() // K, ldx=K, ldo=ldo, bias=self.W.get(bkey), **kw))

    def wslin(self, xbuf, M, C1, wkey, outbuf, ldo, *, T, C2=0, epi=0, pro=0, taps=1, ntr=0, **kw):
        """one weight-streaming GEMM launch (wsgemm.hip) on weights packed by ops.pack_wsgemm / pack_wsgemm_conv3x3"""
        wt = self.W[wkey]
        Ktot = taps * (C1 + C2)
        nout = wt.numel() // Ktot
        sched = ops.wsgemm_schedule(M, Ktot, nout, ntr, epi, pro, taps)
        return self.wsgemm(xbuf, wt, outbuf, M=M, Nout=nout, C1=C1, ldx1=C1, ldo=ldo, C2=C2, taps=taps, epi=epi, pro=pro, eps=LN_EPS, T=T,
                           ntr=ntr, sched=sched, **kw)

    def layernorm(self, x: Act, name) -> Act:
        out = self.act(x.C, x.H, x.W)
        self.add(ops.layernorm(x.buf, self.W[name + ".g"], self.W[name + ".beta"], out.buf, rows=self.B * x.H * x.W, C=x.C, ldx=x.C, ldo=x.C))
        return out

    def ident_affine(self, C):
        if C not in self.ident:
            self.ident[C] = (torch.ones(C, dtype=torch.float16, device=self.device), torch.zeros(C, dtype=torch.float16, device=self.device))
        return self.ident[C]

    def gn_stats_target(self, x: Act, x2: Optional[Act], T, cpg):
        """Ask the producers of x (and x2) to accumulate this GroupNorm's statistics; the accumulator pointer or None"""
        return self.gn_acc_for([(x.producer, 0)] + ([(x2.producer, x.C)] if x2 is not None else []), T=T, cpg=cpg)

    def gn(self, x: Act, name, eps, silu, x2: Optional[Act] = None, affine: bool = True) -> Act:
        """affine=False: normalise only (gamma = 1, beta = 0): the consumer's packed weights carry the affine part."""
        T, cat = x.H * x.W, _x2(x2)
        C = x.C + cat["C2"]
        out = self.act(C, x.H, x.W)
        gam, bet = (self.W[name + ".g"], self.W[name + ".beta"]) if affine else self.ident_affine(C)
        self.groupnorm(x.buf, gam, bet, out.buf, T=T, C1=x.C, eps=eps, act=silu, acc_ptr=self.gn_stats_target(x, x2, T, C // self.G),
                       x2=cat["x2"], C2=cat["C2"])
        return out

    def conv3(self, x: Act, name, stride=1, ups=0, epi=0, res: Optional[Act] = None, temb: Optional[int] = None) -> Act:
        """3x3 conv (+ bias, + the time-embedding rows from column `temb`, + res) by the kernel its packed form names"""
        W, B, form = self.W, self.B, self.form(name)
        Ho, Wo = (x.H << ups, x.W << ups) if stride == 1 else ((x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1)
        cout = W[name + ".b"].numel()
        out = self.act(cout, Ho, Wo)
        kw = dict(bias=W[name + ".b"], **_res(res), **self.temb_rows(temb, Ho * Wo))
        if form == "cconv":
            # patch-resident activations + register-streamed weights (cconv.hip): resnet convs of the wide levels, up-samplers
            assert stride == 1 and epi == 0
            kg = ops.cconv_schedule(self.N, Ho, Wo, cout, x.C)[1]          # (the packing's: decided on the stream batch)
            out.producer = self.cconv(x.buf, W[name + ".cw"], out.buf, B=B, H=Ho, W=Wo, C1=x.C, ldx1=x.C, Nout=cout, ldo=cout, KG=kg, ups=ups,
                                      sched=ops.cconv_schedule(B, Ho, Wo, cout, x.C, KG=kg), **kw)
            return out
        if form == "ws":
            # resnet conv at a few-token level: weight-streaming GEMM over (tap, channel chunk) stages (wsgemm.hip)
            assert stride == 1 and not ups and epi == 0
            out.producer = self.wslin(x.buf, B * x.H * x.W, x.C, name + ".ww", out.buf, cout, T=x.H * x.W, taps=9, B=B, H=x.H, W=x.W, **kw)
            return out
        wt = W[name + ".w"]
        cinp = wt.shape[1] // 9
        patch = ops.pconv_patch(B, x.H, x.W, cout, x.C) if (stride == 1 and not ups and epi == 0 and cinp == x.C) else None
        if patch is not None:
            # resnet convs at the resolutions where a CU's ingest, not the matrix cores, bounds the implicit-GEMM kernel:
            # activation patch resident in LDS, fetched once per 64-channel chunk instead of once per tap (pconv.hip)
            out.producer = self.add(ops.pconv(x.buf, wt, out.buf, B=B, H=x.H, W=x.W, C1=x.C, ldx1=x.C, CinP=cinp, Nout=cout, ldo=cout,
                                              patch=patch, **kw))
            return out
        out.producer = self.gemm(x.buf, wt, out.buf, M=B * Ho * Wo, Nout=cout, C1=x.C, ldx1=x.C, CinP=cinp, ldo=cout, taps=9, B=B,
                                 Hin=x.H, Win=x.W, Hout=Ho, Wout=Wo, stride=stride, ups=ups, epi=epi, **kw)
        return out

    def linear(self, x: Act, name, res: Optional[Act] = None, x2: Optional[Act] = None, form: Optional[str] = None, **pro) -> Act:
        """Linear layer `name` (+ res) of x | x2 into a new activation.  pro: pro / eps / T / G / gn_acc_ptr of a fused norm prologue
        (row GEMM only)"""
        W, M, cat = self.W, self.B * x.H * x.W, _x2(x2)
        form = form or self.form(name)
        assert not pro or form == "row"
        if form == "ws":
            out = self.act(W[name + ".ww"].numel() // (x.C + cat["C2"]), x.H, x.W)
            out.producer = self.wslin(x.buf, M, x.C, name + ".ww", out.buf, out.C, T=x.H * x.W, bias=W.get(name + ".wb"), **_res(res), **cat)
        elif form == "row":
            assert x2 is None
            out = self.act(W[name + ".rw"].numel() // x.C, x.H, x.W)
            out.producer = self.rowlin(x.buf, M, x.C, name + ".rw", name + ".rb", out.buf, out.C, **_res(res), **pro)
        else:
            wt = W[name + ".w"]
            out = self.act(wt.shape[0], x.H, x.W)
            out.producer = self.linear_raw(x.buf, M, x.C, x.C, wt, out.buf, out.C, bias=W[name + ".b"], **_res(res), **cat)
        return out

    # ------------------------------------------------------------------ norm -> layer
    def gn_linear(self, x: Act, nname, eps, lname, T: Optional[int] = None) -> Act:
        """GroupNorm -> Linear (T: as in `form`).  Row GEMM path: the normalisation is the GEMM's prologue (statistics from x's
        producers), the affine part lives in the packed weights; if the statistics cannot come from the producers or a sample is
        not a whole number of 32-token tiles, a normalise-only GroupNorm launch runs in front."""
        form, Tx = self.form(lname, T), x.H * x.W
        acc_ptr = self.gn_stats_target(x, None, Tx, x.C // self.G) if form == "row" and Tx % 32 == 0 else None
        if acc_ptr is not None:
            return self.linear(x, lname, pro=2, eps=eps, T=Tx, G=self.G, gn_acc_ptr=acc_ptr)
        hn = self.gn(x, nname, eps, False, affine=(form != "row"))
        y = self.linear(hn, lname, form=form)
        self.free(hn)
        return y

    def ln_linear(self, x: Act, nname, lname, out: Act, *, T: Optional[int] = None, sfx="", epi=0, out_t=None, ntr=0, ldt=0,
                  st=0) -> Tuple[Act, Optional[Act]]:
        """LayerNorm `nname` -> Linear `lname` into `out` (out.C = its row pitch), by the form the layer has (`form`): one
        weight-streaming or token-row launch with the norm as its prologue, or a LayerNorm launch + implicit GEMM.  out_t / ntr /
        ldt / st: the last `ntr` output channels leave transposed (V^T[sample][channel][ldt]).  Returns (out, the LayerNorm's
        activation for the caller to free -- None where no launch of its own ran).  (The implicit-GEMM path gives `out` back and
        takes it again behind the LayerNorm's buffer: what the cross-attention query did, and no change for the others.)"""
        W, M, C, tr = self.W, self.B * x.H * x.W, x.C, dict(out_t=out_t, ntr=ntr, ldt=ldt, st=st)
        form = self.form(lname, T, sfx)
        if form == "ws":
            self.wslin(x.buf, M, C, lname + ".ww" + sfx, out.buf, out.C, T=x.H * x.W, bias=W.get(lname + ".wb" + sfx),
                       colsum=W[lname + ".wcs" + sfx], epi=epi, pro=1, **tr)
            return out, None
        if form == "row":
            self.rowlin(x.buf, M, C, lname + ".rw" + sfx, lname + ".rb" + sfx, out.buf, out.C, pro=1, eps=LN_EPS, epi=epi, **tr)
            return out, None
        self.free(out)
        n = self.layernorm(x, nname)
        out = self.act(out.C, out.H, out.W)
        if out_t is None:
            wt = W[lname + ".w" + sfx] if (lname + ".w" + sfx) in W else W[lname]          # (the temporal q | k | v: no suffix)
            self.linear_raw(n.buf, M, C, C, wt, out.buf, out.C, bias=W.get(lname + ".b" + sfx), epi=epi)
        else:
            stem, Tx = lname[:-len("qkv")], x.H * x.W
            self.linear_raw(n.buf, M, C, C, W[stem + "qk"], out.buf, out.C)
            # V^T[b] = Wv . n[b]^T : the same GEMM with operand roles swapped (tokens act as "channels")
            wv = W[stem + "v"]
            self.gemm(wv, n.buf, out_t, M=C, Nout=Tx, C1=C, ldx1=wv.shape[1], CinP=C, ldo=ldt, batch=self.B, sx1=0, sw=Tx * C, so=st)
        return out, n

    def geglu_ff(self, x: Act, nname, name, T: Optional[int] = None) -> Act:
        """x + FF2(GEGLU(FF1(LayerNorm(x))))"""
        hid, n = self.ln_linear(x, nname, name, self.act(4 * x.C, x.H, x.W), T=T, sfx="1", epi=1)
        out = self.linear(hid, name + ".net.2", res=x)
        self.free(hid); self.free(n)
        return out

    # ------------------------------------------------------------------ token-resident segments (rowchain.hip)
    def block_tail(self, ao: Act, res1: Act, res2: Act, to_out, ff, proj_out) -> Optional[Act]:
        """attention output projection + residual -> LayerNorm -> GEGLU -> FF2 + residual -> proj_out + block residual as ONE
        token-resident launch (rowchain.hip) where the level's M / 32 blocks fill the chip (C = 320); None = not here."""
        W, T, C = self.W, ao.H * ao.W, ao.C
        keys = (to_out + ".rw", to_out + ".rb", ff + ".rw1", ff + ".rb1", ff + ".net.2.chw", ff + ".net.2.chb", proj_out + ".rw", proj_out + ".rb")
        if not (ops.rowchain_ok(self.B * T, C, T) and all(k in W for k in keys)):
            return None
        out = self.act(C, ao.H, ao.W)
        out.producer = self.add(ops.rowchain(ao.buf, res1.buf, res2.buf, out.buf, M=self.B * T, C=C, w_out=W[keys[0]], b_out=W[keys[1]],
                                             w_ff1=W[keys[2]], b_ff1=W[keys[3]], w_ff2=W[keys[4]], b_ff2=W[keys[5]], w_po=W[keys[6]],
                                             b_po=W[keys[7]], eps=LN_EPS))
        return out

    def block_head(self, x: Act, a_name, b_name, passes, *, res: Optional[Act] = None, gn_of: Optional[Act] = None, vt: bool = False):
        """Two dependent layers as one token-resident launch (rowchain.hip head segment): h = A(x) (+ res) -- or A(GroupNorm(x)) with
        the statistics from x's producers -- stored as the residual stream, then B(LayerNorm(h)) -> out, `passes` x C columns
        (q | k | v, or the cross-attention's query; `vt`: q | k, and V leaves transposed into a buffer of its own).  Returns
        (h, out, V^T), all allocated here -- or (None, None, None), with nothing allocated or attached, when the segment does not
        run here: the caller emits the two launches."""
        W, T, C, G = self.W, x.H * x.W, x.C, self.G
        keys = (a_name + ".rw", a_name + ".rb", b_name + ".rw")
        if not (ops.rowchain_ok(self.B * T, C, T) and all(k in W for k in keys)):
            return None, None, None
        acc_ptr = self.gn_stats_target(gn_of, None, T, C // G) if gn_of is not None else None
        if gn_of is not None and acc_ptr is None:
            return None, None, None
        out, out_t, tr = self.act((passes - vt) * C, x.H, x.W), None, {}
        if vt:
            ldvt = round_up(T, 8)
            out_t = self.arena.alloc(self.B * C * ldvt)
            tr = dict(out_t=out_t, ldt=ldvt, st=C * ldvt, ldo=out.C)
        h = self.act(C, x.H, x.W)
        self.add(ops.rowchain_head(x.buf, h.buf, out.buf, M=self.B * T, C=C, wA=W[keys[0]], bA=W[keys[1]], wB=W[keys[2]],
                                   bB=W.get(b_name + ".rb"), passes=passes, resA=(res.buf if res is not None else None), gn_acc_ptr=acc_ptr,
                                   T=T, G=G, eps_gn=self.cfg.transformer_norm_eps, eps_ln=LN_EPS, **tr))
        return h, out, out_t

    # ------------------------------------------------------------------ blocks
    def gn_conv3(self, x: Act, x2: Optional[Act], nname, cname, **kw) -> Act:
        """conv3(silu(GroupNorm(x | x2))) (reference resnet.py:233-234, 249-250): GroupNorm launch + conv.  (The cconv launch can
        normalise its patch itself, ops.cconv gn_acc_ptr; in the frame that lost: profiles/round6_f_cconv_gn_fused_ab.txt.)"""
        hn = self.gn(x, nname, self.cfg.norm_eps, True, x2=x2)
        out = self.conv3(hn, cname, **kw)
        self.free(hn)
        return out

    def resnet(self, x: Act, name, skip: Optional[Act] = None) -> Act:
        h1 = self.gn_conv3(x, skip, name + ".norm1", name + ".conv1", temb=self.temb_offsets[name])
        sc = name + ".conv_shortcut"
        if (sc + ".w") in self.W or (sc + ".ww") in self.W:
            res = self.linear(x, sc, x2=skip)
        else:
            assert skip is None
            res = None
        out = self.gn_conv3(h1, None, name + ".norm2", name + ".conv2", res=(res or x))
        self.free(res); self.free(h1)
        return out

    def spatial(self, x: Act, name) -> Act:
        cfg, W, B = self.cfg, self.W, self.B
        T, C, HW = x.H * x.W, x.C, (x.H, x.W)
        b = name + ".transformer_blocks.0"
        if self.form(name + ".proj_in", T) == "igemm" and (name + ".proj_in.w") not in W:
            raise ValueError(f"{name}: T = {T} tokens per sample is no multiple of 32 at this level and the packed weights "
                             "lack the implicit-GEMM form of this block (packed-weight file written at another "
                             "resolution): re-pack from the state dict at this resolution")
        attn = dict(B=B, H=cfg.num_heads, d=C // cfg.num_heads, Tq=T, ldo=C, so=T * C)
        # --- proj_in behind the block's GroupNorm, norm1 -> q | k | V^T: one launch where the head segment runs
        ldvt = round_up(T, 8)
        y, qk, vt = self.block_head(x, name + ".proj_in", b + ".attn1.qkv", 3, gn_of=x, vt=True)
        if y is None:
            y = self.gn_linear(x, name + ".norm", cfg.transformer_norm_eps, name + ".proj_in", T=T)
            qk, vt = self.act(2 * C, *HW), self.arena.alloc(B * C * ldvt)
            qk, n1 = self.ln_linear(y, b + ".norm1", b + ".attn1.qkv", qk, T=T, out_t=vt, ntr=C, ldt=ldvt, st=C * ldvt)
            self.free(n1)
        # --- self attention
        ao = self.act(C, *HW)
        self.add(ops.flash_attn(qk.buf, qk.buf, vt, ao.buf, Tk=T, ldq=2 * C, ldk=2 * C, ldvt=ldvt, sq=T * 2 * C, sk=T * 2 * C, svt=C * ldvt,
                                k_off=C, **attn))
        self.free(qk); self.arena.release(vt)
        # --- attn1.to_out + residual, norm2 -> cross-attention query: one launch where the head segment runs
        y2, q2, _ = self.block_head(ao, b + ".attn1.to_out.0", b + ".attn2.to_q", 1, res=y)
        fused = y2 is not None
        if not fused:
            q2 = self.act(C, *HW)
            y2 = self.linear(ao, b + ".attn1.to_out.0", res=y)
        self.free(ao); self.free(y)
        if not fused:
            q2, n2 = self.ln_linear(y2, b + ".norm2", b + ".attn2.to_q", q2, T=T)
            self.free(n2)
        # --- text cross attention (K / V^T of all 16 layers come from two batched GEMMs at plan start)
        off, per_row = self.text_offsets[name], int(self.Bt > 1)
        ao = self.act(C, *HW)
        self.add(ops.flash_attn(q2.buf, self.text_k, self.text_vt, ao.buf, Tk=self.text_len, ldq=C, ldk=self.text_total, ldvt=TEXT_PAD,
                                sq=T * C, sk=per_row * TEXT_PAD * self.text_total, svt=per_row * self.text_total * TEXT_PAD, k_off=off,
                                vt_off=off * TEXT_PAD, **attn))
        self.free(q2)
        # --- attn2.to_out + residual -> feed-forward + residual -> proj_out + block residual: one launch where the tail segment runs
        tail = self.block_tail(ao, y2, x, b + ".attn2.to_out.0", b + ".ff", name + ".proj_out")
        if tail is not None:
            self.free(ao); self.free(y2)
            return tail
        y3 = self.linear(ao, b + ".attn2.to_out.0", res=y2)
        self.free(ao); self.free(y2)
        y4 = self.geglu_ff(y3, b + ".norm3", b + ".ff", T=T)
        self.free(y3)
        out = self.linear(y4, name + ".proj_out", res=x)
        self.free(y4)
        return out

    def motion(self, x: Act, name, idx_base: int) -> Act:
        cfg, W, B = self.cfg, self.W, self.B
        T, C, L = x.H * x.W, x.C, cfg.window_size
        t = name + ".temporal_transformer"
        b = t + ".transformer_blocks.0"
        # proj_in behind the module's GroupNorm, LayerNorm -> q | k | v of the first attention: one launch where the head segment runs
        y, qkv, _ = self.block_head(x, t + ".proj_in", b + ".attention_blocks.0.qkv", 3, gn_of=x)
        if y is None:
            y = self.gn_linear(x, t + ".norm", cfg.transformer_norm_eps, t + ".proj_in")
        for j in range(2):
            a = b + f".attention_blocks.{j}"
            if qkv is None:
                qkv, nrm = self.ln_linear(y, b + f".norms.{j}", a + ".qkv", self.act(3 * C, x.H, x.W))
                self.free(nrm)
            ao = self.act(C, x.H, x.W)
            pe = (W[a + ".q_pe"], W[a + ".k_pe"], W[a + ".v_pe"])
            cache = self.kv_cache[idx_base + j]
            if self.mode == "stream":
                op = self.add(ops.tattn_stream(qkv.buf, cache, *pe, self.in_pe_idx, self.in_upd, self.in_bias, ao.buf, N=B, T=T, C=C, L=L,
                                               H=cfg.temporal_heads, variant=self.tattn_variant))
            else:
                op = self.add(ops.tattn_warmup(qkv.buf, cache[0], *pe, ao.buf, F=B, T=T, C=C, L=L, H=cfg.temporal_heads))
            self.tattn_ops.append((op.tag, idx_base + j))
            self.free(qkv)
            y2 = qkv = None
            if j == 0:
                # to_out + residual, LayerNorm -> q | k | v of the second attention: one launch where the head segment runs
                y2, qkv, _ = self.block_head(ao, a + ".to_out.0", b + ".attention_blocks.1.qkv", 3, res=y)
            else:
                tail = self.block_tail(ao, y, x, a + ".to_out.0", b + ".ff", t + ".proj_out")
                if tail is not None:
                    self.free(ao); self.free(y)
                    return tail
            if y2 is None:
                y2 = self.linear(ao, a + ".to_out.0", res=y)
            self.free(ao); self.free(y)
            y = y2
        y2 = self.geglu_ff(y, b + ".ff_norm", b + ".ff")
        self.free(y)
        out = self.linear(y2, t + ".proj_out", res=x)
        self.free(y2)
        return out

    # ------------------------------------------------------------------ the plan
    def conditioning(self):
        """`cond_pl`: time embedding (sinusoid -> MLP -> SiLU -> every resnet's time_emb_proj in ONE skinny GEMM) and the text K / V^T
        of all cross-attention layers (two GEMMs)"""
        cfg, W, Bt = self.cfg, self.W, self.Bt
        self.use(self.cond_pl)
        c0, E = cfg.block_out_channels[0], cfg.time_embed_dim
        t_sin, t_h1, t_h2 = (torch.zeros(Bt, n, dtype=torch.float16, device=self.device) for n in (c0, E, E))
        self.add(ops.timestep_embed(self.in_t, t_sin, N=Bt, dim=c0))
        l1, l2 = "time_embedding.linear_1", "time_embedding.linear_2"
        self.add(ops.skinny_linear(t_sin, W[l1 + ".w"], W[l1 + ".b"], t_h1, M=Bt, K=c0, Nout=E, silu_out=True))
        self.add(ops.skinny_linear(t_h1, W[l2 + ".w"], W[l2 + ".b"], t_h2, M=Bt, K=E, Nout=E, silu_out=True))   # only silu(emb) is ever consumed (resnet.py:238)
        self.add(ops.skinny_linear(t_h2, W["temb_all.w"], W["temb_all.b"], self.temb_all, M=Bt, K=E, Nout=self.temb_total))
        D, kp, n = cfg.cross_attention_dim, self.text_kp, self.text_total
        self.gemm(self.in_enc, W["text_k.w"], self.text_k, M=Bt * TEXT_PAD, Nout=n, C1=D, ldx1=kp, CinP=kp, ldo=n)
        self.gemm(W["text_v.w"], self.in_enc, self.text_vt, M=n, Nout=TEXT_PAD, C1=D, ldx1=kp, CinP=kp, ldo=TEXT_PAD, batch=Bt, sx1=0,
                  sw=TEXT_PAD * kp, so=n * TEXT_PAD)
        self.use(self.pl)

    def stem(self) -> Act:
        """NCHW latents -> channels-last (padded to 8 channels), conv_in + depth mapping network"""
        cfg, hw = self.cfg, self.h * self.w
        x_in, d_in = self.act(8, self.h, self.w), self.act(8, self.h, self.w)
        self.add(ops.nchw_to_nhwc(self.in_sample, x_in.buf, B=self.B, C=cfg.in_channels, HW=hw, Cpad=8))
        self.add(ops.nchw_to_nhwc(self.in_depth, d_in.buf, B=self.B, C=cfg.in_channels, HW=hw, Cpad=8))
        x0 = self.conv3(x_in, "conv_in")
        e = self.conv3(d_in, "flow_conv_in.conv_in", epi=2)
        for i in range(self.n_map_blocks):
            e2 = self.conv3(e, f"flow_conv_in.blocks.{i}", epi=2)
            self.free(e)
            e = e2
        x = self.conv3(e, "flow_conv_in.conv_out", res=x0)     # depth embedding + conv_in(sample) (:523-526)
        for a in (e, x0, x_in, d_in):
            self.free(a)
        return x

    def blocks(self, x: Act) -> Act:
        """down -> mid -> up (`motion_module_idx` order): an input is given back once its block has run, unless a skip connection holds it"""
        skips, mm = [x], 0
        for blk in unet_blocks(self.cfg):
            skip = skips.pop() if blk.skip == "pop" else None
            if blk.kind == "resnet":
                y = self.resnet(x, blk.name, skip=skip)
            elif blk.kind == "spatial":
                y = self.spatial(x, blk.name)
            elif blk.kind == "motion":
                y, mm = self.motion(x, blk.name, mm), mm + 2
            else:
                y = self.conv3(x, blk.name, stride=(2 if blk.kind == "down" else 1), ups=int(blk.kind == "up"))
            if all(x is not s for s in skips):
                self.free(x)
            self.free(skip)
            x = y
            if blk.skip == "push":
                skips.append(x)
        return x

    def build(self) -> "UNetPlan":
        cfg = self.cfg
        self.conditioning()
        x = self.blocks(self.stem())
        hn = self.gn(x, "conv_norm_out", cfg.norm_eps, True)
        self.free(x)
        y = self.conv3(hn, "conv_out")
        self.add(ops.nhwc_to_nchw(y.buf, self.out_sample, B=self.B, C=cfg.out_channels, HW=self.h * self.w, ld=cfg.out_channels))
        self.kv_ptrs = [c.data_ptr() for c in self.kv_cache]
        return self.finish()
