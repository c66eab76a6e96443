"""HipAutoencoderKL -- the SD-1.5 `AutoencoderKL` in the `stream.vae` slot when the tiny VAE is off.

Boundary (reference): with `use_tiny_vae=False` (live2diff/utils/wrapper.py:37, :468-470) `stream.vae` is the pipeline's own
diffusers 0.25 `AutoencoderKL` (animatediff/pipeline/pipeline_animatediff_depth.py:267), whose weights a DreamBooth style or a
separate VAE file may replace (animatediff/converter/convert.py:40-45, :52-69; here `convert.build_vae_state_dict`).  The
pipeline calls `vae.encode(x).latent_dist.sample(generator)` (pipeline_stream_animation_depth.py:317 image, :345 depth map)
and `vae.decode(z, return_dict=False)[0]` (:322), and reads `vae.config.scaling_factor` and `vae.dtype`.

The network (block_out_channels 128, 256, 512, 512; 2 resnets per encoder level, 3 per decoder level; GroupNorm 32 / eps 1e-6;
one single-head attention of d = 512 in each mid block) runs on the UNet's kernels, one static plan per (side, batch, H, W):
  * channels-last fp16 activations `[B*H*W, C]` from the plan's `Arena`; the image / latent are padded to 8 channels by the layout op;
  * resnet: the GroupNorm statistics come from the epilogue of the op that wrote x (`ops.gn_target`); where `ops.cconv_ok`
    holds the conv is `cconv` with its GroupNorm + SiLU prologue, elsewhere `gn_apply` + the implicit-GEMM / patch conv (the
    `gn_stats` / one-launch forms when no producer can take the statistics); conv2 adds the shortcut (a 1x1 igemm when the
    width changes) in its epilogue;
  * down-sampler: igemm with stride 2 and `pad_same` (bottom / right padding, the same as diffusers' F.pad(0, 1, 0, 1) + pad 0
    for every side divisible by 8); up-sampler: nearest x2 folded into the conv's gather;
  * attention: GroupNorm, one q | k | v igemm (Nout 1536), `ops.vae_attn` (csrc/vae_attn.hip), the to_out igemm with the
    residual in its epilogue;
  * `quant_conv` is folded into the encoder's conv_out on the host (a linear map of a conv's output); `post_quant_conv` stays
    its own 1x1 launch (folding its bias into decoder.conv_in would put it under that conv's zero padding);
  * the conv kernels form byte offsets in 32 bits: a batch whose largest activation would reach 2^31 bytes runs as
    sub-batches through one plan.
"""
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

from . import _lib, ops
from .plan import Act, PlanBuilder

BLOCK_OUT = (128, 256, 512, 512)
ENC_LAYERS, DEC_LAYERS = 2, 3
GROUPS, EPS = 32, 1e-6
SCALING_FACTOR = 0.18215
ATTN_LINEARS = ("to_q", "to_k", "to_v", "to_out.0")
MAX_ACT_BYTES = (1 << 31) - 1        # the conv kernels' 32-bit byte offsets


def sd_vae_param_spec() -> "OrderedDict[str, Tuple[int, ...]]":
    """diffusers `AutoencoderKL.state_dict()` names -> shapes (SD-1.5 configuration: 248 tensors, 83 653 863 parameters)."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(p, cin, cout, k=3):
        spec[p + "weight"] = (cout, cin, k, k)
        spec[p + "bias"] = (cout,)

    def norm(p, c):
        spec[p + "weight"] = (c,)
        spec[p + "bias"] = (c,)

    def resnet(p, cin, cout):
        norm(p + "norm1.", cin)
        conv(p + "conv1.", cin, cout)
        norm(p + "norm2.", cout)
        conv(p + "conv2.", cout, cout)
        if cin != cout:
            conv(p + "conv_shortcut.", cin, cout, 1)

    def mid(p, c):
        a = p + "attentions.0."
        norm(a + "group_norm.", c)
        for n in ATTN_LINEARS:
            spec[a + n + ".weight"] = (c, c)
            spec[a + n + ".bias"] = (c,)
        resnet(p + "resnets.0.", c, c)
        resnet(p + "resnets.1.", c, c)

    conv("encoder.conv_in.", 3, BLOCK_OUT[0])
    cin = BLOCK_OUT[0]
    for i, c in enumerate(BLOCK_OUT):
        for j in range(ENC_LAYERS):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}.", cin if j == 0 else c, c)
        cin = c
        if i < len(BLOCK_OUT) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv.", c, c)
    mid("encoder.mid_block.", BLOCK_OUT[-1])
    norm("encoder.conv_norm_out.", BLOCK_OUT[-1])
    conv("encoder.conv_out.", BLOCK_OUT[-1], 8)
    conv("decoder.conv_in.", 4, BLOCK_OUT[-1])
    mid("decoder.mid_block.", BLOCK_OUT[-1])
    cin = BLOCK_OUT[-1]
    for i, c in enumerate(reversed(BLOCK_OUT)):
        for j in range(DEC_LAYERS):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}.", cin if j == 0 else c, c)
        cin = c
        if i < len(BLOCK_OUT) - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv.", c, c)
    norm("decoder.conv_norm_out.", BLOCK_OUT[0])
    conv("decoder.conv_out.", BLOCK_OUT[0], 3)
    conv("quant_conv.", 8, 8, 1)
    conv("post_quant_conv.", 4, 4, 1)
    return spec


def random_vae_kl_state_dict(dtype=torch.float16, device="cpu") -> Dict[str, torch.Tensor]:
    """Key-hashed deterministic weights (weights._fill: seed = crc32(key)); GroupNorm scales near 1."""
    from .weights import _fill
    out = OrderedDict()
    for k, shp in sd_vae_param_spec().items():
        t = _fill("vae_kl." + k, shp, 1.0)
        if k.endswith("group_norm.weight"):
            t = 1.0 + 0.1 * t
        out[k] = t.to(device=device, dtype=dtype)
    return out


def _randn_like_diffusers(shape, generator, device, dtype):
    """diffusers.utils.torch_utils.randn_tensor: a CPU generator draws on the CPU and the sample is moved; a list draws per row"""
    if isinstance(generator, (list, tuple)):
        if len(generator) == 1:
            generator = generator[0]
        else:
            rows = [_randn_like_diffusers((1,) + tuple(shape[1:]), g, device, dtype) for g in generator]
            return torch.cat(rows, 0)
    rand_device = device
    if generator is not None and generator.device.type != torch.device(device).type:
        if generator.device.type != "cpu":
            raise ValueError(f"cannot draw a {device} tensor from a {generator.device.type} generator")
        rand_device = "cpu"
    return torch.randn(shape, generator=generator, device=rand_device, dtype=dtype).to(device)


class HipDiagonalGaussian:
    """diffusers' DiagonalGaussianDistribution over the encoder's moments [B, 8, h, w] (fp16): `sample` draws eps the way
    diffusers does (one randn per call) and combines on the device (ops.vae_posterior)."""

    def __init__(self, moments: torch.Tensor):
        self.parameters = moments
        self.deterministic = False

    @property
    def mean(self):
        return self.parameters[:, :4]

    @property
    def logvar(self):
        return self.parameters[:, 4:].clamp(-30.0, 20.0)

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self):
        return torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def sample(self, generator=None) -> torch.Tensor:
        B, _, h, w = self.parameters.shape
        eps = _randn_like_diffusers((B, 4, h, w), generator, self.parameters.device, torch.float16)
        out = torch.empty(B, 4, h, w, dtype=torch.float16, device=self.parameters.device)
        ops.run(ops.vae_posterior(self.parameters, eps.contiguous(), out, B=B, HW=h * w))
        return out


class _Out:
    """`.latent_dist` / `.sample` holder (diffusers AutoencoderKLOutput / DecoderOutput)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class HipAutoencoderKL:
    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda"):
        self.device = torch.device(device)
        self.dtype = torch.float16
        self.config = SimpleNamespace(scaling_factor=SCALING_FACTOR, latent_channels=4, in_channels=3, out_channels=3,
                                      block_out_channels=BLOCK_OUT, layers_per_block=ENC_LAYERS, norm_num_groups=GROUPS)
        self.device_name = "dry-run" if ops.DRY_RUN else _lib.device_name()
        spec = sd_vae_param_spec()
        missing = [k for k in spec if k not in state_dict]
        if missing:
            raise KeyError(f"AutoencoderKL state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
        sd = {}
        for k, shp in spec.items():
            t = state_dict[k]
            if ".attentions.0.to_" in k and t.dim() == 4 and tuple(t.shape[2:]) == (1, 1):
                t = t[:, :, 0, 0]                    # LDM checkpoints keep the attention projections as 1x1 convs
            if tuple(t.shape) != tuple(shp):
                raise ValueError(f"{k}: shape {tuple(t.shape)}, expected {shp}")
            sd[k] = t.detach().to(device=self.device, dtype=torch.float16)
        # quant_conv folded into encoder.conv_out (exact: a 1x1 linear map of the conv's output), in fp32
        wq, bq = state_dict["quant_conv.weight"].float().reshape(8, 8).cpu(), state_dict["quant_conv.bias"].float().cpu()
        wc, bc = state_dict["encoder.conv_out.weight"].float().cpu(), state_dict["encoder.conv_out.bias"].float().cpu()
        sd["encoder.conv_out.weight"] = torch.einsum("om,mikl->oikl", wq, wc).to(self.device, torch.float16)
        sd["encoder.conv_out.bias"] = (wq @ bc + bq).to(self.device, torch.float16)
        # post_quant_conv padded to 8 output channels (zero rows, zero bias): the decoder's conv_in then reads whole 16-byte rows
        wp = torch.zeros(8, 4, dtype=torch.float16, device=self.device)
        wp[:4] = sd["post_quant_conv.weight"].reshape(4, 4)
        bp = torch.zeros(8, dtype=torch.float16, device=self.device)
        bp[:4] = sd["post_quant_conv.bias"]
        sd["post_quant_conv.weight"], sd["post_quant_conv.bias"] = wp, bp
        self.sd = sd
        self._packed = {}
        self._plans = {}

    # duck-typed members of the reference's vae
    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------ packed weights (built on first use, shared by plans)
    def _pk(self, key, fn):
        t = self._packed.get(key)
        if t is None:
            t = self._packed[key] = fn()
        return t

    def _conv3_w(self, name):
        return self._pk((name, "igemm"), lambda: ops.pack_conv3x3(self.sd[name + ".weight"]))

    def _cconv_w(self, name, kg):
        # keyed by the K-group count: a plan never streams weights packed for another schedule's KG
        return self._pk((name, "cconv", kg), lambda: ops.pack_cconv(self.sd[name + ".weight"], kg))

    def _lin_w(self, name):
        return self._pk((name, "linear"), lambda: ops.pack_linear(self.sd[name + ".weight"]))

    def _bias(self, name):
        return self._pk((name, "bias"), lambda: ops.f32(self.sd[name + ".bias"]))

    def _qkv(self, p):
        w = self._pk((p, "qkv"), lambda: ops.pack_linear(torch.cat([self.sd[f"{p}.{n}.weight"] for n in ATTN_LINEARS[:3]], 0)))
        b = self._pk((p, "qkv_b"), lambda: ops.f32(torch.cat([self.sd[f"{p}.{n}.bias"] for n in ATTN_LINEARS[:3]], 0)))
        return w, b

    # ------------------------------------------------------------------ plans
    @staticmethod
    def _sub_batch(side: str, H: int, W_: int) -> int:
        """largest batch whose biggest activation stays below 2^31 bytes (decoder: 256 channels at the image size; encoder:
        128 channels at the image size)"""
        img = H * W_ * (64 if side == "dec" else 1)
        per = img * (256 if side == "dec" else 128) * 2
        return max(1, MAX_ACT_BYTES // per)

    def _build(self, side: str, B: int, H: int, W_: int):
        """side 'enc': static input [B,3,H,W] -> moments [B,8,H/8,W/8]; 'dec': [B,4,h,w] latent -> [B,3,8h,8w]."""
        dev = self.device
        st = PlanBuilder(dev, B, sk_counters=1 << 16, gn_layers=96, G=GROUPS)
        st.cconv_gn = 0
        ar, add, gemm, new_act, free = st.arena, st.add, st.gemm, st.act, st.free

        def gn_acc_of(x: Act):
            """ask x's producer to accumulate this GroupNorm's statistics; the accumulator pointer or None"""
            return st.gn_acc_for([(x.producer, 0)], T=x.H * x.W, cpg=x.C // GROUPS)

        def gn(x: Act, name, silu, acc_ptr=None) -> Act:
            out = new_act(x.C, x.H, x.W)
            st.groupnorm(x.buf, self.sd[name + ".weight"], self.sd[name + ".bias"], out.buf, T=x.H * x.W, C1=x.C, eps=EPS, act=silu,
                         acc_ptr=acc_ptr)
            return out

        def conv3(x: Act, name, stride=1, ups=0, res: Optional[Act] = None, gn_name=None, ldo=None) -> Act:
            """3x3 conv (of silu(GroupNorm(x)) when gn_name is given)"""
            cout = self.sd[name + ".weight"].shape[0]
            Ho, Wo = (x.H * 2, x.W * 2) if ups else ((x.H // 2, x.W // 2) if stride == 2 else (x.H, x.W))
            rk = dict(res=(res.buf if res is not None else None), ldr=(res.C if res is not None else 0))
            acc_ptr = gn_acc_of(x) if gn_name else None
            if stride == 1 and ops.cconv_ok(Ho, Wo, cout, x.C) and (gn_name is None or acc_ptr is not None):
                out = new_act(cout, Ho, Wo)
                sched = ops.cconv_schedule(B, Ho, Wo, cout, x.C)
                kw = {}
                if gn_name is not None:
                    st.cconv_gn += 1
                    kw.update(gn_acc_ptr=acc_ptr, gn_gamma=self.sd[gn_name + ".weight"], gn_beta=self.sd[gn_name + ".bias"],
                              gn_G=GROUPS, gn_eps=EPS)
                out.producer = st.cconv(x.buf, self._cconv_w(name, sched[1]), out.buf, B=B, H=Ho, W=Wo, C1=x.C, ldx1=x.C,
                                        Nout=cout, ldo=cout, KG=sched[1], ups=ups, bias=self._bias(name), sched=sched, **rk, **kw)
                return out
            hn = gn(x, gn_name, True, acc_ptr) if gn_name else x
            wt = self._conv3_w(name)
            cinp = wt.shape[1] // 9
            ldo = ldo or cout
            out = new_act(cout, Ho, Wo, ld=ldo)
            patch = ops.pconv_patch(B, x.H, x.W, cout, hn.C) if (stride == 1 and not ups and cinp == hn.C) else None
            if patch is not None:
                out.producer = add(ops.pconv(hn.buf, wt, out.buf, B=B, H=x.H, W=x.W, C1=hn.C, ldx1=hn.C, CinP=cinp, Nout=cout, ldo=ldo,
                                             patch=patch, bias=self._bias(name), **rk))
            else:
                out.producer = gemm(hn.buf, wt, out.buf, M=B * Ho * Wo, Nout=cout, C1=hn.C, ldx1=hn.C,
                                    CinP=cinp, ldo=ldo, bias=self._bias(name), taps=9, B=B, Hin=x.H, Win=x.W, Hout=Ho, Wout=Wo,
                                    stride=stride, ups=ups, pad_same=(stride == 2), **rk)
            if gn_name:
                free(hn)
            return out

        def linear(x: Act, wt, bias, nout, res: Optional[Act] = None, ldo=None) -> Act:
            ldo = ldo or nout
            out = new_act(nout, x.H, x.W, ld=ldo)
            out.producer = gemm(x.buf, wt, out.buf, M=B * x.H * x.W, Nout=nout, C1=x.C, ldx1=x.C, CinP=wt.shape[1], ldo=ldo,
                                bias=bias, res=(res.buf if res is not None else None), ldr=(res.C if res is not None else 0))
            return out

        def resnet(x: Act, p) -> Act:
            h1 = conv3(x, p + ".conv1", gn_name=p + ".norm1")
            sc = None
            if (p + ".conv_shortcut.weight") in self.sd:
                sc = linear(x, self._lin_w(p + ".conv_shortcut"), self._bias(p + ".conv_shortcut"), h1.C)
            out = conv3(h1, p + ".conv2", gn_name=p + ".norm2", res=(sc if sc is not None else x))
            free(h1)
            free(sc)
            free(x)
            return out

        def attention(x: Act, p) -> Act:
            T = x.H * x.W
            hn = gn(x, p + ".group_norm", ops.ACT_NONE, gn_acc_of(x))
            wqkv, bqkv = self._qkv(p)
            qkv = linear(hn, wqkv, bqkv, 3 * x.C)
            free(hn)
            a = new_act(x.C, x.H, x.W)
            S = ops.vae_attn_schedule(B, T)
            n_img, n_ws = ops.vae_attn_sizes(B, T, S)
            img = ar.alloc(n_img)
            ws = ar.alloc(n_ws, torch.float32) if n_ws else None
            add(ops.vae_attn(qkv.buf, a.buf, img, ws, B=B, T=T, ld=3 * x.C, ldo=x.C, S=S))
            ar.release(img)
            ar.release(ws)
            free(qkv)
            out = linear(a, self._lin_w(p + ".to_out.0"), self._bias(p + ".to_out.0"), x.C, res=x)
            free(a)
            free(x)
            return out

        def mid(x: Act, p) -> Act:
            x = resnet(x, p + ".resnets.0")
            x = attention(x, p + ".attentions.0")
            return resnet(x, p + ".resnets.1")

        h, w = H, W_
        if side == "enc":
            st.inp = torch.zeros(B, 3, h * w, dtype=torch.float16, device=dev)
            x = new_act(8, h, w)
            add(ops.nchw_to_nhwc(st.inp, x.buf, B=B, C=3, HW=h * w, Cpad=8))
            y = conv3(x, "encoder.conv_in")
            free(x)
            x = y
            for i in range(len(BLOCK_OUT)):
                for j in range(ENC_LAYERS):
                    x = resnet(x, f"encoder.down_blocks.{i}.resnets.{j}")
                if i < len(BLOCK_OUT) - 1:
                    y = conv3(x, f"encoder.down_blocks.{i}.downsamplers.0.conv", stride=2)
                    free(x)
                    x = y
            x = mid(x, "encoder.mid_block")
            y = conv3(x, "encoder.conv_out", gn_name="encoder.conv_norm_out")         # (quant_conv folded in)
            free(x)
            st.out = torch.zeros(B, 8, y.H * y.W, dtype=torch.float16, device=dev)
            add(ops.nhwc_to_nchw(y.buf, st.out, B=B, C=8, HW=y.H * y.W, ld=8))
            st.out_shape = (B, 8, y.H, y.W)
        else:
            st.inp = torch.zeros(B, 4, h * w, dtype=torch.float16, device=dev)
            x = new_act(8, h, w)
            add(ops.nchw_to_nhwc(st.inp, x.buf, B=B, C=4, HW=h * w, Cpad=8))
            y = linear(x, self._lin_w("post_quant_conv"), self._bias("post_quant_conv"), 8)
            free(x)
            x = conv3(y, "decoder.conv_in")
            free(y)
            x = mid(x, "decoder.mid_block")
            for i in range(len(BLOCK_OUT)):
                for j in range(DEC_LAYERS):
                    x = resnet(x, f"decoder.up_blocks.{i}.resnets.{j}")
                if i < len(BLOCK_OUT) - 1:
                    y = conv3(x, f"decoder.up_blocks.{i}.upsamplers.0.conv", ups=1)
                    free(x)
                    x = y
            y = conv3(x, "decoder.conv_out", gn_name="decoder.conv_norm_out", ldo=4)
            free(x)
            st.out = torch.zeros(B, 3, y.H * y.W, dtype=torch.float16, device=dev)
            add(ops.nhwc_to_nchw(y.buf, st.out, B=B, C=3, HW=y.H * y.W, ld=4))
            st.out_shape = (B, 3, y.H, y.W)
        return st.finish()

    def _plan(self, side, B, H, W_):
        if side == "enc" and (H % 8 or W_ % 8):
            raise ValueError(f"image size {H}x{W_} must be divisible by 8")
        Bp = min(B, self._sub_batch(side, H, W_))
        key = (side, Bp, H, W_)
        st = self._plans.get(key)
        if st is None:
            st = self._plans[key] = self._build(side, Bp, H, W_)
        return st

    def _run(self, side, x, cin):
        B, C, H, W_ = x.shape
        if C != cin:
            raise ValueError(f"{'encode' if side == 'enc' else 'decode'} expects [B,{cin},H,W], got {tuple(x.shape)}")
        st = self._plan(side, B, H, W_)
        if B == st.B:
            st.inp.copy_(x.reshape(B, C, H * W_))
            st.pl.run()
            return st.out.view(st.out_shape)
        out = torch.empty((B,) + st.out_shape[1:], dtype=torch.float16, device=self.device)
        for b0 in range(0, B, st.B):                  # sub-batches through one plan (a short last one leaves stale rows unread)
            n = min(st.B, B - b0)
            st.inp[:n].copy_(x[b0:b0 + n].reshape(n, C, H * W_))
            st.pl.run()
            out[b0:b0 + n] = st.out[:n].view((n,) + st.out_shape[1:])
        return out

    # ------------------------------------------------------------------ the boundary calls
    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """x [B,3,H,W] in [-1,1] -> `.latent_dist` over moments [B,8,H/8,W/8] (a view of the plan's static output, valid until the
        next encode of the same shape)."""
        dist = HipDiagonalGaussian(self._run("enc", x, 3))
        return _Out(latent_dist=dist) if return_dict else (dist,)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, generator=None, return_dict: bool = True):
        img = self._run("dec", z, 4)
        return _Out(sample=img) if return_dict else (img,)

    def plan_summary(self):
        names = {v: k[3:].lower() for k, v in vars(_lib).items() if k.startswith("OP_") and isinstance(v, int)}
        return {k: dict(st.summary(), batch=st.B, gn_fallback=st.gn_self_launches + st.gn_stats_launches, cconv_gn=st.cconv_gn,
                        kinds={names.get(kd, kd): n for kd, n in sorted(st.kinds.items())})
                for k, st in self._plans.items()}
