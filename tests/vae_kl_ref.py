"""fp32 torch restatement of diffusers 0.25 `AutoencoderKL` (SD-1.5 configuration) on the keys of `sd_vae_param_spec`: encode to
moments, the posterior draw, decode.  Test infrastructure: the attention restatement is pinned to F.scaled_dot_product_attention /
nn.MultiheadAttention (tests/test_vae_kl_cpu.py); the resnet block, the bottom / right-padding down-sampler and the posterior clamp
are restated from diffusers (the AutoencoderKL section)."""
import torch
import torch.nn.functional as F

G, EPS = 32, 1e-6
LEVELS = 4


def _lin(x, sd, p):
    w = sd[p + ".weight"]
    return x @ w.reshape(w.shape[0], -1).t() + sd[p + ".bias"]


def _conv(x, sd, p, **kw):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], **kw)


def _gn(x, sd, p):
    return F.group_norm(x, G, sd[p + ".weight"], sd[p + ".bias"], EPS)


def resnet(x, sd, p):
    h = _conv(F.silu(_gn(x, sd, p + ".norm1")), sd, p + ".conv1", padding=1)
    h = _conv(F.silu(_gn(h, sd, p + ".norm2")), sd, p + ".conv2", padding=1)
    if (p + ".conv_shortcut.weight") in sd:
        x = _conv(x, sd, p + ".conv_shortcut")
    return x + h


def attention(x, sd, p):
    """GroupNorm, q / k / v, one head of d = C, scale C^-1/2, to_out.0, residual (rescale_output_factor 1)"""
    B, C, H, W = x.shape
    h = _gn(x, sd, p + ".group_norm").reshape(B, C, H * W).transpose(1, 2)
    q, k, v = (_lin(h, sd, f"{p}.{n}") for n in ("to_q", "to_k", "to_v"))
    a = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1) @ v
    return x + _lin(a, sd, p + ".to_out.0").transpose(1, 2).reshape(B, C, H, W)


def mid(x, sd, p):
    x = resnet(x, sd, p + ".resnets.0")
    x = attention(x, sd, p + ".attentions.0")
    return resnet(x, sd, p + ".resnets.1")


def encode(x, sd):
    """[B,3,H,W] -> moments [B,8,H/8,W/8] (mean = channels 0-3, raw logvar = 4-7)"""
    h = _conv(x, sd, "encoder.conv_in", padding=1)
    for i in range(LEVELS):
        for j in range(2):
            h = resnet(h, sd, f"encoder.down_blocks.{i}.resnets.{j}")
        if i < LEVELS - 1:
            h = _conv(F.pad(h, (0, 1, 0, 1)), sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", stride=2)
    h = mid(h, sd, "encoder.mid_block")
    h = _conv(F.silu(_gn(h, sd, "encoder.conv_norm_out")), sd, "encoder.conv_out", padding=1)
    return _conv(h, sd, "quant_conv")


def posterior(moments, eps):
    mean, logvar = moments[:, :4], moments[:, 4:].clamp(-30.0, 20.0)
    return mean + torch.exp(0.5 * logvar) * eps


def decode(z, sd):
    h = _conv(_conv(z, sd, "post_quant_conv"), sd, "decoder.conv_in", padding=1)
    h = mid(h, sd, "decoder.mid_block")
    for i in range(LEVELS):
        for j in range(3):
            h = resnet(h, sd, f"decoder.up_blocks.{i}.resnets.{j}")
        if i < LEVELS - 1:
            h = _conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", padding=1)
    return _conv(F.silu(_gn(h, sd, "decoder.conv_norm_out")), sd, "decoder.conv_out", padding=1)
