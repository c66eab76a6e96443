"""CPU tests (-m "not gpu") of the SD AutoencoderKL host side: parameter inventory, the LDM -> diffusers key map pinned to the
reference's converter, weight-ingestion errors, plan validation without a device, and the fp32 restatement's own pins."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def _zeros_sd():
    from live2diff_amd.vae_kl_hip import sd_vae_param_spec
    return {k: torch.zeros(s, dtype=torch.float16) for k, s in sd_vae_param_spec().items()}


def test_vae_kl_spec_matches_the_published_model():
    from live2diff_amd.vae_kl_hip import sd_vae_param_spec
    spec = sd_vae_param_spec()
    assert len(spec) == 248 and sum(torch.Size(s).numel() for s in spec.values()) == 83653863
    assert spec["encoder.conv_out.weight"] == (8, 512, 3, 3) and spec["quant_conv.weight"] == (8, 8, 1, 1)
    assert spec["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert spec["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert spec["decoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in spec and "decoder.up_blocks.3.upsamplers.0.conv.weight" not in spec


def test_vae_converter_matches_the_reference_key_map():
    """tests/golden/vae_kl_convert_keys.json: the reference's convert_ldm_vae_checkpoint on a tagged synthetic checkpoint"""
    from live2diff_amd.convert import LDM_VAE_PREFIX, build_vae_state_dict, convert_ldm_vae_checkpoint, ldm_vae_key_map
    from live2diff_amd.vae_kl_hip import sd_vae_param_spec
    gold = json.load(open(os.path.join(GOLDEN, "vae_kl_convert_keys.json")))
    assert ldm_vae_key_map() == gold["keys"]
    spec = sd_vae_param_spec()
    ckpt = {}
    for i, (old, new) in enumerate(ldm_vae_key_map().items()):
        shp = spec[new] + ((1, 1) if ".attn_1." in old and len(spec[new]) == 2 else ())
        ckpt[LDM_VAE_PREFIX + old] = torch.full(shp, float(i))
    out = convert_ldm_vae_checkpoint(ckpt)
    assert {k: list(v.shape) for k, v in out.items()} == gold["shapes"]
    # DreamBooth (first_stage_model.*) then a standalone VAE file under `state_dict`, in that order, over the base dict
    base = {k: torch.zeros(1) for k in spec}
    vae_file = {"state_dict": {k[len(LDM_VAE_PREFIX):]: v + 1000 for k, v in ckpt.items()}}
    sd = build_vae_state_dict(base, dreambooth=ckpt)
    assert torch.equal(sd["decoder.conv_in.weight"], out["decoder.conv_in.weight"])
    sd = build_vae_state_dict(base, dreambooth=ckpt, vae=vae_file)
    assert torch.equal(sd["decoder.conv_in.weight"], out["decoder.conv_in.weight"] + 1000)
    del ckpt[LDM_VAE_PREFIX + "encoder.mid.attn_1.q.weight"]
    with pytest.raises(KeyError):
        convert_ldm_vae_checkpoint(ckpt)


def test_vae_kl_weight_ingestion_errors(dry_run):
    from live2diff_amd.vae_kl_hip import HipAutoencoderKL
    sd = _zeros_sd()
    for k in list(sd):
        if ".attentions.0.to_" in k and k.endswith("weight"):
            sd[k] = sd[k][:, :, None, None]                   # LDM-style 1x1 conv projections are accepted
    v = HipAutoencoderKL(sd, device="cpu")
    assert v.sd["encoder.mid_block.attentions.0.to_q.weight"].shape == (512, 512)
    with pytest.raises(ValueError):
        v.encode(torch.zeros(1, 3, 100, 64, dtype=torch.float16))
    sd.pop("decoder.conv_out.bias")
    with pytest.raises(KeyError):
        HipAutoencoderKL(sd, device="cpu")


@pytest.mark.parametrize("B,H,W", [(1, 512, 512), (8, 256, 256), (1, 576, 1024), (1, 520, 392)])
def test_vae_kl_plans_validate_without_gpu(dry_run, B, H, W):
    from live2diff_amd import _lib
    from live2diff_amd.vae_kl_hip import HipAutoencoderKL
    v = HipAutoencoderKL(_zeros_sd(), device="cpu")
    dist = v.encode(torch.zeros(B, 3, H, W, dtype=torch.float16)).latent_dist
    assert dist.parameters.shape == (B, 8, H // 8, W // 8) and dist.mean.shape == (B, 4, H // 8, W // 8)
    img = v.decode(torch.zeros(B, 4, H // 8, W // 8, dtype=torch.float16), return_dict=False)[0]
    assert img.shape == (B, 3, H, W)
    assert v.config.scaling_factor == 0.18215 and v.config.latent_channels == 4 and v.dtype == torch.float16 and v.to("cuda") is v
    s = v.plan_summary()
    enc, dec = s[("enc", B, H, W)], s[("dec", B, H // 8, W // 8)]
    for p in (enc, dec):
        assert p["kinds"]["vae_attn"] == 1 and p["batch"] == B
    if (H, W) == (512, 512):
        # every resnet conv of the 512^2 levels on cconv with the GroupNorm prologue (20 encoder / 28 decoder convs), the
        # decoder's up-samplers too
        assert enc["cconv_gn"] == 20 and dec["cconv_gn"] == 28 and dec["kinds"]["cconv"] == 31 and enc["gn_fallback"] == 0
    if (H, W) == (520, 392):
        assert "cconv" not in enc["kinds"] and enc["gn_fallback"] > 0       # 392 / 16 is no whole patch: the fallback path
    assert _lib.OP_VAE_ATTN == 32


def test_vae_kl_sub_batches_bound_the_largest_activation():
    from live2diff_amd.vae_kl_hip import HipAutoencoderKL
    assert HipAutoencoderKL._sub_batch("dec", 64, 64) == 15                # 256 ch x 512^2 x 2 B = 128 MB per sample
    assert HipAutoencoderKL._sub_batch("dec", 72, 128) * 256 * 576 * 1024 * 2 < 2 ** 31
    assert HipAutoencoderKL._sub_batch("enc", 512, 512) >= 8


def test_oracle_attention_matches_sdpa_and_multihead_attention():
    """the restatement's mid-block attention (one head, d = C, GroupNorm in front, residual) against
    F.scaled_dot_product_attention and nn.MultiheadAttention with the same projections"""
    import vae_kl_ref as R
    g = torch.Generator().manual_seed(0)
    C, H, W = 64, 6, 5
    R_G = R.G
    R.G = 8
    try:
        sd = {"a.group_norm.weight": 1 + 0.1 * torch.randn(C, generator=g), "a.group_norm.bias": 0.1 * torch.randn(C, generator=g)}
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            sd[f"a.{n}.weight"] = torch.randn(C, C, generator=g) * C ** -0.5
            sd[f"a.{n}.bias"] = 0.1 * torch.randn(C, generator=g)
        x = torch.randn(2, C, H, W, generator=g)
        got = R.attention(x, sd, "a")
        h = F.group_norm(x, 8, sd["a.group_norm.weight"], sd["a.group_norm.bias"], 1e-6).flatten(2).transpose(1, 2)
        q, k, v = (h @ sd[f"a.{n}.weight"].t() + sd[f"a.{n}.bias"] for n in ("to_q", "to_k", "to_v"))
        a = F.scaled_dot_product_attention(q, k, v)
        ref = x + (a @ sd["a.to_out.0.weight"].t() + sd["a.to_out.0.bias"]).transpose(1, 2).reshape(x.shape)
        assert torch.allclose(got, ref, atol=1e-5)
        mha = torch.nn.MultiheadAttention(C, 1, batch_first=True)
        with torch.no_grad():
            mha.in_proj_weight.copy_(torch.cat([sd[f"a.{n}.weight"] for n in ("to_q", "to_k", "to_v")]))
            mha.in_proj_bias.copy_(torch.cat([sd[f"a.{n}.bias"] for n in ("to_q", "to_k", "to_v")]))
            mha.out_proj.weight.copy_(sd["a.to_out.0.weight"])
            mha.out_proj.bias.copy_(sd["a.to_out.0.bias"])
            m = mha(h, h, h, need_weights=False)[0]
        assert torch.allclose(got, x + m.transpose(1, 2).reshape(x.shape), atol=1e-5)
        # rows of a batch do not interact
        assert torch.allclose(R.attention(x[1:], sd, "a"), got[1:], atol=1e-6)
    finally:
        R.G = R_G


def test_oracle_downsampler_and_posterior():
    """the down-sampler pads the bottom / right edges only (what igemm's pad_same does), and the posterior clamps logvar to
    [-30, 20]"""
    import vae_kl_ref as R
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, 16, 24, generator=g)
    w = torch.randn(5, 4, 3, 3, generator=g)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    assert y.shape == (1, 5, 8, 12)
    # output row i reads input rows 2i .. 2i + 2 (the last one past the edge is zero): no top / left padding
    xp = torch.zeros(1, 4, 17, 25)
    xp[..., :16, :24] = x
    assert torch.allclose(y[0, :, 3, 4], (xp[0, :, 6:9, 8:11][None] * w).sum((1, 2, 3)), atol=1e-5)
    m = torch.zeros(1, 8, 2, 2)
    m[:, 4:] = torch.tensor([-100.0, 100.0, 0.0, 2.0]).view(1, 1, 2, 2).expand(1, 4, 2, 2)
    eps = torch.ones(1, 4, 2, 2)
    z = R.posterior(m, eps)
    assert torch.allclose(z[0, 0].flatten(), torch.exp(0.5 * torch.tensor([-30.0, 20.0, 0.0, 2.0])))
