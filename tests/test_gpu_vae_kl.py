"""-m gpu: the SD AutoencoderKL (`HipAutoencoderKL`, vae_kl_hip.py) and its two new ops (csrc/vae_attn.hip) through the C ABI,
against torch fp32 (single ops) and the fp32 restatement tests/vae_kl_ref.py computed on the CPU (encode, decode, the pipeline).

Tolerances (fp16 storage, fp32 accumulate): the attention op rel-L2 <= 2e-3; the whole encoder / decoder rel-L2 <= 1e-2 and
cosine >= 0.9995 (the TAESD bounds)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


def _attn(L, qkv, B, T, ld, img, ws):
    out = torch.empty(B * T, 512, dtype=torch.float16, device=DEV)
    L.run(L.vae_attn(qkv, out, img, ws, B=B, T=T, ld=ld, ldo=512))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,T", [(1, 64), (2, 2304), (1, 4096), (1, 4225), (1, 9216)])
def test_vae_attn_op(L, B, T):
    """one head of d = 512 (the mid-block attention) against torch fp32 at the latent sizes of 64^2 .. 576x1024 images, odd T
    included; the same call twice is bit-identical, and so is a call on workspaces poisoned with NaN"""
    g = torch.Generator().manual_seed(B * 10000 + T)
    ld = 1536 + 8                                       # (a row stride wider than q | k | v)
    qkv = torch.randn(B * T, ld, generator=g)
    qkv[:, :512] *= 3.0                                 # sharper rows than unit scores
    qkv = qkv.half().to(DEV)
    q, k, v = (qkv[:, 512 * i:512 * (i + 1)].float().view(B, T, 512) for i in range(3))
    ref = torch.softmax(q @ k.transpose(1, 2) * 512 ** -0.5, dim=-1) @ v
    S = L.vae_attn_schedule(B, T)
    n_img, n_ws = L.vae_attn_sizes(B, T, S)
    img = torch.empty(n_img, dtype=torch.float16, device=DEV)
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=DEV)
    got = _attn(L, qkv, B, T, ld, img, ws)
    r = rel(got.view(B, T, 512), ref)
    print(f"B={B} T={T} splits={S}: rel-L2 {r:.3e}")
    assert torch.isfinite(got).all() and r <= 2e-3, r
    assert torch.equal(_attn(L, qkv, B, T, ld, img, ws), got)
    img.fill_(float("nan"))
    ws.fill_(float("nan"))
    assert torch.equal(_attn(L, qkv, B, T, ld, img, ws), got)


def test_vae_attn_rejects_shapes_it_cannot_take(L):
    from live2diff_amd import _lib
    qkv = torch.zeros(64, 1536, dtype=torch.float16, device=DEV)
    out = torch.zeros(64, 512, dtype=torch.float16, device=DEV)
    img = torch.zeros(L.vae_attn_sizes(1, 64, 1)[0], dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="vae_attn"):
        L.run(L.vae_attn(qkv, out, img, B=1, T=64, ld=1000, ldo=512, S=1))           # ld < 3 * 512
    assert _lib.OP_VAE_ATTN == 32 and _lib.OP_VAE_POSTERIOR == 33


def test_vae_posterior_op(L):
    g = torch.Generator().manual_seed(5)
    B, HW = 3, 37 * 23
    mom = (torch.randn(B, 8, HW, generator=g) * 4).half()
    mom[0, 4, :5] = -80.0                                # below the clamp
    mom[1, 5, :5] = 40.0                                 # above it
    eps = torch.randn(B, 4, HW, generator=g).half()
    out = torch.empty(B, 4, HW, dtype=torch.float16, device=DEV)
    L.run(L.vae_posterior(mom.to(DEV), eps.to(DEV), out, B=B, HW=HW))
    torch.cuda.synchronize()
    m32 = mom.float()
    ref = m32[:, :4] + torch.exp(0.5 * m32[:, 4:].clamp(-30, 20)) * eps.float()
    err = (out.float().cpu() - ref).abs() / ref.abs().clamp_min(1.0)
    assert err.max() <= 1e-3, err.max()


@pytest.fixture(scope="module")
def kl():
    from live2diff_amd.vae_kl_hip import HipAutoencoderKL, random_vae_kl_state_dict
    sd = random_vae_kl_state_dict()
    return HipAutoencoderKL(sd, device=DEV), {k: v.float() for k, v in sd.items()}


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (2, 128, 96), (1, 512, 512)])
def test_vae_kl_encode_decode_vs_oracle(kl, B, H, W):
    """moments and decoded image against the fp32 restatement on the same fp16-rounded weights and inputs; 64^2 and 128x96 run
    the fallback convs at their small levels (no cconv / producer statistics there), 512^2 the cconv path at every level"""
    import vae_kl_ref as R
    v, sd32 = kl
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).half()
    mom = v.encode(x.to(DEV)).latent_dist.parameters.clone()
    torch.cuda.synchronize()
    ref = R.encode(x.float(), sd32)
    assert mom.shape == ref.shape == (B, 8, H // 8, W // 8)
    print(f"encode {B}x{H}x{W}: rel-L2 {rel(mom, ref):.3e} cos {cos(mom, ref):.6f}")
    assert torch.isfinite(mom).all() and rel(mom, ref) <= 1e-2 and cos(mom, ref) >= 0.9995
    z = (torch.randn(B, 4, H // 8, W // 8, generator=g) * 1.5).half()
    img = v.decode(z.to(DEV), return_dict=False)[0].clone()
    torch.cuda.synchronize()
    ref = R.decode(z.float(), sd32)
    assert img.shape == ref.shape == (B, 3, H, W)
    print(f"decode {B}x{H}x{W}: rel-L2 {rel(img, ref):.3e} cos {cos(img, ref):.6f}")
    assert torch.isfinite(img).all() and rel(img, ref) <= 1e-2 and cos(img, ref) >= 0.9995
    assert torch.equal(v.decode(z.to(DEV), return_dict=False)[0], img)                 # static plan: bit-identical
    assert torch.equal(v.encode(x.to(DEV)).latent_dist.parameters, mom)


def test_vae_kl_sample_draws_like_diffusers(kl):
    """`latent_dist.sample(generator)`: one torch.randn per call on the generator's device (a CPU generator draws there and the
    sample moves), combined on the device by the posterior op; equal seeds give equal samples"""
    import vae_kl_ref as R
    v, _ = kl
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1).half().to(DEV)
    dist = v.encode(x).latent_dist
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    g3 = torch.Generator()
    g3.set_state(g1.get_state())                      # a clone of the generator the first sample draws from
    a, b = dist.sample(g1), dist.sample(g2)
    assert torch.equal(a, b)
    eps = torch.randn((2, 4, 8, 8), generator=g3, dtype=torch.float16)
    ref = R.posterior(dist.parameters.float().cpu(), eps.float())
    assert (a.float().cpu() - ref).abs().max() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(dist.mode(), dist.mean) and dist.mean.shape == (2, 4, 8, 8)
    assert torch.allclose(dist.std.float(), torch.exp(0.5 * dist.logvar.float()), rtol=2e-3)
    gd = torch.Generator(device=DEV).manual_seed(3)
    assert dist.sample(gd).device.type == "cuda" and not torch.equal(dist.sample(), dist.sample())


def test_pipeline_runs_on_hip_vae_kl():
    """StreamAnimateDiffusionDepth with `stream.vae` = HipAutoencoderKL and, separately, an oracle-backed AutoencoderKL object,
    the same generator seed for both: `prepare` + frames agree within the VAE tolerance, which holds only if both sides draw
    their posterior samples and noise in the same order (encode_image: sample, noise; encode_depth: sample)"""
    from types import SimpleNamespace

    import vae_kl_ref as R
    from live2diff_amd.config import tiny_config
    from live2diff_amd.pipeline_stream_animation_depth import StreamAnimateDiffusionDepth
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.vae_kl_hip import HipAutoencoderKL, _randn_like_diffusers, random_vae_kl_state_dict
    from live2diff_amd.weights import random_state_dict
    cfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=64)
    H = W = 64
    sd = {k: v.to(DEV) for k, v in random_state_dict(cfg, dtype=torch.float16).items()}
    vsd = random_vae_kl_state_dict()
    vsd32 = {k: v.float() for k, v in vsd.items()}

    class OracleDist:
        def __init__(self, m):
            self.m = m

        def sample(self, generator=None):
            eps = _randn_like_diffusers((self.m.shape[0], 4) + tuple(self.m.shape[2:]), generator, torch.device(DEV), torch.float16)
            return R.posterior(self.m, eps.float().cpu()).half().to(DEV)

    class OracleVAE:                    # test infrastructure (CPU fp32) in the caller-owned `stream.vae` slot
        dtype = torch.float16
        config = SimpleNamespace(scaling_factor=0.18215)

        def encode(self, x):
            return SimpleNamespace(latent_dist=OracleDist(R.encode(x.float().cpu(), vsd32)))

        def decode(self, z, return_dict=False):
            return (R.decode(z.float().cpu(), vsd32).half().to(DEV),)

    class StubDepth:
        dtype = torch.float16

        def __call__(self, images):
            return (images.float().mean(1) * 4 + 9).to(torch.float16)

    g = torch.Generator().manual_seed(8)
    warm = [torch.rand(3, H, W, generator=g) for _ in range(cfg.sink_size)]
    frames = [torch.rand(1, 3, H, W, generator=g) for _ in range(3)]
    emb = torch.randn(1, 77, 64, generator=g)
    outs = []
    for hip in (True, False):
        torch.manual_seed(0)
        pipe = SimpleNamespace(device=torch.device(DEV), vae_scale_factor=8, unet=HipStreamingUNet(sd, cfg, H // 8, W // 8, 2),
                               vae=(HipAutoencoderKL(vsd, device=DEV) if hip else OracleVAE()), depth_model=StubDepth(), scheduler=None)
        s = StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, do_add_noise=False,
                                        warmup_frames=cfg.sink_size, window_size=cfg.window_size)
        s.prepare_cache(H, W, 2)
        first = s.prepare(warm, prompt_embeds=emb, seed=3)
        res = [s(f.to(DEV)).clone() for f in frames]
        assert torch.isfinite(first).all() and all(torch.isfinite(r).all() for r in res)
        outs.append([first] + res)
    for i, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape
        print(f"frame {i}: rel-L2 {rel(a, b):.3e}")
        assert rel(a, b) <= 3e-2 and cos(a, b) >= 0.999, (i, rel(a, b))
