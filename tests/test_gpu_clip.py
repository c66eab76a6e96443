"""GPU tests of the CLIP text encoder (csrc/clip.hip, live2diff_amd/clip_hip.py): every new op against torch fp32, the full-size
encode against the fp32 restatement (tests/clip_ref.py), repeatability, hipGraph replay, batch independence and the pipeline
wiring through HipPromptEncoder."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def full():
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, random_clip_text_state_dict
    sd = random_clip_text_state_dict(SD15_CLIP, 0)
    enc = HipClipTextEncoder({k: v.half() for k, v in sd.items()}, DEV)
    return sd, enc


def _prompt_ids(B, V, lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, 77), V - 1, dtype=torch.int64)
    for b in range(B):
        ids[b, 0] = V - 2
        ids[b, 1:lengths[b] + 1] = torch.randint(0, V - 2, (lengths[b],), generator=g)
    return ids


# ------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("T", [77, 80])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_clip_attn_matches_torch(T, B):
    from live2diff_amd import ops
    H, d = 12, 64
    C = H * d
    g = torch.Generator().manual_seed(T * 10 + B)
    qkv = (torch.randn(B * T, 3 * C, generator=g) * 2).half()
    out = torch.zeros(B * T, C, dtype=torch.float16, device=DEV)
    ops.run(ops.clip_attn(qkv.to(DEV), out, B=B, T=T, H=H, d=d, ldq=3 * C, ldo=C, scale=d ** -0.5))
    torch.cuda.synchronize()
    q, k, v = (qkv.float().view(B, T, 3, H, d)[:, :, j].transpose(1, 2) for j in range(3))
    mask = torch.full((T, T), float("-inf")).triu(1)
    ref = (torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, -1) @ v).transpose(1, 2).reshape(B * T, C)
    assert rel(out, ref) < 2e-3


@pytest.mark.parametrize("K,N,pro,epi", [(768, 2304, 1, 0), (768, 768, 0, 2), (768, 3072, 1, 1), (3072, 768, 0, 2),
                                         (192, 192, 1, 0), (384, 192, 0, 2), (192, 384, 1, 1)])
@pytest.mark.parametrize("M", [77, 154, 308])
def test_clip_linear_matches_torch(K, N, pro, epi, M):
    from live2diff_amd import ops
    g = torch.Generator().manual_seed(K + N + M + epi)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = torch.randn(N, generator=g) * 0.1
    if pro:
        x = torch.randn(M, K, generator=g) * 3 + 0.5
        gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        xin = torch.nn.functional.layer_norm(x, (K,), gam, bet, 1e-5).half().float()
        xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    else:
        x = torch.randn(M, K, generator=g).half()
        xin, xd, gd, bd = x.float(), x.to(DEV), None, None
    h = xin @ w.float().t() + b
    if epi == 2:
        res = torch.randn(M, N, generator=g)
        out, ref = res.clone().to(DEV), res + h
    else:
        out = torch.zeros(M, N, dtype=torch.float16, device=DEV)
        ref = h * torch.sigmoid(1.702 * h) if epi == 1 else h
    ops.run(ops.clip_linear(xd, ops.pack_clip_linear(w.to(DEV)), out, M=M, K=K, Nout=N, ldx=K, ldo=N, bias=b.to(DEV), gamma=gd,
                            beta=bd, epi=epi))
    torch.cuda.synchronize()
    assert rel(out, ref) < 2e-3


def test_clip_embed_and_ln_exact():
    from live2diff_amd import ops
    g = torch.Generator().manual_seed(1)
    V, P, C, B = 1000, 77, 768, 3
    tok, pos = (torch.randn(V, C, generator=g) * 0.02).half(), (torch.randn(P, C, generator=g) * 0.01).half()
    ids = torch.randint(0, V, (B * 77,), generator=g)
    out = torch.zeros(B * 77, C, device=DEV)
    ops.run(ops.clip_embed(ids.to(DEV), tok.to(DEV), pos.to(DEV), out, rows=B * 77, T=77, C=C, V=V, P=P))
    torch.cuda.synchronize()
    ref = tok.float()[ids] + pos.float().repeat(B, 1)
    assert torch.equal(out.cpu(), ref)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    x = torch.randn(B * 77, C, generator=g) * 5
    o = torch.zeros(B * 77, C, dtype=torch.float16, device=DEV)
    ops.run(ops.clip_ln(x.to(DEV), gam.to(DEV), bet.to(DEV), o, rows=B * 77, C=C, ldx=C, ldo=C))
    torch.cuda.synchronize()
    assert rel(o, torch.nn.functional.layer_norm(x, (C,), gam, bet, 1e-5)) < 1e-3


# ------------------------------------------------------------------------------------------------ full encoder
@pytest.mark.parametrize("clip_skip", [None, 1, 2])
def test_full_encode_matches_restatement(full, clip_skip):
    from clip_ref import clip_text_forward
    from live2diff_amd.clip_hip import SD15_CLIP
    sd, enc = full
    ids = _prompt_ids(2, SD15_CLIP.vocab_size, [9, 75], seed=clip_skip or 0)       # the second prompt: 75 tokens (the truncation limit)
    out = enc.encode(ids.to(DEV), clip_skip)
    torch.cuda.synchronize()
    ref = clip_text_forward(sd, SD15_CLIP, ids, clip_skip)
    assert out.shape == (2, 77, 768) and out.dtype == torch.float16
    assert rel(out, ref) < 2e-3


def test_outlier_channels_stay_finite_and_accurate():
    """Real CLIP residual streams carry a few channels ~100x the rest: scale those embedding channels and compare."""
    from clip_ref import clip_text_forward
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, random_clip_text_state_dict
    sd = random_clip_text_state_dict(SD15_CLIP, 4)
    for k in ("embeddings.token_embedding.weight", "embeddings.position_embedding.weight"):
        w = sd[k].clone()
        w[:, [7, 300, 581]] *= 100
        sd[k] = w.half().float()
    enc = HipClipTextEncoder({k: v.half() for k, v in sd.items()}, DEV)
    ids = _prompt_ids(1, SD15_CLIP.vocab_size, [30], seed=4)
    out = enc.encode(ids, 2)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert rel(out, clip_text_forward(sd, SD15_CLIP, ids, 2)) < 3e-3


def test_repeatable_graph_equals_direct_and_batch_independent(full):
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder
    sd, enc = full
    ids = _prompt_ids(4, SD15_CLIP.vocab_size, [5, 40, 75, 12], seed=9)
    a = enc.encode(ids.to(DEV))
    b = enc.encode(ids.to(DEV))
    direct = HipClipTextEncoder({k: v.half() for k, v in sd.items()}, DEV, use_graph=False)
    c = direct.encode(ids.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    for j in range(4):
        alone = enc.encode(ids[j:j + 1].to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(alone[0], a[j]), j


def test_cfg_matches_two_encodes(full):
    """CFG with clip_skip: the unconditional half through every layer, the conditional half with clip_skip (one plan)."""
    from live2diff_amd.clip_hip import SD15_CLIP
    sd, enc = full
    ids = _prompt_ids(2, SD15_CLIP.vocab_size, [0, 20], seed=11)
    both = enc.encode_cfg(ids, 2)
    u, c = enc.encode(ids[:1]), enc.encode(ids[1:], 2)
    torch.cuda.synchronize()
    assert torch.equal(both[0], u[0]) and torch.equal(both[1], c[0])


# ------------------------------------------------------------------------------------------------ pipeline wiring
class _StubVAE:
    dtype = torch.float16

    class config:
        scaling_factor = 0.5

    def encode(self, x):
        lat = torch.nn.functional.avg_pool2d(x.float(), 8)
        lat = torch.cat([lat, lat.mean(1, keepdim=True)], 1).to(torch.float16)
        return type("Out", (), {"latents": lat})()

    def decode(self, z, return_dict=False):
        return (torch.nn.functional.interpolate(z[:, :3].float(), scale_factor=8, mode="nearest").to(torch.float16),)


class _StubDepth:
    dtype = torch.float16

    def __call__(self, images):
        return images.float().mean(1).to(torch.float16) + 1.0


def test_pipeline_prompt_through_hip_prompt_encoder():
    from types import SimpleNamespace

    from live2diff_amd.clip_hip import HipClipTextEncoder, HipPromptEncoder, random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    from live2diff_amd.config import tiny_config
    from live2diff_amd.pipeline_stream_animation_depth import StreamAnimateDiffusionDepth
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import random_state_dict
    import dataclasses
    tok = ClipTokenizer.from_dir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_tok"))
    ccfg = dataclasses.replace(tiny_clip_config(), hidden_size=768, num_attention_heads=12, intermediate_size=768,
                               num_hidden_layers=3, vocab_size=len(tok.encoder))
    enc = HipClipTextEncoder({k: v.half() for k, v in random_clip_text_state_dict(ccfg, 5).items()}, DEV, ccfg)
    penc = HipPromptEncoder(enc, tok, default_clip_skip=1)
    cfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=768)
    H = W = 128
    sd = {k: v.to(DEV) for k, v in random_state_dict(cfg, dtype=torch.float16).items()}
    g = torch.Generator().manual_seed(5)
    warm = [torch.rand(3, H, W, generator=g) for _ in range(cfg.sink_size)]
    frames = [torch.rand(1, 3, H, W, generator=g) for _ in range(4)]

    def make():
        pipe = SimpleNamespace(device=torch.device(DEV), vae_scale_factor=8, unet=HipStreamingUNet(sd, cfg, H // 8, W // 8, 2),
                               vae=_StubVAE(), depth_model=_StubDepth(), scheduler=None)
        pipe._encode_prompt = penc._encode_prompt
        s = StreamAnimateDiffusionDepth(pipe, num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, do_add_noise=False,
                                        warmup_frames=cfg.sink_size, window_size=cfg.window_size)
        s.clip_skip = 1
        s.prepare_cache(H, W, 2)
        return s

    runs = []
    for by_prompt in (True, False):
        torch.manual_seed(0)
        s = make()
        if by_prompt:
            first = s.prepare(warm, prompt="a photo of a cat", seed=3)
        else:
            first = s.prepare(warm, prompt_embeds=enc.encode(tok(["a photo of a cat"]).to(DEV), 1), seed=3)
        s.enable_device_step()
        res = [first.clone(), s(frames[0].to(DEV)).clone()]
        if by_prompt:
            s.update_prompt("origami style, paper folding")
        else:
            s.prompt_embeds = enc.encode(tok(["origami style, paper folding"]).to(DEV), 1).repeat(s.batch_size, 1, 1)
            s.unet.invalidate_text_cache()
            s._device_step.set_prompt(s.prompt_embeds)
        res += [s(f.to(DEV)).clone() for f in frames[1:]]
        runs.append(res)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.isfinite(a).all() and torch.equal(a, b), i
    # the prompt change reaches the frame: same pipeline, same frames, without the update
    torch.manual_seed(0)
    s = make()
    s.prepare(warm, prompt="a photo of a cat", seed=3)
    s.enable_device_step()
    s(frames[0].to(DEV))
    kept = [s(f.to(DEV)).clone() for f in frames[1:]]
    assert not torch.equal(kept[-1], runs[0][-1])
