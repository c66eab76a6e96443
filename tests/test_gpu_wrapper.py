"""-m gpu: `StreamAnimateDiffusionDepthWrapper` end to end on native components with synthetic weights -- uint8 frames in, uint8
frames out -- against the same stack composed by hand (ingest -> pipeline -> egress), in `__call__` and in push / pop mode, and
one full-size construction."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
PROMPT = "a cat, paper folding"


def u8_frames(n, Hs, Ws, seed, bright=()):
    g = torch.Generator().manual_seed(seed)
    f = torch.randint(0, 256, (n, Hs, Ws, 3), dtype=torch.uint8, generator=g)
    for i in bright:
        f[i] = 128 + f[i] // 2                                   # every pixel >= 128: non-negative everywhere once in [-1, 1]
    return f.numpy()


class Parts:
    """state dicts made once; every stack builds its own objects (own plans, own static buffers) from them"""

    def __init__(self, ucfg, clip_cfg, H, W, N):
        from live2diff_amd.clip_hip import random_clip_text_state_dict
        from live2diff_amd.clip_tokenizer import ClipTokenizer
        from live2diff_amd.midas_hip import random_midas_state_dict
        from live2diff_amd.vae_hip import random_taesd_state_dict
        from live2diff_amd.weights import device_random_state_dict
        self.ucfg, self.clip_cfg, self.H, self.W, self.N = ucfg, clip_cfg, H, W, N
        self.unet_sd = device_random_state_dict(ucfg, DEV)
        self.vae_sd = random_taesd_state_dict(device=DEV)
        self.midas_sd = random_midas_state_dict(device=DEV)
        self.clip_sd = random_clip_text_state_dict(clip_cfg, 3)
        self.tok = ClipTokenizer.from_dir(os.path.join(HERE, "golden", "clip_tok"))
        self.unet0 = None

    def pipe(self):
        from live2diff_amd.clip_hip import HipClipTextEncoder, HipPromptEncoder
        from live2diff_amd.midas_hip import HipMidas
        from live2diff_amd.unet_hip import HipStreamingUNet
        from live2diff_amd.vae_hip import HipTinyVAE
        # (later stacks share the first one's packed weights: read-only, and the packing pass runs once)
        unet = HipStreamingUNet(self.unet0 or self.unet_sd, self.ucfg, self.H // 8, self.W // 8, self.N, device=DEV)
        self.unet0 = self.unet0 or unet
        penc = HipPromptEncoder(HipClipTextEncoder(self.clip_sd, DEV, self.clip_cfg), self.tok, default_clip_skip=1)
        return SimpleNamespace(device=torch.device(DEV), vae_scale_factor=8, unet=unet, vae=HipTinyVAE(self.vae_sd, device=DEV),
                               depth_model=HipMidas(self.midas_sd, device=DEV), scheduler=None, _encode_prompt=penc._encode_prompt)


def test_wrapper_u8_equals_hand_composition_and_push_pop():
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.frame_io import HipFrameIO, _PassThrough, ingest_ref
    from live2diff_amd.pipeline_stream_animation_depth import StreamAnimateDiffusionDepth
    from live2diff_amd.stream_step_hip import HipStreamStep
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(6, 96, 128, seed=2, bright=(3,))
    assert frames[3].min() >= 128 and ingest_ref(frames[3], H, W).min() >= 0        # the frame a range probe would map twice
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(**more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        warm_out = w.prepare(warm, PROMPT)
        assert isinstance(w.stream._device_step, HipStreamStep)
        return w, warm_out

    w, warm_out = wrapper()
    assert warm_out.shape == (8, H, W, 3) and 0 <= float(warm_out.min()) and float(warm_out.max()) <= 1
    got = [w(f) for f in frames]
    assert all(o.dtype == np.uint8 and o.shape == (H, W, 3) for o in got)
    assert not np.array_equal(got[1], got[2]) and len({o.tobytes() for o in got}) == 6 and got[0].std() > 0
    assert len(w.stream.inference_time_list) == 6

    # the same stack by hand: ingest -> pipeline (pass-through processor: the normalised frame is not probed) -> egress
    torch.manual_seed(0)
    s = StreamAnimateDiffusionDepth(parts.pipe(), **kw)
    s.prepare_cache(H, W, 2)
    s.image_processor = _PassThrough()
    io = HipFrameIO(H, W, device=DEV)
    s.prepare(io.ingest(warm), prompt=PROMPT, seed=SEED)
    s.enable_device_step(seed=SEED)
    for i, f in enumerate(frames):
        want = io.egress(s(io.ingest(f))[0]).copy()
        n = int((want != got[i]).sum())
        print(f"frame {i}: {n} differing bytes")
        assert n == 0, f"frame {i}{' (the bright one)' if i == 3 else ''}"

    w.output_type = "pil"                        # a seventh frame as PIL: Image.fromarray of the u8 result
    w2, _ = wrapper()
    for f in frames:
        w2(f)
    pil, u8 = w(frames[0]), w2(frames[0])
    assert pil.size == (W, H) and pil.mode == "RGB" and np.array_equal(np.array(pil), u8)

    # push / pop: frame t + 1 is pushed before frame t is popped
    wp, _ = wrapper(frame_pipelining=True)
    out = []
    wp.push(frames[0])
    for i in range(len(frames)):
        if i + 1 < len(frames):
            wp.push(frames[i + 1])
        out.append(wp.pop())
    torch.cuda.synchronize()
    for i in range(len(frames)):
        assert np.array_equal(out[i], got[i]), f"push / pop frame {i} differs from __call__"


def test_wrapper_inputs_pil_path_and_float(tmp_path):
    """a PIL image / a file path is resized on the host and takes the identity ingest; a float [3,H,W] tensor in [0, 1] takes the
    reference's path; "pt" / "np" / "latent" keep the reference's shapes"""
    from PIL import Image

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=8, window_size=16, seed=SEED, device=DEV)
    src = u8_frames(1, 96, 128, seed=4)[0]
    pil = Image.fromarray(src)
    pil.save(tmp_path / "f.png")
    resized = np.array(pil.resize((W, H)))
    outs = []
    for inp in (pil, str(tmp_path / "f.png"), resized, torch.from_numpy(resized).to(DEV)):
        torch.manual_seed(0)
        w = Wrapper.from_components(parts.pipe(), output_type="u8", **kw)
        w.prepare(torch.rand(8, 3, H, W, generator=torch.Generator().manual_seed(3)), PROMPT)      # float warm-up frames in [0, 1]
        outs.append(w(inp))
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    x = torch.from_numpy(resized).permute(2, 0, 1).float() / 255.0
    for ot, check in (("pt", lambda o: o.dtype == torch.float16 and o.shape == (3, H, W) and o.device.type == "cpu"),
                      ("np", lambda o: o.dtype == np.float32 and o.shape == (H, W, 3) and 0 <= o.min() and o.max() <= 1),
                      ("latent", lambda o: o.shape == (3, H, W) and o.device.type == "cpu")):
        w.output_type = ot
        assert check(w(x)), ot
    w.output_type = "u8"
    o = w(x)
    assert o.dtype == np.uint8 and o.shape == (H, W, 3)


def test_full_size_construction_runs():
    from live2diff_amd.clip_hip import SD15_CLIP
    from live2diff_amd.config import sd15_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ucfg = sd15_config()
    parts = Parts(ucfg, SD15_CLIP, 512, 512, 4)
    w = Wrapper.from_components(parts.pipe(), num_inference_steps=50, t_index_list=[25, 31, 37, 43], width=512, height=512,
                                output_type="u8", seed=SEED, device=DEV, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)
    assert w.batch_size == 4
    w.prepare(u8_frames(8, 720, 1280, seed=5), PROMPT)
    outs = [w(f) for f in u8_frames(3, 720, 1280, seed=6)]
    for o in outs:
        assert o.shape == (512, 512, 3) and o.dtype == np.uint8 and o.min() != o.max()
    assert len(w.stream.inference_time_list) == 3
    print("inference_time_list (s):", [round(t, 4) for t in w.stream.inference_time_list])
