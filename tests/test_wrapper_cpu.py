"""CPU tests (-m "not gpu") of live2diff_amd/wrapper.py: the config loader, the engine prefix, the assembly from model files
(dry-run: plans are built and validated, nothing is launched), keyword refusals, `postprocess_image` against the reference's
own outputs (tests/golden/frame_io.npz) and `__call__` on the mock components of tests/pipeline_mocks.py."""
import json
import os

import numpy as np
import pytest
import torch

from live2diff_amd import wrapper as WR
from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "configs")


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


# ----------------------------------------------------------------------------- config
def test_load_config_merges_base_recursively(tmp_path):
    (tmp_path / "base.yaml").write_text(
        "pretrained_model_path: ./sd\nunet_additional_kwargs:\n  cond_mapping: true\n  motion_module_kwargs:\n"
        "    temporal_position_encoding_max_len: 24\n    attention_kwargs:\n      window_size: 16\n      sink_size: 8\n"
        "third_party_dict:\n  dreambooth: base.safetensors\n")
    (tmp_path / "child.yaml").write_text(
        f"base: {tmp_path / 'base.yaml'}\nthird_party_dict:\n  clip_skip: 2\nunet_additional_kwargs:\n  motion_module_kwargs:\n"
        "    attention_kwargs:\n      window_size: 24\nt_index_list: [30, 40]\n")
    cfg = WR.load_config(tmp_path / "child.yaml")
    assert "base" not in cfg and cfg["pretrained_model_path"] == "./sd" and cfg["t_index_list"] == [30, 40]
    assert cfg["third_party_dict"] == {"dreambooth": "base.safetensors", "clip_skip": 2}
    assert cfg["unet_additional_kwargs"]["cond_mapping"] is True
    assert WR.stream_sizes(cfg) == (24, 8, 24)
    (tmp_path / "rel.yaml").write_text("base: ./base.yaml\nprompt: x\n")           # found beside the config, from any cwd
    assert WR.load_config(tmp_path / "rel.yaml")["pretrained_model_path"] == "./sd"
    (tmp_path / "bad.yaml").write_text("base: ./nowhere.yaml\n")
    with pytest.raises(FileNotFoundError, match="base"):
        WR.load_config(tmp_path / "bad.yaml")


def test_reference_configs_load():
    cfg = WR.load_config(os.path.join(CONFIGS, "toonyou.yaml"))
    assert WR.stream_sizes(cfg)[:2] == (16, 8)
    assert cfg["t_index_list"] == [25, 31, 37, 43] and cfg["third_party_dict"]["clip_skip"] == 2
    assert cfg["num_inference_steps"] == 50 and cfg["noise_scheduler_kwargs"]["beta_schedule"] == "linear"
    assert cfg["motion_module_path"].endswith("live2diff.ckpt") and cfg["unet_additional_kwargs"]["cond_mapping"] is True


def test_get_model_prefix_is_the_references_string():
    p = os.path.join(CONFIGS, "toonyou.yaml")
    assert Wrapper.get_model_prefix(p, "lcm", True, 4, 512, 512) == "toonyou_beta6--lcm--step4--tiny_vae-True--h-512--w-512"
    s = Wrapper.get_model_prefix(p, "lcm", True, 4, 512, 512, lora_dict={"a/b.safetensors": 0.5})
    assert s == "toonyou_beta6--lcm--step4--b-0.5--tiny_vae-True--h-512--w-512"
    assert Wrapper.get_model_prefix(p, "lcm", False, 2, 512, 768, dreambooth="x/y.ckpt").startswith("y--lcm--step2--tiny_vae-False--h-512--w-768")
    assert Wrapper.get_model_prefix(os.path.join(CONFIGS, "base_config.yaml"), "lcm", True, 4, 64, 64).startswith("sd15--")


# ----------------------------------------------------------------------------- keywords
@pytest.mark.parametrize("kw", [dict(acceleration="tensorrt"), dict(acceleration="none"), dict(cfg_type="self"),
                                dict(use_denoising_batch=False), dict(frame_buffer_size=2), dict(device_ids=[0, 1]),
                                dict(few_step_model_type="turbo"), dict(opt_unet=True)])
def test_unsupported_keywords_raise_naming_themselves(kw):
    name = next(iter(kw))
    args = dict(config_path=os.path.join(CONFIGS, "toonyou.yaml"), few_step_model_type="lcm", num_inference_steps=50)
    with pytest.raises(ValueError, match=name):
        Wrapper(**{**args, **kw})
    with pytest.raises(ValueError, match=name):
        Wrapper.from_components(object(), num_inference_steps=50, t_index_list=[1], **kw)


# ----------------------------------------------------------------------------- postprocess against the reference's outputs
def test_postprocess_image_matches_reference_fixture(golden):
    g = golden("frame_io")
    w = Wrapper.__new__(Wrapper)
    w.io, w.frame_buffer_size = None, 1
    x = torch.from_numpy(g["x"])
    for b in range(x.shape[0]):
        xb = x[b:b + 1]
        pt = w.postprocess_image(xb, "pt")
        assert pt.dtype == torch.float16 and pt.device.type == "cpu" and np.array_equal(pt.numpy(), g["pt"][b])
        npo = w.postprocess_image(xb, "np")
        assert npo.dtype == np.float32 and np.array_equal(npo, g["np"][b])
        assert np.array_equal(np.array(w.postprocess_image(xb, "pil")), g["pil"][b])
        u8 = w.postprocess_image(xb, "u8")
        assert u8.dtype == np.uint8 and np.array_equal(u8, g["pil"][b])
        assert torch.equal(w.postprocess_image(xb, "latent"), xb[0])
    with pytest.raises(ValueError):
        w.postprocess_image(g["x"], "pil")


# ----------------------------------------------------------------------------- __call__ on the mock components
def test_call_on_mock_components_is_postprocess_of_stream(monkeypatch):
    import pipeline_mocks as M

    import live2diff_amd.pipeline_stream_animation_depth as P
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)

    def build(as_wrapper):
        pipe = M.MockPipe()
        pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), M.MockDepth()
        pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
        kw = dict(num_inference_steps=50, t_index_list=[10, 20, 30], width=M.W, height=M.H)
        if as_wrapper:
            w = Wrapper.from_components(pipe, output_type="pt", dtype=torch.float32, device="cpu", seed=2, **kw)
            s = w.stream
        else:
            w = None
            s = P.StreamAnimateDiffusionDepth(pipe, torch_dtype=torch.float32, **kw)
            s.prepare_cache(M.H, M.W, 3)
        s.scheduler = M.MockScheduler()
        s.timesteps = s.scheduler.timesteps
        s.image_processor = M.MockImageProcessor()
        s.unet_warmup = M.MockWarmupUNet()
        return w, s, pipe

    w, _, wpipe = build(True)
    assert (w.batch_size, w.width, w.height, w.output_type, w.frame_buffer_size, w.device, w.dtype) == (3, M.W, M.H, "pt", 1, "cpu", torch.float32)
    _, s, _ = build(False)
    frames = list(M.frames(4, seed=11))
    # (the host path draws its re-noising from the global generator: the two stacks run one after the other from the same seed)
    torch.manual_seed(123)
    warm_w = w.prepare(M.frames(8, seed=7), "a prompt")
    assert getattr(w.stream, "_device_step", None) is None           # mock UNet: the host path stays
    got = [w(img, prompt="another prompt" if i == 2 else None) for i, img in enumerate(frames)]
    w.output_type = "u8"
    got_u8 = w(M.frames(1, seed=12)[0])
    torch.manual_seed(123)
    warm_s = s.prepare(M.frames(8, seed=7), "a prompt", seed=2)
    assert warm_w.shape == (8, M.H, M.W, 3) and torch.equal(warm_w, (warm_s.permute(0, 2, 3, 1).clip(-1, 1) + 1) / 2)
    for i, img in enumerate(frames):
        if i == 2:
            s.update_prompt("another prompt")
        want = (s(img) / 2 + 0.5).clamp(0, 1)[0].cpu()
        assert got[i].shape == (3, M.H, M.W) and torch.equal(got[i], want), i
    assert [c[0] for c in wpipe.calls] == ["a prompt", "another prompt"]
    from live2diff_amd.frame_io import egress_ref
    assert got_u8.dtype == np.uint8 and np.array_equal(got_u8, egress_ref(s(M.frames(1, seed=12)[0]))[0].numpy())


# ----------------------------------------------------------------------------- assembly from files (dry-run)
def _zoo(tmp_path, with_motion=True):
    """a model zoo at test scale in the layout the reference's configs name"""
    from safetensors.torch import save_file

    from live2diff_amd.clip_hip import random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.vae_hip import random_taesd_state_dict
    from live2diff_amd.weights import random_state_dict
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    sd = random_state_dict(ucfg, dtype=torch.float16)
    is_motion = lambda k: ".motion_modules." in k or k.startswith("flow_conv_in.")
    model = tmp_path / "models" / "sd"
    for sub in ("unet", "text_encoder", "tokenizer"):
        (model / sub).mkdir(parents=True)
    save_file({k: v for k, v in sd.items() if not is_motion(k)}, str(model / "unet" / "diffusion_pytorch_model.safetensors"))
    (model / "unet" / "config.json").write_text(json.dumps(dict(block_out_channels=[64, 128, 256, 256], cross_attention_dim=ccfg.hidden_size)))
    save_file({k: v.to(torch.float16) for k, v in random_clip_text_state_dict(ccfg, 1).items()}, str(model / "text_encoder" / "model.safetensors"))
    (model / "text_encoder" / "config.json").write_text(json.dumps(dict(
        vocab_size=ccfg.vocab_size, hidden_size=ccfg.hidden_size, intermediate_size=ccfg.intermediate_size, num_hidden_layers=ccfg.num_hidden_layers,
        num_attention_heads=ccfg.num_attention_heads, max_position_embeddings=ccfg.max_position_embeddings, hidden_act="quick_gelu")))
    for name in ("vocab.json", "merges.txt"):
        (model / "tokenizer" / name).write_bytes(open(os.path.join(HERE, "golden", "clip_tok", name), "rb").read())
    motion = {"module." + k: v + 0.25 for k, v in sd.items() if is_motion(k)}
    if with_motion:
        torch.save({"global_step": 7, "state_dict": motion}, str(tmp_path / "models" / "live2diff.ckpt"))
    g = torch.Generator().manual_seed(5)
    tgt = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    c = sd[tgt + ".weight"].shape[0]
    lcm = {f"lora_unet_{tgt.replace('.', '_')}.lora_down.weight": torch.randn(4, c, generator=g).half(),
           f"lora_unet_{tgt.replace('.', '_')}.lora_up.weight": torch.randn(c, 4, generator=g).half(),
           f"lora_unet_{tgt.replace('.', '_')}.alpha": torch.tensor(2.0)}
    save_file(lcm, str(tmp_path / "models" / "lcm_lora.safetensors"))
    save_file(random_taesd_state_dict(width=16), str(tmp_path / "models" / "taesd.safetensors"))
    cfg = dict(pretrained_model_path=str(model), motion_module_path=str(tmp_path / "models" / "live2diff.ckpt"),
               depth_model_path=str(tmp_path / "models" / "dpt_hybrid_384.pt"), few_step_lora_path=str(tmp_path / "models" / "lcm_lora.safetensors"),
               taesd_path=str(tmp_path / "models" / "taesd.safetensors"),
               unet_additional_kwargs=dict(motion_module_kwargs=dict(temporal_position_encoding_max_len=24,
                                                                     attention_kwargs=dict(window_size=16, sink_size=8))),
               noise_scheduler_kwargs=dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                                           steps_offset=1, clip_sample=False),
               third_party_dict=dict(clip_skip=2), t_index_list=[30, 40], num_inference_steps=50)
    import yaml
    (tmp_path / "style.yaml").write_text(yaml.safe_dump(cfg))
    return str(tmp_path / "style.yaml"), ucfg, sd, motion, lcm


def test_assembly_from_files(dry_run, tmp_path, monkeypatch):
    from live2diff_amd import convert
    from live2diff_amd import unet_hip
    from live2diff_amd.clip_hip import HipClipTextEncoder
    from live2diff_amd.midas_hip import HipMidas, random_midas_state_dict
    from live2diff_amd.vae_hip import HipTinyVAE
    path, ucfg, sd, motion, lcm = _zoo(tmp_path)
    monkeypatch.setattr(WR, "load_depth_state_dict", lambda p: random_midas_state_dict())
    seen = []
    real_init = unet_hip.HipStreamingUNet.__init__

    def spy(self, state_dict, *a, **k):
        seen.append(state_dict)
        real_init(self, state_dict, *a, **k)

    monkeypatch.setattr(unet_hip.HipStreamingUNet, "__init__", spy)
    engines = tmp_path / "engines"
    kw = dict(config_path=path, few_step_model_type="lcm", num_inference_steps=50, width=128, height=128, device="cpu",
              engine_dir=engines, output_type="u8")
    w = Wrapper(**kw)
    assert w.batch_size == 2 and w.stream.t_list == [30, 40] and w.stream.clip_skip == 2
    assert (w.stream.warmup_frames, w.stream.window_size) == (8, 16) and w.io is None
    assert isinstance(w.stream.unet, unet_hip.HipStreamingUNet) and isinstance(w.stream.vae, HipTinyVAE) and w.stream.vae.width == 16
    assert isinstance(w.stream.depth_detector, HipMidas) and isinstance(w.stream.text_encoder, HipClipTextEncoder)
    assert len(w.stream.kv_cache_list) == len(w.stream.unet.mm_layout)
    # the state dict handed to the UNet is build_state_dict on the same files, by hand
    base = {k: (v if k not in {m[len("module."):] for m in motion} else torch.zeros_like(v)) for k, v in sd.items()}
    want = convert.build_state_dict(base, ucfg, motion_ckpt={"state_dict": motion}, few_step_lora=lcm)
    got = seen[0]
    assert isinstance(got, dict) and set(got) == set(want)
    assert all(torch.equal(got[k], want[k]) for k in want)
    tgt = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight"
    assert not torch.equal(got[tgt], sd[tgt])                                     # the few-step LoRA was merged
    mk = next(k for k in sd if ".motion_modules." in k)
    assert torch.equal(got[mk], sd[mk] + 0.25)                                    # ... and the motion checkpoint
    cache = engines / (unet_hip.HipStreamingUNet.packed_cache_name("sd15", "lcm", 16, {}, 16, 16, 2) + ".safetensors")
    assert cache.is_file()
    w2 = Wrapper(**kw)
    assert len(seen) == 2 and str(seen[1]) == str(cache)                          # second construction: the packed file
    assert all(torch.equal(w2.stream.unet.W[k].cpu(), w.stream.unet.W[k].cpu()) for k in w.stream.unet.W)


def test_missing_files_name_their_config_key(dry_run, tmp_path, monkeypatch):
    from live2diff_amd.midas_hip import random_midas_state_dict
    path, *_ = _zoo(tmp_path, with_motion=False)
    monkeypatch.setattr(WR, "load_depth_state_dict", lambda p: random_midas_state_dict())
    kw = dict(config_path=path, few_step_model_type="lcm", num_inference_steps=50, width=128, height=128, device="cpu",
              engine_dir=None)
    with pytest.raises(FileNotFoundError, match="motion_module_path.*live2diff.ckpt"):
        Wrapper(**kw)
    with pytest.raises(FileNotFoundError, match="config_path"):
        Wrapper(**{**kw, "config_path": str(tmp_path / "nope.yaml")})
    torch.save({}, str(tmp_path / "models" / "live2diff.ckpt"))
    with pytest.raises(FileNotFoundError, match="third_party_dict.dreambooth"):
        Wrapper(**{**kw, "dreambooth_path": str(tmp_path / "style.safetensors")})


def test_surviving_placeholder_raises(dry_run, tmp_path, monkeypatch):
    """a parameter that neither the 2D UNet nor the motion checkpoint provides is an error, not a silent zero / random init"""
    from live2diff_amd.midas_hip import random_midas_state_dict
    path, ucfg, sd, motion, _ = _zoo(tmp_path)
    drop = next(k for k in motion if ".motion_modules." in k)
    torch.save({"state_dict": {k: v for k, v in motion.items() if k != drop}}, str(tmp_path / "models" / "live2diff.ckpt"))
    monkeypatch.setattr(WR, "load_depth_state_dict", lambda p: random_midas_state_dict())
    with pytest.raises(KeyError, match=drop[len("module."):].replace(".", r"\.")):
        Wrapper(config_path=path, few_step_model_type="lcm", num_inference_steps=50, width=128, height=128, device="cpu", engine_dir=None)


def test_inflate_2d_unet_shapes_and_placeholders():
    from live2diff_amd import convert
    from live2diff_amd.config import tiny_config
    from live2diff_amd.weights import random_state_dict, unet_param_spec
    cfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=64)
    sd = random_state_dict(cfg, dtype=torch.float16)
    two_d = {k: v for k, v in sd.items() if ".motion_modules." not in k and not k.startswith("flow_conv_in.")}
    out = convert.inflate_2d_unet(two_d, cfg)
    assert list(out) == list(unet_param_spec(cfg))
    for k, shp in unet_param_spec(cfg).items():
        assert tuple(out[k].shape) == tuple(shp)
        assert torch.equal(out[k], sd[k]) if k in two_d else not out[k].any()
    bad = dict(two_d)
    bad["conv_in.weight"] = torch.zeros(64, 9, 3, 3)
    with pytest.raises(ValueError, match="conv_in.weight"):
        convert.inflate_2d_unet(bad, cfg)


def test_stream_frames_tool_reads_and_aligns(tmp_path):
    """tools/stream_frames.py: an .npy stack or a folder of images in; outputs aligned by batch_size - 1 (reference test.py:169-174)"""
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("stream_frames", os.path.join(os.path.dirname(HERE), "tools", "stream_frames.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    stack = np.random.default_rng(0).integers(0, 256, (5, 12, 16, 3), dtype=np.uint8)
    np.save(tmp_path / "f.npy", stack)
    assert np.array_equal(tool.read_frames(str(tmp_path / "f.npy")), stack)
    (tmp_path / "dir").mkdir()
    for i, f in enumerate(stack):
        Image.fromarray(f).save(tmp_path / "dir" / f"{i:03d}.png")
    assert np.array_equal(tool.read_frames(str(tmp_path / "dir")), stack)
    np.save(tmp_path / "bad.npy", stack.astype(np.float32))
    with pytest.raises(ValueError):
        tool.read_frames(str(tmp_path / "bad.npy"))
    assert tool.align(list(range(10)), 4) == list(range(3, 10)) and tool.align([1, 2], 1) == [1, 2]
