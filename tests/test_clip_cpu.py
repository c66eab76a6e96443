"""CPU tests of the CLIP text encoder: the fp32 restatement against transformers (clip_hf.npz), the tokenizer against
transformers' CLIPTokenizer (golden/clip_tok), text-encoder conversion / LoRA merge against the reference's functions
(clip_convert.npz), clip_skip layer counting, the static plan under dry run and HipPromptEncoder's return convention."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def hf():
    return np.load(os.path.join(GOLD, "clip_hf.npz"))


@pytest.fixture
def dry():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_restatement_matches_transformers_tiny(hf):
    from clip_ref import clip_text_forward
    from live2diff_amd.clip_hip import random_clip_text_state_dict, tiny_clip_config
    cfg = tiny_clip_config()
    sd, ids = random_clip_text_state_dict(cfg, 1), torch.from_numpy(hf["tiny_ids"])
    for k in (None, 1):
        assert rel(clip_text_forward(sd, cfg, ids, k), hf["tiny_" + ("none" if k is None else str(k))]) < 1e-5


def test_restatement_matches_transformers_full(hf):
    from clip_ref import clip_text_forward
    from live2diff_amd.clip_hip import SD15_CLIP, random_clip_text_state_dict
    sd, ids = random_clip_text_state_dict(SD15_CLIP, 0), torch.from_numpy(hf["full_ids"])
    out, hidden = clip_text_forward(sd, SD15_CLIP, ids, None, all_hidden=True)
    sel = torch.from_numpy(hf["full_sel"])
    lnf = lambda x: torch.nn.functional.layer_norm(x, (768,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], 1e-5)
    for k in (None, 1, 2):
        o = out if k is None else lnf(hidden[-(k + 1)])
        tag = "none" if k is None else str(k)
        assert rel(o.reshape(-1)[sel], hf[f"full_{tag}_vals"]) < 1e-5
        assert rel(o.norm(dim=-1), hf[f"full_{tag}_rownorm"]) < 1e-5


@pytest.mark.parametrize("use_regex", [True, False])
def test_tokenizer_matches_clip_tokenizer(use_regex):
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    if use_regex:
        pytest.importorskip("regex")
    d = os.path.join(GOLD, "clip_tok")
    tok = ClipTokenizer.from_dir(d, use_regex=use_regex)
    fx = json.load(open(os.path.join(d, "ids.json"), encoding="utf-8"))
    assert len(fx["prompts"]) == 20
    for p, ids in zip(fx["prompts"], fx["ids"]):
        assert tok.encode(p) == ids, p
    assert tok("")[0].tolist()[:2] == [tok.bos_id, tok.eos_id] and tok("").shape == (1, 77)


def test_tokenizer_fallback_split_equals_regex():
    regex = pytest.importorskip("regex")
    from live2diff_amd.clip_tokenizer import SPLIT_PATTERN, split_stdlib
    pat = regex.compile(SPLIT_PATTERN)
    for t in ["it's a 'test' y'all'd", "<|endoftext|>x!<|startoftext|>", "a1b22c ..--!! 'll'", "Ünïcödé ½ ² ٣ 漢字", "'re're'"]:
        assert split_stdlib(t) == pat.findall(t), t


def test_convert_ldm_clip_checkpoint_matches_reference():
    from live2diff_amd.convert import convert_ldm_clip_checkpoint
    g = np.load(os.path.join(GOLD, "clip_convert.npz"))
    ckpt = {k: torch.zeros(1) for k in g["ldm_keys"]}
    assert sorted(convert_ldm_clip_checkpoint(ckpt)) == list(g["conv_keys"])
    with pytest.raises(KeyError):
        convert_ldm_clip_checkpoint({"model.diffusion_model.conv_in.weight": torch.zeros(1)})


def test_merge_text_lora_matches_reference():
    from live2diff_amd.clip_hip import random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.convert import merge_text_lora
    g = np.load(os.path.join(GOLD, "clip_convert.npz"))
    lora = {k[len("lora."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("lora.")}
    for prefixed in (False, True):
        sd = random_clip_text_state_dict(tiny_clip_config(), 2)
        if prefixed:
            sd = {"text_model." + k: v for k, v in sd.items()}
        touched = merge_text_lora(sd, lora, 0.7)
        merged = [k[len("merged_idx."):] for k in g.files if k.startswith("merged_idx.")]
        assert sorted(t[len("text_model."):] if prefixed else t for t in touched) == sorted(merged)
        for k in merged:
            v = sd[("text_model." if prefixed else "") + k].reshape(-1)[torch.from_numpy(g["merged_idx." + k])]
            assert torch.allclose(v, torch.from_numpy(g["merged_val." + k]), rtol=0, atol=1e-6), k
    with pytest.raises(KeyError):
        merge_text_lora(random_clip_text_state_dict(tiny_clip_config(), 2),
                        {"lora_te_text_model_encoder_layers_9_mlp_fc1.lora_down.weight": torch.zeros(4, 192),
                         "lora_te_text_model_encoder_layers_9_mlp_fc1.lora_up.weight": torch.zeros(384, 4)}, 1.0)


def test_build_text_encoder_state_dict_order():
    """DreamBooth text encoder over the base, then each LoRA: the LoRA lands on the DreamBooth weights."""
    from live2diff_amd.clip_hip import random_clip_text_state_dict, tiny_clip_config
    from live2diff_amd.convert import LDM_CLIP_PREFIX, build_text_encoder_state_dict
    cfg = tiny_clip_config()
    base, db = random_clip_text_state_dict(cfg, 2), random_clip_text_state_dict(cfg, 3)
    ckpt = {LDM_CLIP_PREFIX + "text_model." + k: v for k, v in db.items()}
    k = "encoder.layers.0.mlp.fc1.weight"
    stem = "lora_te_text_model_encoder_layers_0_mlp_fc1"
    up, down = torch.ones(384, 1), torch.full((1, 192), 0.5)
    out = build_text_encoder_state_dict(base, ckpt, [({stem + ".lora_up.weight": up, stem + ".lora_down.weight": down}, 0.2)])
    assert torch.equal(out["final_layer_norm.weight"], db["final_layer_norm.weight"])
    assert torch.allclose(out[k], db[k] + 0.1)
    with pytest.raises(KeyError):
        build_text_encoder_state_dict(base, {"model.diffusion_model.x": torch.zeros(1)})


def test_clip_skip_layer_count_and_dry_run_plan(dry):
    from live2diff_amd import _lib
    from live2diff_amd.clip_hip import SD15_CLIP, HipClipTextEncoder, clip_launches, random_clip_text_state_dict
    sd = {k: v.half() for k, v in random_clip_text_state_dict(SD15_CLIP, 0).items()}
    sd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    enc = HipClipTextEncoder({("text_model." + k if "encoder." in k else k): v for k, v in sd.items()}, "cpu")
    assert enc.layer_weight_bytes > 170e6
    for B in (1, 2, 4):
        for k in (None, 1, 2):
            st = enc.plan(B, k)
            n = len(st.pl)
            assert n == clip_launches(SD15_CLIP, k) == 5 * (12 - (k or 0)) + 2 <= 62
            kinds = [op.kind for op in st.pl._ops]
            assert kinds[0] == _lib.OP_CLIP_EMBED and kinds[-1] == _lib.OP_CLIP_LN
            assert kinds.count(_lib.OP_CLIP_ATTN) == 12 - (k or 0) and kinds.count(_lib.OP_CLIP_LINEAR) == 4 * (12 - (k or 0))
            st.pl.run()                                            # every op validates
        st = enc.plan(2, None, early=(2, 1))
        assert len(st.pl) == 63
        st.pl.run()
    with pytest.raises(ValueError):
        enc.plan(1, 12)
    with pytest.raises(KeyError):
        HipClipTextEncoder({k: v for k, v in sd.items() if "fc2" not in k}, "cpu")


def test_dry_run_rejects_bad_shapes(dry):
    from live2diff_amd import _lib, ops
    x = torch.zeros(77, 700, dtype=torch.float16)
    w = torch.zeros(768 * 700, dtype=torch.float16)
    out = torch.zeros(77, 768, dtype=torch.float16)
    with pytest.raises(_lib.L2DError):
        ops.run(ops.clip_linear(x, w, out, M=77, K=700, Nout=768, ldx=700, ldo=768, NW=1, MT=3))
    qkv = torch.zeros(200, 3 * 768, dtype=torch.float16)
    with pytest.raises(_lib.L2DError):
        ops.run(ops.clip_attn(qkv, out, B=1, T=200, H=12, d=64, ldq=3 * 768, ldo=768, scale=0.125))


class _FakeEncoder:
    def __init__(self):
        self.calls = []

    def encode(self, ids, clip_skip=None):
        self.calls.append(("encode", ids.shape[0], clip_skip))
        return ids[:, :, None].float().expand(-1, -1, 4).half() + (clip_skip or 0)

    def encode_cfg(self, ids, clip_skip=None):
        self.calls.append(("cfg", ids.shape[0], clip_skip))
        return ids[:, :, None].float().expand(-1, -1, 4).half()


def test_prompt_encoder_return_convention_and_default_clip_skip():
    from live2diff_amd.clip_hip import HipPromptEncoder
    from live2diff_amd.clip_tokenizer import ClipTokenizer
    tok = ClipTokenizer.from_dir(os.path.join(GOLD, "clip_tok"))
    fe = _FakeEncoder()
    pe = HipPromptEncoder(fe, tok, default_clip_skip=2)
    e = pe._encode_prompt(prompt="a cat", device="cpu", num_videos_per_prompt=1, do_classifier_free_guidance=False)
    assert e.shape == (1, 77, 4) and e[0].shape == (77, 4) and fe.calls[-1] == ("encode", 1, 2)
    pe._encode_prompt(prompt="a cat", device="cpu", num_videos_per_prompt=1, do_classifier_free_guidance=False, negative_prompt=None,
                      clip_skip=None)
    assert fe.calls[-1] == ("encode", 1, None)                     # an explicit None is honoured
    e = pe._encode_prompt(prompt="a cat", device="cpu", num_videos_per_prompt=3, do_classifier_free_guidance=True,
                          negative_prompt="blurry", clip_skip=1)
    assert e.shape == (6, 77, 4) and fe.calls[-1] == ("cfg", 2, 1)
    assert torch.equal(e[0, :, 0].long(), torch.tensor(tok.encode("blurry"))) and torch.equal(e[3, :, 0].long(), torch.tensor(tok.encode("a cat")))
    e = pe._encode_prompt(prompt=["a", "b"], device="cpu", num_videos_per_prompt=1, do_classifier_free_guidance=True)
    assert e.shape == (4, 77, 4) and torch.equal(e[0, :, 0].long(), torch.tensor(tok.encode("")))
    with pytest.raises(TypeError):
        pe._encode_prompt(prompt="a", device="cpu", num_videos_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=["x"])
