#!/usr/bin/env python
"""Golden fixtures of the CLIP text encoder, generated in the build container with transformers and the
reference checkout; never on the GPU box.

  clip_hf.npz          transformers' CLIPTextModel (attn_implementation="eager", fp32) loaded with random_clip_text_state_dict:
                       SD-1.x size (seed 0): two prompts' ids and, for clip_skip None / 1 / 2, 4096 sampled output values plus the
                       norm of every token row; tiny config (seed 1): full outputs for clip_skip None / 1
  clip_tok/            a synthetic vocab.json + merges.txt (byte alphabet + the 119 merges BPE learns from a small text) and ids.json: the
                       ids transformers' CLIPTokenizer gives for 20 prompts (padding="max_length", max_length=77, truncation)
  clip_convert.npz     the reference's convert_ldm_clip_checkpoint (convert_from_ckpt.py:591-599) key list on a synthetic LDM
                       checkpoint, and its convert_lora_model_level (convert_lora_safetensor_to_diffusers.py:22-101) merging a
                       kohya text LoRA (rank 4, q / out_proj / fc1 / fc2 targets) into a tiny CLIPTextModel at alpha = 0.7
                       (2048 sampled entries of every merged tensor)

Run here only:  python tests/golden/gen_golden_clip.py
"""
import collections
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from gen_golden_convert import _load  # noqa: E402
from live2diff_amd.clip_hip import SD15_CLIP, random_clip_text_state_dict, tiny_clip_config  # noqa: E402
from live2diff_amd.clip_tokenizer import bytes_to_unicode  # noqa: E402

PROMPTS = [
    "a photo of a cat",
    "A Photo Of A CAT",
    "masterpiece, best quality, 1girl, solo, looking at viewer",
    "don't stop; it's the cat's toy -- isn't it?!",
    "they'll say we've been there, I'm sure you'd agree",
    "   lots   of\t\twhitespace \n here   ",
    "",
    "numbers 12345 and 3.14159, 2024-10-16",
    "café naïve résumé crème brûlée",
    "日本語のテキスト and 中文",
    "emoji 🙂🎉 test",
    "(((emphasis))) [brackets] {braces} <angle>",
    "hello!!!??? ...",
    "user@example.com #hashtag $100 50%",
    "origami style, paper folding, colorful",
    "mixed123letters456 and_under_score",
    "ÀÉÎÕÜ upper accents",
    "a " * 40 + "end",
    " ".join(f"word{i}" for i in range(60)),
    "the quick brown fox jumps over the lazy dog",
]
TRAIN = ("a photo of the cat and the dog, best quality masterpiece; the quick brown fox jumps over the lazy dog. "
         "origami style paper folding colorful watercolor painting of a girl looking at the viewer, solo, "
         "there they were, it is what it is, numbers and letters, hello world")


def _hf_model(cfg):
    from transformers import CLIPTextConfig, CLIPTextModel
    hc = CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                        max_position_embeddings=cfg.max_position_embeddings, layer_norm_eps=cfg.layer_norm_eps,
                        hidden_act="quick_gelu", bos_token_id=0, eos_token_id=2, pad_token_id=1)
    return CLIPTextModel._from_config(hc, attn_implementation="eager").eval()


def _ids(B, V, g, lengths):
    """BOS, random body, EOS, EOS padding (the SD-1.x layout)"""
    ids = torch.full((B, 77), V - 1, dtype=torch.int64)
    for b in range(B):
        n = lengths[b]
        ids[b, 0] = V - 2
        ids[b, 1:n + 1] = torch.randint(0, V - 2, (n,), generator=g)
    return ids


@torch.no_grad()
def _run(m, sd, ids, skips):
    m.load_state_dict(sd, strict=True)
    o = m(ids, output_hidden_states=True)
    outs = {}
    for k in skips:
        outs[k] = o.last_hidden_state if k is None else m.final_layer_norm(o.hidden_states[-(k + 1)])
    return outs


def gen_hf():
    g = torch.Generator().manual_seed(0)
    res = {}
    cfg = SD15_CLIP
    ids = _ids(2, cfg.vocab_size, g, [9, 75])
    outs = _run(_hf_model(cfg), random_clip_text_state_dict(cfg, 0), ids, (None, 1, 2))
    res["full_ids"] = ids.numpy()
    sel = torch.randint(0, 2 * 77 * 768, (4096,), generator=g)
    res["full_sel"] = sel.numpy()
    for k, o in outs.items():
        tag = "none" if k is None else str(k)
        res[f"full_{tag}_vals"] = o.reshape(-1)[sel].numpy()
        res[f"full_{tag}_rownorm"] = o.norm(dim=-1).numpy()
    tc = tiny_clip_config()
    tids = _ids(3, tc.vocab_size, g, [0, 20, 75])
    touts = _run(_hf_model(tc), random_clip_text_state_dict(tc, 1), tids, (None, 1))
    res["tiny_ids"] = tids.numpy()
    for k, o in touts.items():
        res["tiny_" + ("none" if k is None else str(k))] = o.numpy()
    np.savez_compressed(os.path.join(HERE, "clip_hf.npz"), **res)
    print("clip_hf.npz:", sorted(res))


def _learn_merges(text, n):
    bu = bytes_to_unicode()
    words = collections.Counter()
    for w in text.lower().replace(",", " ").replace(".", " ").replace(";", " ").split():
        sym = [bu[b] for b in w.encode()]
        sym[-1] += "</w>"
        words[tuple(sym)] += 1
    merges = []
    for _ in range(n):
        pairs = collections.Counter()
        for w, c in words.items():
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p: pairs[p])
        merges.append(best)
        nw = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i < len(w) - 1 and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            nw[tuple(out)] += c
        words = nw
    return merges


def gen_tok():
    from transformers import CLIPTokenizer
    d = os.path.join(HERE, "clip_tok")
    os.makedirs(d, exist_ok=True)
    bu = list(bytes_to_unicode().values())
    vocab_l = bu + [c + "</w>" for c in bu]
    merges = _learn_merges(TRAIN, 300)
    vocab_l += ["".join(m) for m in merges]
    vocab_l += ["<|startoftext|>", "<|endoftext|>"]
    vocab = {t: i for i, t in enumerate(vocab_l)}
    with open(os.path.join(d, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(d, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(" ".join(m) for m in merges) + "\n")
    tok = CLIPTokenizer.from_pretrained(d)
    ids = tok(PROMPTS, padding="max_length", max_length=77, truncation=True).input_ids
    with open(os.path.join(d, "ids.json"), "w", encoding="utf-8") as f:
        json.dump({"prompts": PROMPTS, "ids": ids}, f, ensure_ascii=False)
    print("clip_tok:", len(vocab), "tokens,", len(merges), "merges, bos/eos", vocab["<|startoftext|>"], vocab["<|endoftext|>"])


def gen_convert():
    ref_ckpt = _load("convert_from_ckpt")
    ref_lora = _load("convert_lora_safetensor_to_diffusers")
    tc = tiny_clip_config()
    sd = random_clip_text_state_dict(tc, 2)
    ldm = {"cond_stage_model.transformer.text_model." + k: v for k, v in sd.items()}
    ldm["cond_stage_model.transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    ldm["model.diffusion_model.conv_in.weight"] = torch.zeros(1)
    ldm["first_stage_model.decoder.conv_in.weight"] = torch.zeros(1)
    conv = ref_ckpt.convert_ldm_clip_checkpoint(ldm)
    res = {"ldm_keys": np.array(sorted(ldm)), "conv_keys": np.array(sorted(conv))}
    m = _hf_model(tc)
    m.load_state_dict(sd, strict=True)

    class TE(torch.nn.Module):         # the 4.x module tree (text_encoder.text_model.encoder...) the reference walks
        def __init__(self, tm):
            super().__init__()
            self.text_model = tm

    g = torch.Generator().manual_seed(3)
    lora = {}
    for i in range(tc.num_hidden_layers):
        for mod, (o, n) in {"self_attn_q_proj": (192, 192), "self_attn_out_proj": (192, 192), "mlp_fc1": (384, 192),
                            "mlp_fc2": (192, 384)}.items():
            stem = f"lora_te_text_model_encoder_layers_{i}_{mod}"
            lora[stem + ".lora_down.weight"] = 0.1 * torch.randn(4, n, generator=g)
            lora[stem + ".lora_up.weight"] = 0.1 * torch.randn(o, 4, generator=g)
            lora[stem + ".alpha"] = torch.tensor(4.0)
    with torch.no_grad():
        ref_lora.convert_lora_model_level(dict(lora), unet=None, text_encoder=TE(m), alpha=0.7)
    after = m.state_dict()
    for k, v in lora.items():
        res["lora." + k] = v.numpy()
    for k in sd:                       # merged tensors: 2048 sampled entries each (flat index, value after the merge)
        if not torch.equal(after[k], sd[k]):
            idx = torch.randint(0, after[k].numel(), (2048,), generator=g)
            res["merged_idx." + k], res["merged_val." + k] = idx.numpy(), after[k].reshape(-1)[idx].numpy()
    np.savez_compressed(os.path.join(HERE, "clip_convert.npz"), **res)
    print("clip_convert.npz:", len(conv), "converted keys,", sum(k.startswith("merged_idx.") for k in res), "merged tensors")


if __name__ == "__main__":
    gen_tok()
    gen_convert()
    gen_hf()
