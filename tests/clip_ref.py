"""fp32 torch restatement of SD-1.x's CLIP text tower (test infrastructure; transformers' CLIPTextModel with eager attention,
pinned against it by tests/golden/clip_hf.npz).  Keys as live2diff_amd.clip_hip.clip_text_spec."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F


def clip_text_forward(sd: Dict[str, torch.Tensor], cfg, input_ids: torch.Tensor, clip_skip: Optional[int] = None,
                      all_hidden: bool = False):
    """[B, T] ids -> [B, T, C] fp32: last layer + final LayerNorm, or with clip_skip = k layer (L - k)'s output + final LayerNorm.
    all_hidden: also return the list of hidden states (embeddings, then every layer's output)."""
    W = {k: v.float() for k, v in sd.items()}
    C, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    d = C // H
    B, T = input_ids.shape
    x = W["embeddings.token_embedding.weight"][input_ids] + W["embeddings.position_embedding.weight"][:T][None]
    hidden = [x]
    causal = torch.full((T, T), float("-inf"), device=x.device).triu(1)
    lin = lambda v, p: F.linear(v, W[p + ".weight"], W[p + ".bias"])
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        h = F.layer_norm(x, (C,), W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps)
        q, k, v = (lin(h, p + f"self_attn.{n}_proj").view(B, T, H, d).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + causal, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, C), p + "self_attn.out_proj")
        h = lin(F.layer_norm(x, (C,), W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps), p + "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), p + "mlp.fc2")
        hidden.append(x)
    src = hidden[-1] if clip_skip is None else hidden[-(clip_skip + 1)]
    out = F.layer_norm(src, (C,), W["final_layer_norm.weight"], W["final_layer_norm.bias"], eps)
    return (out, hidden) if all_hidden else out
