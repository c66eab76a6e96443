"""CLIP byte-level BPE tokenizer, host side, with no transformers import.

Pinned to transformers' `CLIPTokenizer` as installed with this project (5.x, the `tokenizers`-backed class; there is no ftfy in the
build image, and 4.x without ftfy took its BasicTokenizer path instead): NFC, runs of whitespace -> one space, lowercase; the split
pattern `<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+` (whitespace between pieces
dropped); every piece's UTF-8 bytes through the `bytes_to_unicode` table; BPE with `</w>` on the last symbol of a word; BOS 49406 +
at most 75 tokens + EOS 49407, padded to 77 with the pad token (`special_tokens_map.json` / `tokenizer_config.json`, default
`<|endoftext|>`).  No ftfy / html.unescape clean-up is applied (neither does the pinned tokenizer).

The split uses the `regex` module when it is importable, else a stdlib scanner over unicodedata categories (L* letters, N*
numbers) that yields the same pieces.
"""
import json
import os
import re
import unicodedata
from functools import lru_cache
from typing import Dict, List, Optional

try:
    import regex as _regex
except ImportError:          # pragma: no cover - depends on the machine
    _regex = None

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
SPLIT_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""
_CONTRACTIONS = ("s", "t", "re", "ve", "m", "ll", "d")


@lru_cache()
def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2 / CLIP byte -> printable unicode character table."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def _is_letter(ch: str) -> bool:
    return unicodedata.category(ch).startswith("L")


def _is_number(ch: str) -> bool:
    return unicodedata.category(ch).startswith("N")


def split_stdlib(text: str) -> List[str]:
    """The split pattern as a scanner (alternatives tried in the pattern's order at every position)."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch.isspace():
            i += 1
            continue
        sp = next((s for s in (BOS, EOS) if text.startswith(s, i)), None)
        if sp:
            out.append(sp)
            i += len(sp)
            continue
        if ch == "'":
            c = next((c for c in _CONTRACTIONS if text.startswith(c, i + 1)), None)
            if c:
                out.append("'" + c)
                i += 1 + len(c)
                continue
        j = i + 1
        if _is_letter(ch):
            while j < n and _is_letter(text[j]):
                j += 1
        elif not _is_number(ch):
            while j < n and not (text[j].isspace() or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
        out.append(text[i:j])
        i = j
    return out


class ClipTokenizer:
    def __init__(self, vocab: Dict[str, int], merges: List[str], max_length: int = 77, pad_token: str = EOS,
                 use_regex: Optional[bool] = None):
        self.encoder = dict(vocab)
        self.bpe_ranks = {tuple(m.split()): r for r, m in enumerate(merges)}
        self.max_length = max_length
        self.bos_id, self.eos_id = self.encoder[BOS], self.encoder[EOS]
        self.unk_id = self.eos_id                    # CLIPTokenizer's unk_token is <|endoftext|>
        self.pad_id = self.encoder[pad_token]
        self.byte_encoder = bytes_to_unicode()
        if use_regex is None:
            use_regex = _regex is not None
        if use_regex and _regex is None:
            raise ImportError("the regex module is not installed")
        self._pat = _regex.compile(SPLIT_PATTERN) if use_regex else None
        self._cache = {}

    @classmethod
    def from_dir(cls, path: str, max_length: int = 77, use_regex: Optional[bool] = None) -> "ClipTokenizer":
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            lines = f.read().split("\n")
        merges = [ln for ln in lines if ln and not ln.startswith("#version")]
        pad = EOS
        for name in ("special_tokens_map.json", "tokenizer_config.json"):
            fp = os.path.join(path, name)
            if os.path.exists(fp):
                with open(fp, encoding="utf-8") as f:
                    p = json.load(f).get("pad_token")
                if isinstance(p, dict):
                    p = p.get("content")
                if p:
                    pad = p
                    break
        return cls(vocab, merges, max_length=max_length, pad_token=pad, use_regex=use_regex)

    def normalize(self, text: str) -> str:
        return re.sub(r"\s+", " ", unicodedata.normalize("NFC", text)).lower()

    def split(self, text: str) -> List[str]:
        return self._pat.findall(text) if self._pat is not None else split_stdlib(text)

    def bpe(self, token: str) -> List[str]:
        if token in self._cache:
            return self._cache[token]
        word = list(token[:-1]) + [token[-1] + "</w>"]
        while len(word) > 1:
            pairs = {(word[i], word[i + 1]) for i in range(len(word) - 1)}
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if best not in self.bpe_ranks:
                break
            a, b = best
            merged, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        self._cache[token] = word
        return word

    def tokenize_ids(self, text: str) -> List[int]:
        """ids without BOS / EOS, untruncated"""
        ids = []
        for piece in self.split(self.normalize(text)):
            if piece in (BOS, EOS):
                ids.append(self.encoder[piece])
                continue
            mapped = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
            ids.extend(self.encoder.get(t, self.unk_id) for t in self.bpe(mapped))
        return ids

    def encode(self, text: str) -> List[int]:
        """[BOS] + first (max_length - 2) ids + [EOS], padded to max_length (padding='max_length', truncation=True)"""
        ids = [self.bos_id] + self.tokenize_ids(text)[: self.max_length - 2] + [self.eos_id]
        return ids + [self.pad_id] * (self.max_length - len(ids))

    def __call__(self, texts):
        import torch

        texts = [texts] if isinstance(texts, str) else list(texts)
        return torch.tensor([self.encode(t) for t in texts], dtype=torch.int64)
