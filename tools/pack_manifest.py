"""Manifest of the UNet's packed weights -> tests/golden/pack_manifest.json.

The packing pass turns a reference-keyed state dict into `W` (name -> packed tensor; the key suffix says which kernel's form a layer
has) plus a few scalars.  For the six UNet shapes of tools/plan_fingerprint.py this tool reports the STRUCTURE of that result --
every key of `W` with shape and dtype, `temb_offsets`, `text_offsets`, `n_map_blocks`, `temb_total`, `text_total`, `text_kp`,
`_pack_layout()` -- and, with --digests, a sha256 per packed tensor.  tests/test_pack_manifest.py compares the structure with the
committed fixture; the digests are for comparing two commits on ONE machine (packing folds norms, sums columns and projects the
positional encodings in floating point, whose last bit may depend on the host's BLAS), so they are printed and never committed.

    python tools/pack_manifest.py               compare the structure with the fixture
    python tools/pack_manifest.py --write       regenerate the fixture after a DELIBERATE change of the packed format
    python tools/pack_manifest.py --digests     print "<config> <key> <sha256>" per packed tensor, and a total

It only uses the UNet's constructor, `.W`, the offset attributes and `_pack_layout()`.  Run it with no L2D_* override set.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "pack_manifest.json")

# the UNet entries of plan_fingerprint.PLANS: name -> (config keywords or None for the tiny config, h, w, N)
TINY = dict(channels=(64, 128, 256, 256), cross_attention_dim=96)
CONFIGS = {
    "unet-tiny-16x24-n2": (None, 16, 24, 2),
    "unet-sd15-64x64-n2-l16": ({}, 64, 64, 2),
    "unet-sd15-32x32-n1-l12": (dict(window_size=12, sink_size=4), 32, 32, 1),
    "unet-sd15-72x128-n2-l40": (dict(window_size=40, sink_size=8), 72, 128, 2),
    "unet-sd15-48x48-n2": ({}, 48, 48, 2),
    "unet-sd15-64x32-n2": (dict(window_size=16, sink_size=8), 64, 32, 2),
}
SCALARS = ("temb_offsets", "text_offsets", "n_map_blocks", "temb_total", "text_total", "text_kp")
_sd_cache = {}


def _state_dict(cfg, random):
    """zeros give the structure; the digests need non-zero weights, generated once per channel configuration (the state dict does
    not depend on the window)"""
    import torch

    from live2diff_amd.weights import random_state_dict, unet_param_spec
    if not random:
        return {k: torch.zeros(shp, dtype=torch.float16) for k, shp in unet_param_spec(cfg).items()}
    key = (cfg.block_out_channels, cfg.cross_attention_dim)
    if key not in _sd_cache:
        _sd_cache[key] = random_state_dict(cfg, dtype=torch.float16)
    return _sd_cache[key]


def pack(name, random=False):
    """the UNet of one entry of CONFIGS, packed on the CPU in validate-only mode"""
    from live2diff_amd import _lib
    from live2diff_amd.config import sd15_config, tiny_config
    from live2diff_amd.unet_hip import HipStreamingUNet
    if any(k.startswith("L2D_") for k in os.environ):
        raise RuntimeError("unset the L2D_* overrides: " + ", ".join(k for k in os.environ if k.startswith("L2D_")))
    cfg_kw, h, w, N = CONFIGS[name]
    cfg = tiny_config(**TINY) if cfg_kw is None else sd15_config(**cfg_kw)
    was = _lib._DRY_RUN
    _lib.set_dry_run(True)
    try:
        return HipStreamingUNet(_state_dict(cfg, random), cfg, h, w, N, device="cpu")
    finally:
        _lib.set_dry_run(was)


def structure(unet):
    doc = {k: getattr(unet, k) for k in SCALARS}
    doc["layout"] = unet._pack_layout()
    doc["W"] = {k: f"{str(t.dtype).replace('torch.', '')} {'x'.join(map(str, t.shape))}" for k, t in sorted(unet.W.items())}
    return json.loads(json.dumps(doc))          # (as the fixture holds it: tuples -> lists)


def digests(unet):
    import torch
    return {k: hashlib.sha256(t.detach().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for k, t in sorted(unet.W.items())}


def load_fixture():
    """{configuration: structure}.  The file holds `W` turned inside out -- key -> {shape and dtype: the configurations that have it
    so, as indices into the sorted names} -- because most keys and many shapes are common to the configurations"""
    with open(FIXTURE) as f:
        doc = json.load(f)
    out = {name: dict(v, W={}) for name, v in doc["configs"].items()}
    order = sorted(out)
    for k, specs in doc["W"].items():
        for spec, which in specs.items():
            for j in which:
                out[order[j]]["W"][k] = spec
    return out


def write_fixture(docs):
    Wd = {}
    for j, (name, d) in enumerate(sorted(docs.items())):
        for k, spec in d["W"].items():
            Wd.setdefault(k, {}).setdefault(spec, []).append(j)
    with open(FIXTURE, "w") as f:
        f.write('{\n "configs": {\n')
        f.write(",\n".join(f"  {json.dumps(n)}: {json.dumps({k: v for k, v in d.items() if k != 'W'})}" for n, d in sorted(docs.items())))
        f.write('\n },\n "W": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(Wd.items())) + "\n }\n}\n")


def first_difference(got, want):
    """None when the structures agree, else a sentence naming the first differing entry."""
    for k in (*SCALARS, "layout"):
        if got[k] != want[k]:
            return f"{k}: {got[k]} != fixture {want[k]}"
    for k in sorted(set(got["W"]) | set(want["W"])):
        if got["W"].get(k) != want["W"].get(k):
            return f"W[{k!r}]: {got['W'].get(k)} != fixture {want['W'].get(k)}"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate the fixture (after a deliberate change of the packed format)")
    ap.add_argument("--digests", action="store_true", help="print a sha256 per packed tensor (random weights) instead of comparing")
    ap.add_argument("names", nargs="*", help="entries of CONFIGS (default: all)")
    a = ap.parse_args()
    names = a.names or list(CONFIGS)
    if a.digests:
        n = nbytes = 0
        whole = hashlib.sha256()
        for name in names:
            unet = pack(name, random=True)
            for k, d in digests(unet).items():
                print(name, k, d)
                whole.update(f"{name} {k} {d}\n".encode())
            n, nbytes = n + len(unet.W), nbytes + unet.weight_bytes()
        print(f"total: {n} tensors, {nbytes} bytes, sha256 {whole.hexdigest()}")
        return 0
    docs = {name: structure(pack(name)) for name in names}
    if a.write:
        if a.names and os.path.exists(FIXTURE):                 # a partial regeneration keeps the other entries
            docs = {**load_fixture(), **docs}
        write_fixture(docs)
        print(f"wrote {len(docs)} configurations to {os.path.relpath(FIXTURE, ROOT)}")
        return 0
    want = load_fixture()
    bad = 0
    for name, got in docs.items():
        diff = first_difference(got, want[name]) if name in want else "not in the fixture"
        print(f"{name}: {'same' if diff is None else diff}")
        bad += diff is not None
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
