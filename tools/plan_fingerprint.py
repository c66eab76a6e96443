"""Fingerprints of the static launch plans -> tests/golden/plan_fingerprints.json.

A plan is a list of `l2d_op` records; two builds that emit the same records in the same order, with the same data flow between
their buffers, launch the same work.  `fingerprint(op_lists)` reduces one plan to its op count, a sha256 over the whole plan and
an 8-hex digest per op, with every pointer rewritten as (ordinal of the storage it lands in, byte offset), so the result does not
depend on where the allocator placed anything.  tests/test_plan_fingerprints.py rebuilds every plan below on CPU tensors in
validate-only mode and compares it with the committed fixture: a host-side change that is meant to leave the launches alone
proves it there.

    python tools/plan_fingerprint.py            compare every plan with the fixture
    python tools/plan_fingerprint.py --write    regenerate the fixture after a DELIBERATE plan change (records HEAD's hash)

Run it with no L2D_* override set: the overrides move layers between kernels.
"""
import argparse
import bisect
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")


def _storages(op_lists):
    """Merged [start, end) byte ranges of the storages behind the lists' keep-alive tensors (overlapping views -> one range)."""
    spans = set()

    def walk(keep):
        for t in keep:
            if isinstance(t, (tuple, list)):         # `pl.append(*ops.x(...))` stores an op's keep-alive tuple as one entry
                walk(t)
            elif t is not None and t.untyped_storage().nbytes():
                s = t.untyped_storage()
                spans.add((s.data_ptr(), s.data_ptr() + s.nbytes()))

    for pl in op_lists:
        walk(pl._keep)
    merged = []
    for a, b in sorted(spans):
        if merged and a < merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    return merged


def canonical_ops(op_lists):
    """One tuple per op of the lists, in order: (kind, i, l, bit patterns of f, pointers as (storage ordinal, byte offset)).
    Ordinals number the storages by first use.  A pointer that lands in no kept tensor is an error."""
    spans = _storages(op_lists)
    starts = [a for a, _ in spans]
    ordinal = {}
    out = []
    for li, pl in enumerate(op_lists):
        for j, op in enumerate(pl._ops):
            ptrs = []
            for k in range(len(op.p)):
                v = op.p[k]
                if not v:
                    ptrs.append(None)
                    continue
                s = bisect.bisect_right(starts, v) - 1
                if s < 0 or v >= spans[s][1]:
                    raise ValueError(f"list {li} op {j} (kind {op.kind}): p[{k}] = {v:#x} lands in no tensor the plan keeps alive")
                ptrs.append((ordinal.setdefault(s, len(ordinal)), v - spans[s][0]))
            fbits = struct.unpack("<4I", struct.pack("<4f", *op.f))
            out.append((int(op.kind), tuple(op.i), tuple(op.l), fbits, tuple(ptrs)))
    return out


def fingerprint(op_lists):
    """dict(n_ops, kinds, sha256, ops): `ops` holds 8 hex digits per op, `kinds` the op kinds (to name a differing op)."""
    whole = hashlib.sha256()
    digests, kinds = [], []
    for c in canonical_ops(op_lists):
        r = repr(c).encode()
        whole.update(r)
        digests.append(hashlib.sha256(r).hexdigest()[:8])
        kinds.append(c[0])
    return dict(n_ops=len(digests), sha256=whole.hexdigest(), kinds=kinds, ops="".join(digests))


def first_difference(got, want):
    """None when the fingerprints agree, else a sentence naming the first differing op."""
    if got["sha256"] == want["sha256"] and got["n_ops"] == want["n_ops"]:
        return None
    g = [got["ops"][8 * j:8 * j + 8] for j in range(got["n_ops"])]
    w = [want["ops"][8 * j:8 * j + 8] for j in range(want["n_ops"])]
    for j, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return (f"first differing op: index {j}, kind {got['kinds'][j]} (fixture: kind {want['kinds'][j]}); "
                    f"{got['n_ops']} ops built, {want['n_ops']} in the fixture")
    return f"{got['n_ops']} ops built, {want['n_ops']} in the fixture; the common prefix agrees"


# ----------------------------------------------------------------------------- the plans the fixture covers
def _unet(cfg_kw, h, w, N, tiny=None):
    import torch

    from live2diff_amd.config import sd15_config, tiny_config
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import random_state_dict, unet_param_spec
    if tiny is not None:
        cfg = tiny_config(**tiny)
        sd = random_state_dict(cfg, dtype=torch.float16)
    else:
        cfg = sd15_config(**cfg_kw)
        sd = {k: torch.zeros(shp, dtype=torch.float16) for k, shp in unet_param_spec(cfg).items()}
    unet = HipStreamingUNet(sd, cfg, h, w, N, device="cpu")
    del sd
    kv = unet.prepare_cache(N)
    out = {}
    for mode in ("stream", "warmup"):
        st = unet._plan(mode, kv)
        out[mode] = [st.cond_pl, st.pl]
    return out


def _stream_step():
    import torch

    from live2diff_amd.config import tiny_config
    from live2diff_amd.stream_step_hip import HipStreamStep
    from live2diff_amd.unet_hip import HipStreamingUNet
    from live2diff_amd.weights import random_state_dict
    cfg = tiny_config(channels=(64, 128, 128, 128), cross_attention_dim=64)
    N = 3
    unet = HipStreamingUNet(random_state_dict(cfg, dtype=torch.float16), cfg, 16, 16, N, device="cpu")
    kv = unet.prepare_cache(N)
    one = torch.ones(N, 1, 1, 1, 1, dtype=torch.float16)
    step = HipStreamStep(unet, kv, torch.tensor([399, 299, 199]), torch.zeros(N, 77, 64, dtype=torch.float16), one, one, one, one)
    # (the step's list holds copies of the UNet's records; their tensors are kept alive by the UNet's own lists, which the step owns)
    return {"step": [step.st.cond_pl, step.st.pl, step.pl]}


def _vae_kl():
    import torch

    from live2diff_amd.vae_kl_hip import HipAutoencoderKL, sd_vae_param_spec
    v = HipAutoencoderKL({k: torch.zeros(s, dtype=torch.float16) for k, s in sd_vae_param_spec().items()}, device="cpu")
    return {f"{side}-{B}x{H}x{W}": [v._plan(side, B, H, W).pl]
            for side, B, H, W in (("enc", 1, 64, 64), ("dec", 1, 8, 8), ("enc", 2, 256, 384), ("dec", 2, 32, 48))}


def _taesd():
    import torch

    from live2diff_amd.vae_hip import HipTinyVAE, taesd_param_spec
    v = HipTinyVAE({k: torch.zeros(s, dtype=torch.float16) for k, s in taesd_param_spec().items()}, device="cpu")
    return {f"{side}-{B}x{H}x{W}": [v._plan(side, B, H, W).pl]
            for side, B, H, W in (("enc", 1, 512, 512), ("dec", 1, 64, 64), ("enc", 8, 256, 256))}


def _midas(B, img):
    import torch

    from live2diff_amd.midas_hip import HipMidas, midas_param_spec
    m = HipMidas({k: torch.zeros(s, dtype=torch.float16) for k, s in midas_param_spec(img).items()}, device="cpu", img=img)
    return {"plan": [m._build(B, img, img).pl]}


# name -> builder of {plan name: op lists}; the smallest set that reaches every branch of the shared plan builder
PLANS = {
    "unet-tiny-16x24-n2": lambda: _unet(None, 16, 24, 2, tiny=dict(channels=(64, 128, 256, 256), cross_attention_dim=96)),
    "unet-sd15-64x64-n2-l16": lambda: _unet({}, 64, 64, 2),                                   # cfg-2: rowchain, cconv, wsgemm, tuned tables
    "unet-sd15-32x32-n1-l12": lambda: _unet(dict(window_size=12, sink_size=4), 32, 32, 1),    # cfg-1: chain off, row GEMM everywhere
    "unet-sd15-72x128-n2-l40": lambda: _unet(dict(window_size=40, sink_size=8), 72, 128, 2),  # cfg-5
    "unet-sd15-48x48-n2": lambda: _unet({}, 48, 48, 2),                # untuned: gn_self / gn_stats fallbacks, deep split-K
    "unet-sd15-64x32-n2": lambda: _unet(dict(window_size=16, sink_size=8), 64, 32, 2),        # narrow latent: no wsgemm conv at level 3
    "stream-step-tiny": _stream_step,
    "vae-kl": _vae_kl,
    "taesd": _taesd,
    "midas-1x384": lambda: _midas(1, 384),
    "midas-3x128": lambda: _midas(3, 128),
}


def build(name):
    """{"<name>/<plan>": fingerprint} of one entry of PLANS, built on CPU tensors in validate-only mode."""
    from live2diff_amd import _lib
    if any(k.startswith("L2D_") for k in os.environ):
        raise RuntimeError("unset the L2D_* overrides: " + ", ".join(k for k in os.environ if k.startswith("L2D_")))
    was = _lib._DRY_RUN
    _lib.set_dry_run(True)
    try:
        return {f"{name}/{k}": fingerprint(lists) for k, lists in PLANS[name]().items()}
    finally:
        _lib.set_dry_run(was)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate the fixture (after a deliberate plan change)")
    ap.add_argument("names", nargs="*", help="entries of PLANS (default: all)")
    a = ap.parse_args()
    plans = {}
    for name in a.names or PLANS:
        plans.update(build(name))
        print(f"built {name}", file=sys.stderr)
    if a.write:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        doc = dict(commit=head, plans=plans)
        if a.names and os.path.exists(FIXTURE):                 # a partial regeneration keeps the other entries
            doc["plans"] = {**load_fixture()["plans"], **plans}
        with open(FIXTURE, "w") as f:
            f.write("{\n" + f' "commit": {json.dumps(head)},\n "plans": {{\n')
            f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(doc["plans"].items())))
            f.write("\n }\n}\n")
        print(f"wrote {len(doc['plans'])} plans to {os.path.relpath(FIXTURE, ROOT)}")
        return 0
    want = load_fixture()["plans"]
    bad = 0
    for k, got in plans.items():
        diff = first_difference(got, want[k]) if k in want else "not in the fixture"
        print(f"{k}: {'same' if diff is None else diff}")
        bad += diff is not None
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
