"""CPU tests (-m "not gpu") of the output chain as a whole: the wrapper on the mock components of
tests/pipeline_mocks.py (its host route) against tests/chain_model.py, byte for byte on every output -- one scripted scenario
that sets, changes and clears every mode mid-stream for 1, 2 and 3 denoising steps, seeded random scripts whose coverage is
asserted from the model alone, and seven mutants of the orchestration, each of which must make the scripted scenario fail."""
import numpy as np
import pytest
import torch

import chain_model as CM
from test_matte_cpu import build
from test_steady_cpu import frames_of, moving, pre

CPU_MODES = ("lock", "steady", "matte", "edge", "size")          # (the host route has neither a camera route nor detail)
SIZE_A, SIZE_B = (80, 112, "lanczos"), (48, 96, "bicubic")

# seeds of the random scripts, chosen on the CPU so that the coverage conditions of `test_seeded_scripts` hold
SEEDS = {2: tuple(range(100, 120)), 1: tuple(range(200, 206)), 3: tuple(range(300, 306))}
EVENTS = 24


def source_of(x, kind):
    """the mock image processor's frame, as the delay line keeps it"""
    assert kind == "float", kind
    return pre(x).float()


def start(monkeypatch, n_steps, twin=True):
    """(run, warm-up frames): a wrapper, its model and a twin on the mocks, `DropFilter`s installed, nothing prepared yet"""
    import pipeline_mocks as M
    rec = CM.TapRecorder(monkeypatch)
    w = build(monkeypatch, n_steps, drop=set())
    t = build(monkeypatch, n_steps, drop=set()) if twin else None
    model = CM.ChainModel(n_steps, M.H, M.W, source_of)
    run = CM.ChainRun(w, model, rec, filt=w.stream.similar_filter, twin=t, twin_filt=t.stream.similar_filter if twin else None)
    return run, M.frames(8, seed=7)


# ----------------------------------------------------------------------------- the scripted scenario
def scenario():
    """~30 frames: modes set before `prepare`; each of lock ("ema", "source", an image), steady, matte (both `keep`s, `feather`,
    `show`), matte edge and output size set and cleared mid-stream so that every pair of them overlaps; `set_matte_source` and
    `set_detail` (no-ops on the host route); a second `prepare`; dropped calls, one directly behind a settings change and one
    directly behind a mid-stream start of the line; `output_type` over u8 / pil / jpeg / pt / np with the ValueError where a set
    mode does not serve the type; at the end everything is cleared and the bytes are a twin's that never had a mode."""
    import pipeline_mocks as M
    warm = M.frames(8, seed=7)
    mv = moving(frames_of(14, seed=31))                    # a moving camera
    un = frames_of(12, seed=32)                            # unrelated frames: everything moves between any two
    mw = moving(frames_of(8, seed=33))
    image = M.frames(1, seed=34)[0]
    S = lambda name, *a, **kw: ("set", name, a, kw)
    F, D = (lambda x: ("frame", x)), (lambda x: ("drop", x))
    return [
        S("set_matte", 0.3, 0.7, feather=2), S("set_steady"), ("prepare", warm),
        F(mv[0]), F(mv[1]), F(mv[2]),                                              # matte + steady
        S("set_color_lock", "ema", 0.8, 0.3), F(mv[3]),                            # + lock
        S("set_matte_edge", 2, 4.0), D(mv[4]),                                     # + edge; a drop directly behind a settings change
        F(mv[4]),
        S("set_output_size", *SIZE_A), F(mv[5]),                                   # all five
        ("type", "pil"), F(mv[6]),
        ("type", "jpeg"), F(mv[7]),
        S("set_matte_source", "camera"), S("set_detail"), F(mv[8]),                # no-ops on the host route
        S("set_steady", 3, 12, strength=0.5, radius=1), D(mv[9]),                  # steady restarted, and a drop directly behind it
        S("set_color_lock", "ema", 0.6, 0.5), D(mv[9]),                            # the lock restarted, likewise
        F(mv[9]),
        ("type", "pt"), S("set_matte", 0.1, 0.9), F(mv[10]),                       # both raise: the matte and the size do not serve "pt"
        S("clear_matte"), S("clear_output_size"), S("clear_detail"), S("clear_matte_edge"),
        F(mv[11]),                                                                 # lock + steady as "pt"
        ("type", "np"), F(mv[12]),
        ("type", "latent"), S("set_steady"), F(mv[13]),                            # both raise: nothing serves "latent"
        ("type", "u8"),
        S("set_color_lock", "source", 0.7), S("set_matte", 0.2, 0.8, keep="far"), F(un[0]), F(un[1]),
        S("set_matte", 0.2, 0.8, keep="far", feather=3, show=True), S("set_matte_edge", 3, 10.0), F(un[2]),
        S("set_steady", 2, 10, show=True), F(un[3]), F(un[4]),
        S("clear_steady"), S("clear_matte"), S("clear_color_lock"), F(un[5]),      # the line is gone
        S("set_steady"), F(un[6]), F(un[7]), F(un[8]), F(un[9]),                   # a mid-stream start on unrelated frames
        S("clear_steady"), F(un[10]),
        S("set_color_lock", "source"), D(un[11]), F(un[11]),                       # a drop directly behind a mid-stream start
        S("set_matte", 0.4, 0.6, feather=1), S("set_matte_edge", 1, 2.0), S("set_output_size", *SIZE_B),
        ("prepare", warm),                                                         # a second prepare, modes set
        F(mw[0]), F(mw[1]), S("set_color_lock", image, 0.9), S("set_steady"), F(mw[2]), D(mw[3]), F(mw[3]), F(mw[4]),
        ("type", "jpeg"), S("set_output_size", 72, 100), F(mw[5]),                 # raises: no whole MCUs; the old size stays
        ("type", "u8"),
        S("clear_matte_edge"), S("clear_matte"), S("clear_steady"), S("clear_output_size"), S("clear_color_lock"),
        S("set_matte_source", "stream"), ("twin",),
        F(mw[6]), F(mw[7]), D(mw[0]), F(mw[1]),
    ]


def check_cleared(w):
    assert w._matte_line is None and w.stream.matte_tap is None
    assert w.matte is None and w.color_lock is None and w.steady is None and w.output_size is None and w.detail is None and w.matte_edge is None
    left = [k for k in vars(type(w)) if k.startswith("_") and k.endswith("_dev") and getattr(w, k) is not None]
    assert not left and w._camera is None and w._matte_up is None and w._lock_last is None and w._steady_last is None, left


@pytest.mark.parametrize("n_steps", [1, 2, 3])
def test_scripted_scenario(monkeypatch, n_steps):
    run, _ = start(monkeypatch, n_steps)
    log = run.play(scenario())
    outs = [e for e in log if e != "raised"]
    assert log.count("raised") == 2 and len(outs) >= 30
    check_cleared(run.w)
    # the walk is what its docstring says: every pair of modes acts together, every output type left, frames were repeated under
    # steady and under a lock, the line started mid-stream, and the twin's bytes came back
    for i, a in enumerate(CPU_MODES):
        for b in CPU_MODES[i + 1:]:
            assert sum(1 for e in outs if {a, b} <= e.acts) >= 1, (a, b)
    assert {e.output_type for e in outs} == {"u8", "pil", "jpeg", "pt", "np"}
    assert sum(1 for e in outs if e.repeated and e.acts & {"lock", "steady"}) >= 3
    assert run.m.line_starts == 2
    print(f"N = {n_steps}: {len(outs)} outputs equal the model; stages per output:")
    for i, e in enumerate(log):
        print(f"  {i:2d} " + ("raised" if e == "raised" else f"{e.output_type:4s} {'rep ' if e.repeated else ''}{' '.join(e.stages)}"))


# ----------------------------------------------------------------------------- seeded random scripts
def random_script(seed, n_events=EVENTS, hooks=None):
    """Events drawn from `seed` with fixed weights: frames (a moving camera, now and then a cut to an unrelated frame), dropped
    calls, each mode toggled with random settings, the output type, `prepare`.  Some modes are set before `prepare`.  `hooks`
    (the device test's): its own frames (`warm`, `fresh(g)`, `move(base, k, g)`, `image(g)`, `dress(x, rng)`: the frame as a
    JPEG file, a float tensor or a PIL image now and then), the further `modes` it toggles, the output `types` it draws from
    the probability `preset` of a mode being set before `prepare`, and the `sticky` modes it mostly keeps set."""
    import pipeline_mocks as M
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(int(seed))
    S = lambda name, *a, **kw: ("set", name, a, kw)
    state = dict(base=None, k=0, frames=0, camera=False)

    def fresh(g):
        return torch.rand(3, M.H, M.W, generator=g)

    def move(base, k, g):
        x = (base + torch.randint(-1, 2, (3, M.H, M.W), generator=g) / 255.0).clamp(0, 1)
        x0 = (8 * k) % (M.W - 16)
        x[:, :, x0:x0 + 16] = torch.rand(3, M.H, 16, generator=g)
        return x

    h = dict(warm=None, fresh=fresh, move=move, image=fresh, dress=lambda x, rng: x, modes=CPU_MODES,
             types=["u8", "u8", "pil", "jpeg", "pt", "np"], preset=0.5, sticky=())
    h.update(hooks or {})
    warm = M.frames(8, seed=7) if h["warm"] is None else h["warm"]
    modes = h["modes"]

    def frame():
        if state["base"] is None or rng.random() < 0.15:
            state["base"], state["k"] = h["fresh"](g), 0
            return h["dress"](state["base"], rng)
        state["k"] += 1
        return h["dress"](h["move"](state["base"], state["k"], g), rng)

    def toggle(mode, on):
        if on and mode in h["sticky"] and rng.random() < 0.6:      # (a mode the device scripts mostly keep: new settings, no clear)
            on = False
        if mode == "lock":
            if on and rng.random() < 0.6:
                return S("clear_color_lock")
            to = ("ema", "source", None)[int(rng.integers(3))]
            to = h["image"](g) if to is None else to
            return S("set_color_lock", to, float(rng.choice([1.0, 0.7])), float(rng.choice([0.1, 0.5])))
        if mode == "steady":
            if on and rng.random() < 0.6:
                return S("clear_steady")
            return S("set_steady", float(rng.choice([2, 3])), float(rng.choice([10, 12])), strength=float(rng.choice([0.8, 1.0, 0.5])),
                     radius=int(rng.integers(0, 4)), show=bool(rng.random() < 0.1))
        if mode == "matte":
            if on and rng.random() < 0.4:
                return S("clear_matte")
            return S("set_matte", float(rng.choice([0.2, 0.3, 0.5])), float(rng.choice([0.5, 0.7, 0.8])), keep=str(rng.choice(["near", "far"])),
                     feather=int(rng.integers(0, 4)), show=bool(rng.random() < 0.1))
        if mode == "edge":
            if on and rng.random() < 0.3:
                return S("clear_matte_edge")
            return S("set_matte_edge", int(rng.integers(1, 5)), float(rng.choice([1.0, 4.0, 10.0])))
        if mode == "size":
            if on and rng.random() < 0.5:
                return S("clear_output_size")
            return S("set_output_size", *(SIZE_A, SIZE_B, (64, 64, "bilinear"))[int(rng.integers(3))])
        if mode == "detail":
            if on and rng.random() < 0.3:
                return S("clear_detail")
            return S("set_detail", int(rng.integers(1, 4)), float(rng.choice([1.0, 2.0])), float(rng.choice([1.0, 2.5])),
                     float(rng.choice([64.0, 20.0])), bool(rng.random() < 0.1))
        if mode == "camera":
            return S("set_matte_source", "stream" if on and rng.random() < 0.3 else "camera")
        raise KeyError(mode)

    on = dict.fromkeys(modes, False)
    script = []
    for mode in modes:                                           # before prepare
        if rng.random() < h["preset"]:
            script.append(toggle(mode, False))
            on[mode] = True
    script.append(("prepare", warm))
    ot = "u8"
    for _ in range(n_events):
        r = rng.random()
        if r < 0.50 or not state["frames"]:
            script.append(("frame", frame()))
            state["frames"] += 1
        elif r < 0.60:
            script.append(("drop", frame()))
        elif r < 0.90:
            mode = modes[int(rng.integers(len(modes)))]
            ev = toggle(mode, on[mode])
            # (`on` only steers the draw: a float output type refuses the matte, the size and detail, and nothing changes)
            refused = ev[1].startswith("set_") and ot in ("pt", "np") and mode in ("matte", "size", "detail")
            if not refused:
                on[mode] = ev[1].startswith("set_") and not (ev[1] == "set_matte_source" and ev[2][0] == "stream")
            script.append(ev)
        elif r < 0.97:
            ot = str(rng.choice(h["types"]))
            script.append(("type", ot))
        else:
            script.append(("prepare", warm))
    return script


def tally(logs):
    outs = [e for log in logs for e in log if e != "raised"]
    pairs = {(a, b): sum(1 for e in outs if {a, b} <= e.acts) for i, a in enumerate(CPU_MODES) for b in CPU_MODES[i + 1:]}
    share = {a: sum(1 for e in outs if a in e.acts) / len(outs) for a in CPU_MODES}
    repeated = sum(1 for e in outs if e.repeated and e.acts & {"lock", "steady"})
    return outs, pairs, share, repeated


def test_seeded_scripts(monkeypatch):
    """20 seeds x 24 events at N = 2 and 6 seeds each at N = 1 and N = 3: every output equals the model, and the conditions
    below -- computed from the model alone -- keep a script from quietly running the plain route."""
    logs, starts, raised = [], 0, 0
    for n_steps, seeds in SEEDS.items():
        for seed in seeds:
            with monkeypatch.context() as mp:
                run, _ = start(mp, n_steps, twin=False)
                try:
                    logs.append(run.play(random_script(seed)))
                except AssertionError as e:
                    raise AssertionError(f"N = {n_steps}, seed {seed}: {e}") from e
                starts += run.m.line_starts
                raised += logs[-1].count("raised")
    outs, pairs, share, repeated = tally(logs)
    print(f"{len(logs)} scripts, {len(outs)} outputs, {raised} refused calls, {starts} mid-stream line starts, "
          f"{repeated} repeated frames under steady or a lock")
    print("outputs on which both modes act:", {f"{a}+{b}": n for (a, b), n in pairs.items()})
    print("share of the outputs a mode acts on:", {a: round(s, 3) for a, s in share.items()})
    assert min(pairs.values()) >= 10, pairs
    assert min(share.values()) >= 0.25, share
    assert repeated >= 5 and starts >= 5


def test_device_scripts_reach_the_device_routes():
    """the condition of tests/test_gpu_chain.py::test_seeded_scripts_on_device, from the model alone (`play_model_only`): at
    least half of the outputs of its three scripts sit on the device-only routes -- so the seeds are known to hold before a
    device runs them"""
    import test_gpu_chain as G
    warm = np.stack(G.unrelated(8, seed=1))
    logs = []
    for seed in G.DEVICE_SEEDS:
        assert seed in SEEDS[2]
        model = CM.ChainModel(2, G.H, G.W, G.source_of, source_tol=5e-4, device_route=True)
        logs.append(CM.play_model_only(model, random_script(seed, hooks=G.device_hooks(warm))))
    n, total = G.on_device_routes(logs)
    print(f"{total} outputs, {n} on the device-only routes")
    assert 2 * n >= total and total >= 30


# ----------------------------------------------------------------------------- mutants of the orchestration
def old_steadied(self, image_tensor, slot, repeated):
    """`_steadied` as it was before the steady start was fixed: the sequence starts on whatever slot `take()` hands out"""
    from live2diff_amd.steady import steady_ref
    st = self._steady
    if repeated and self._steady_last is not None:
        return self._steady_last
    if slot is None:
        self._steady_init, self._steady_last = True, None
        return image_tensor
    out, self._steady_state = steady_ref(image_tensor[:1], slot.source, self._steady_state, lo=st["lo"], hi=st["hi"], strength=st["strength"],
                                         radius=st["radius"], show=st["show"], init=self._steady_init)
    out = torch.from_numpy(out)
    self._steady_init = False
    self._steady_last = out
    return out


def plant(mp, name):
    from live2diff_amd import matte as MT
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as W
    locked, steadied = W._locked, W._steadied
    if name == "steady in front of the lock":
        def first(self, x, slot, repeated):
            if self._steady is not None:
                x = steadied(self, x, slot, repeated)
            return locked(self, x, slot, repeated)
        mp.setattr(W, "_locked", first)
        mp.setattr(W, "_steadied", lambda self, x, slot, repeated: x if self._lock is not None else steadied(self, x, slot, repeated))
    elif name == "take() pairs k - (N - 2)":
        def take(self):
            k = self.taken
            self.taken += 1
            idx = min(max(k - (self.n - 2), self._first) - self._first, len(self._hist) - 1)
            self.last_own = k - (self.n - 1) >= self._first
            self._last_id = self._hist[idx]
            self.last = self.slots[self._last_id]
            keep_from = self.taken - (self.n - 1)
            while self._first < keep_from and len(self._hist) > 1:
                self._hist.popleft()
                self._first += 1
            return self.last
        mp.setattr(MT.MatteLine, "take", take)
    elif name == "a repeated frame runs steady again":
        mp.setattr(W, "_steadied", lambda self, x, slot, repeated: steadied(self, x, slot, False))
    elif name == "_steady_last kept across set_steady":
        real = W.set_steady

        def set_steady(self, *a, **kw):
            last = self._steady_last
            real(self, *a, **kw)
            self._steady_last = last
        mp.setattr(W, "set_steady", set_steady)
    elif name == "_lock_last kept across set_color_lock":
        real = W.set_color_lock

        def set_color_lock(self, *a, **kw):
            last = self._lock_last
            real(self, *a, **kw)
            self._lock_last = last
        mp.setattr(W, "set_color_lock", set_color_lock)
    elif name == "the edge refinement behind the feather":
        def composite(styled, source, depth, lo, hi, feather=0, keep="near", show=False, *, edge=None):
            m = MT.matte_ref(depth, lo, hi, 0, keep)
            if feather:
                m = MT._box_pass(MT._box_pass(m, feather, 2), feather, 1)
            if edge is not None:
                src = MT._np16(source)
                m = np.stack([MT.edge_ref(m[b], src[b], edge["radius"], edge["eps"]) for b in range(m.shape[0])])
            m = m[..., None]
            if show:
                return np.rint(np.repeat(m, 3, axis=-1) * np.float32(255.0)).astype(np.uint8)
            vs, vc = MT._unit(styled), MT._unit(source)
            return np.rint((vc + m * (vs - vc)) * np.float32(255.0)).astype(np.uint8)
        mp.setattr(MT, "composite_ref", composite)               # (the wrapper's host route looks it up per frame; the model bound its own)
    elif name == "_steadied before the fix":
        mp.setattr(W, "_steadied", old_steadied)
    else:
        raise KeyError(name)


MUTANTS = ("steady in front of the lock", "take() pairs k - (N - 2)", "a repeated frame runs steady again",
           "_steady_last kept across set_steady", "_lock_last kept across set_color_lock", "the edge refinement behind the feather",
           "_steadied before the fix")


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_fails_the_scenario(monkeypatch, name):
    """each mutant, planted by monkeypatch on the wrapper or on `MatteLine`, makes the scripted scenario fail at N = 2 and at
    N = 3 (the model's own references are bound at its import and stay)"""
    script = scenario()
    for n_steps in (2, 3):
        with monkeypatch.context() as mp:
            run, _ = start(mp, n_steps, twin=False)
            plant(mp, name)
            with pytest.raises(AssertionError) as caught:
                run.play(script)
            print(f"mutant '{name}', N = {n_steps}: {caught.value}")
            assert isinstance(caught.value, CM.ChainMismatch), caught.value
