"""Every static launch plan, rebuilt on CPU tensors in validate-only mode, emits the op records of tests/golden/plan_fingerprints.json:
same kinds, same integer / float arguments, same data flow between buffers (tools/plan_fingerprint.py).  A host-side change that is
meant to leave the launches alone is checked here; after a deliberate plan change regenerate the fixture with
`python tools/plan_fingerprint.py --write`."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_fingerprint as pf  # noqa: E402


@pytest.mark.parametrize("name", list(pf.PLANS))
def test_plan_matches_the_fixture(name, monkeypatch):
    for k in [k for k in os.environ if k.startswith("L2D_")]:
        monkeypatch.delenv(k)
    want = pf.load_fixture()["plans"]
    plans = pf.build(name)
    assert plans
    bad = []
    for key, got in plans.items():
        assert key in want, f"{key} is not in the fixture"
        diff = pf.first_difference(got, want[key])
        if diff is not None:
            print(f"{key}: {diff}")
            bad.append(f"{key}: {diff}")
    assert not bad, "\n".join(bad)


def test_the_fixture_holds_no_other_plans():
    want = pf.load_fixture()
    assert len(want["commit"]) == 40
    assert {k.split("/")[0] for k in want["plans"]} == set(pf.PLANS)


def test_fingerprint_follows_data_flow_not_addresses():
    """two lists with the same records over differently placed buffers agree; re-pointing one operand, or a pointer outside the
    kept tensors, does not pass"""
    import torch

    from live2diff_amd import _lib, ops

    def plan(swap=False):
        a, b, c = (torch.zeros(64, dtype=torch.float16) for _ in range(3))
        pl = _lib.OpList()
        pl.append(*ops.copy(a, b, 128))
        pl.append(*ops.copy(b[16:], c, 64))
        pl.append(*ops.copy((a if swap else b), c, 128))
        return pl, (a, b, c)

    (p1, k1), (p2, k2), (p3, k3) = plan(), plan(), plan(swap=True)
    f1, f2, f3 = pf.fingerprint([p1]), pf.fingerprint([p2]), pf.fingerprint([p3])
    assert f1 == f2 and pf.first_difference(f1, f2) is None
    assert f1["ops"][:16] == f3["ops"][:16] and "index 2" in pf.first_difference(f3, f1)
    assert pf.canonical_ops([p1])[1][4][:2] == ((1, 32), (2, 0))          # (storage ordinal by first use, byte offset)
    stray = torch.zeros(64, dtype=torch.float16)
    p1[2].p[0] = stray.data_ptr()
    with pytest.raises(ValueError):
        pf.fingerprint([p1])
