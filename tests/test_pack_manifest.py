"""The UNet's packing pass, run on the CPU for the six UNet shapes of the plan fingerprints, yields the structure recorded in
tests/golden/pack_manifest.json: every key of `W` with shape and dtype, the offset tables and totals, `_pack_layout()`
(tools/pack_manifest.py).  A change that is meant to leave the packed format alone is checked here; after a deliberate format
change (PACK_FORMAT) regenerate the fixture with `python tools/pack_manifest.py --write`."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pack_manifest as pm  # noqa: E402
import plan_fingerprint as pf  # noqa: E402


@pytest.mark.parametrize("name", list(pm.CONFIGS))
def test_packed_structure_matches_the_fixture(name, monkeypatch):
    for k in [k for k in os.environ if k.startswith("L2D_")]:
        monkeypatch.delenv(k)
    got = pm.structure(pm.pack(name))
    assert got["W"]
    diff = pm.first_difference(got, pm.load_fixture()[name])
    assert diff is None, diff


def test_the_fixture_covers_the_unet_plans_and_every_packed_form():
    want = pm.load_fixture()
    assert set(want) == set(pm.CONFIGS) == {k for k in pf.PLANS if k.startswith("unet-")}
    suffixes = {k.rsplit(".", 1)[1] for d in want.values() for k in d["W"]}
    assert {"w", "w1", "rw", "rw1", "ww", "ww1", "wcs", "cw", "chw"} <= suffixes
