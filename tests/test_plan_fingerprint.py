"""CPU: the complete launch list of every plan kind against tests/golden/plan_fingerprints.json.

A plan builds on CPU tensors with the built library and launches nothing, so what it WOULD launch -- every entry point, argument,
descriptor field, the weight preparation work and the replay bookkeeping -- is pinned here without a GPU (canonical form and cases:
tests/tools/mint_plan_fingerprints.py).  The golden was minted from the engine before it was split into modules; a change that
means to alter a plan re-mints it and shows the per-entry-point launch counts that moved."""
import importlib.util
import json
import os

import pytest

import helpers as H

_spec = importlib.util.spec_from_file_location("mint_plan_fingerprints",
                                               os.path.join(H.ROOT, "tests", "tools", "mint_plan_fingerprints.py"))
MINT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MINT)

CASES = MINT.cases()
_BUILT = {}


def _golden():
    with open(MINT.GOLDEN) as f:
        return json.load(f)


def _fingerprint(case):
    if case["name"] not in _BUILT:
        _BUILT[case["name"]] = MINT.fingerprint(MINT.build_plan(case))
    return _BUILT[case["name"]]


def test_golden_lists_exactly_the_cases():
    assert sorted(_golden()) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_its_fingerprint(case):
    want, got = _golden()[case["name"]], _fingerprint(case)
    # the readable parts first: a moved launch count names the entry point
    assert got["launches"] == want["launches"]
    assert got["counts"] == want["counts"]
    assert got["bytes"] == want["bytes"]
    assert got["sha256"] == want["sha256"]


@pytest.mark.parametrize("case", [c for c in CASES if c["default"]], ids=[c["name"] for c in CASES if c["default"]])
def test_a_switch_changes_the_plan(case):
    """a switch that silently stops applying would leave its case equal to the default one"""
    default = next(c for c in CASES if c["name"] == case["default"])
    assert _fingerprint(case)["sha256"] != _fingerprint(default)["sha256"]
    assert _golden()[case["name"]]["sha256"] != _golden()[default["name"]]["sha256"]
