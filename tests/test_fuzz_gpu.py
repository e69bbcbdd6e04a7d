"""GPU: a bounded, seeded slice of tools/fuzz.py -- randomised differential testing of every kernel family against
the CPU oracle (or, for the kernels that replace torch modules, against those modules): shapes, batch sizes, launch
shapes (shr_set_tuning), non-finite records, negative radii, behind-the-background crops ... drawn at random.
The long run on the round's final kernels is kept in profiles/rNN_fuzz_summary.txt; this one holds every push to the
same checker: a FIXED number of cases per family under a fixed seed (the same cases on every box: what passes here
passes at the next run), ZERO mismatches."""
import importlib.util
import os

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = {"*": 200, "sphere": 100, "mesh": 100, "d2m": 150, "band": 60, "synth": 60, "trigrad": 40, "interp": 40}
GRAD_FAMILIES = ("trigrad", "interp")      # the fixed-point backwards of the triangle family: a test function of their own
SEED = 20260929


@pytest.fixture(scope="module")
def fuzz():
    spec = importlib.util.spec_from_file_location("shr_fuzz", os.path.join(ROOT, "tools", "fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(fuzz, families):
    lines = []
    res = fuzz.run(families, CASES, None, SEED, log=lines.append)
    print("\n".join(lines))
    assert set(res) == set(families)
    assert all(n == CASES.get(name, CASES["*"]) for name, (n, _) in res.items()), res
    assert sum(m for _, m in res.values()) == 0, "\n".join(lines)
    return res


def test_every_family_of_the_fuzzer_is_clean(fuzz):
    """Every entry of FAMILIES is run by this function or by the next one: sixteen in all."""
    names = [name for name, _ in fuzz.FAMILIES]
    assert len(names) == 16 and len(set(names)) == 16 and set(GRAD_FAMILIES) <= set(names)
    res = _run(fuzz, [n for n in names if n not in GRAD_FAMILIES])
    assert len(res) == 14


def test_the_gradient_families_are_clean_and_skip_little(fuzz):
    """trigrad and interp judge a case by the error bound of tests/fixed_point_ref.py, which needs every reference term
    finite; a case that is not is skipped and counted, and more than 5 % of a family's cases skipped fails."""
    res = _run(fuzz, list(GRAD_FAMILIES))
    assert len(res) == 2
    for name in GRAD_FAMILIES:
        assert fuzz.skipped[name] <= 0.05 * res[name][0], (name, fuzz.skipped[name])
