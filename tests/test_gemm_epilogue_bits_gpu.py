"""Bit identity of the conv_gemm epilogues against recorded values: every case of tests/golden/generate_epilogue_bits.py (first-generation
direct / staged paths, the register epilogue's fast and generic paths on the second- and third-generation tiles, split-K partials and
the three reduce kernels, 3x3 / temporal gathers) is re-run and the SHA-256 of its output bytes - and of the gn_colsum bytes where the
launch emits them - must equal tests/golden/gemm_epilogue_bits.json, which was recorded on an MI355X at the commit BEFORE the epilogue
code was factored into gemm_epilogue.h. No tolerance, no skipped case: a refactor of that code must not move a bit.
On a mismatch: `python tests/golden/generate_epilogue_bits.py --only <case> --dump DIR` at both commits saves the tensors."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("generate_epilogue_bits", os.path.join(_GOLDEN, "generate_epilogue_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.JSON_PATH) as _f:
    RECORDED = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(RECORDED) == sorted(gen.CASES), sorted(set(RECORDED) ^ set(gen.CASES))


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_epilogue_bits(dev, name):
    got = gen.digests(gen.run_case(name, dev))
    want = RECORDED[name]
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, f"{name}: {bad} differ from the recorded bytes"
