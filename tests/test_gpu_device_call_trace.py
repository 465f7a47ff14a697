"""What every `*_device` wrapper of reductive_amd/pq.py hands to the C library, case by case, against the trace recorded
from the commit before the wrappers shared one marshalling layer (tests/golden/device_call_trace.json; cases and proxy:
tests/device_call_cases.py).  Per case: the symbols called and every argument -- integers, and pointers as NULL, codebook,
stream, an offset into a named input or an address made by the wrapper -- the shape, dtype, strides and bytes of the
returned tensors, and the type and text of a raised exception."""
import json

import pytest

import device_call_cases as dc

pytestmark = pytest.mark.gpu

with open(dc.GOLDEN) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(scope="module")
def env():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return dc.Env(reductive_amd)


def test_the_golden_holds_every_case():
    assert list(GOLDEN) == list(dc.CASES)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_device_call_trace(env, monkeypatch, name):
    assert dc.run_case(env, dc.CASES[name], monkeypatch.setattr) == GOLDEN[name]
