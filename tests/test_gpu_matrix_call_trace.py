"""What every public method of the three resident matrices (reductive_amd/qmatrix.py) asks of `Pq`, case by case, against
the trace recorded from the commit before their searches shared one driver per search kind
(tests/golden/matrix_call_trace.json; cases and recorder: tests/matrix_call_cases.py).  Per case: the Pq device methods
called, in order, with every argument -- scalars, and tensors by dtype, shape, strides and bytes -- the kernels launched,
the dtype, shape and bytes of every returned tensor (of a returned matrix: of every tensor it stores), and the type and
text of a raised exception."""
import json

import pytest

import matrix_call_cases as mc

pytestmark = pytest.mark.gpu

with open(mc.GOLDEN) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(scope="module")
def env():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return mc.Env(reductive_amd)


def test_the_golden_holds_every_case():
    assert list(GOLDEN) == list(mc.CASES)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_matrix_call_trace(env, monkeypatch, name):
    assert mc.run_case(env, mc.CASES[name], monkeypatch.setattr) == GOLDEN[name]
