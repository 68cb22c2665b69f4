"""The plan fuzz on the device (marked gpu): the seeds of
test_plan_fuzz_cpu.py, each plan run through api.py with every operator reading the device
view and the segment layout the one before it returned, held to pyarrow's answer over the
whole tables. Every join's output is compared as a row multiset, the final result row for
row, both exactly, and every row must sit in the partition its key hashes to.

If the device differs from pyarrow while test_plan_fuzz_cpu.py passes, the models agree with
pyarrow and the fault is in a kernel, in dd_host.cpp or in api.py's views and layouts."""

import pytest

from tests import plan_fuzz as pf
from tests.test_plan_fuzz_cpu import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("template,seed", CASES)
def test_device_matches_pyarrow(template, seed):
    case = pf.gen_case(template, seed)
    ref = pf.run_reference(case)
    dev = pf.run_device(case)
    nodes = pf.join_nodes(case["plan"])
    assert len(dev["joined"]) == len(ref["joined"]) == len(nodes)
    for i, (got, want) in enumerate(zip(dev["joined"], ref["joined"])):
        assert len(got) == len(want), f"join {i} ({nodes[i]['type']}): row count differs"
        assert got == want, f"join {i} ({nodes[i]['type']}) differs"
    assert dev["rows"] == ref["rows"]
    assert pf.check_partitions(case, dev) >= len(ref["rows"])
