"""The plan fuzz without a GPU: for every committed (template, seed) the
project's CPU models, chained through their segment layouts, give pyarrow's answer, and
every row sits in the partition its key hashes to. This holds the generator, the reference
executor, the normal form and the partition check before a device is involved; the same
seeds run on the device in test_gpu_plan_fuzz.py.

test_coverage keeps the seed set from going hollow: it fails when the committed seeds stop
meeting the join types, key dtypes, NULLs, partition counts and empty inputs they are here
for."""

import functools

import pytest

from tests import plan_fuzz as pf

# 12 per template, picked so that test_coverage holds (see there)
SEEDS = {
    "agg": (6, 16, 19, 22, 35, 36, 58, 69, 74, 78, 83, 89),
    "join_agg": (6, 16, 23, 28, 34, 54, 61, 65, 74, 79, 91, 93),
    "join_join_agg": (5, 23, 31, 43, 48, 60, 64, 73, 77, 79, 83, 86),
}
CASES = [(t, s) for t in pf.TEMPLATES for s in SEEDS[t]]


@functools.lru_cache(maxsize=None)
def solved(template, seed):
    """(case, reference result, model result), computed once per module run."""
    case = pf.gen_case(template, seed)
    return case, pf.run_reference(case), pf.run_model(case)


def test_generator_is_deterministic():
    a, b = pf.gen_case("join_join_agg", 5), pf.gen_case("join_join_agg", 5)
    assert a["plan"] == b["plan"] and a["P"] == b["P"] and a["exchange"] == b["exchange"]
    for ta, tb in zip(a["tables"], b["tables"]):
        assert ta["schema"] == tb["schema"]
        assert pf.rows_of(ta["cols"], ta["schema"]) == pf.rows_of(tb["cols"], tb["schema"])


@pytest.mark.parametrize("template,seed", CASES)
def test_model_matches_pyarrow(template, seed):
    case, ref, model = solved(template, seed)
    assert len(model["joined"]) == len(ref["joined"]) == len(pf.join_nodes(case["plan"]))
    for i, (got, want) in enumerate(zip(model["joined"], ref["joined"])):
        assert got == want, f"join {i} ({pf.join_nodes(case['plan'])[i]['type']}) differs"
    assert model["rows"] == ref["rows"]
    checked = pf.check_partitions(case, model)
    assert checked >= len(ref["rows"])


def test_partition_check_catches_a_wrong_seg_part():
    """The row multiset of a join stays right when two segments swap partitions; the
    partition check is what notices."""
    case, _, model = solved("join_agg", 6)
    assert case["P"] > 1
    rows, parts = model["joined_parts"][0]
    moved = [(p + 1) % case["P"] for p in parts]
    bad = dict(model, joined_parts=[(rows, moved)])
    with pytest.raises(AssertionError, match="sits in partition"):
        pf.check_partitions(case, bad)


@pytest.mark.parametrize("template", pf.TEMPLATES)
def test_coverage(template):
    runs = [solved(template, s) for s in SEEDS[template]]
    assert len(set(SEEDS[template])) == len(runs) == 12
    cover = [case["cover"] for case, _, _ in runs]

    def met(name):
        return set().union(*[c[name] for c in cover])

    if template == "agg":
        assert met("key_dtypes") == set(pf.AGG_KEY_DTYPES)
        spill = [c for c in cover if c["spill"]]
        assert len(spill) == 3  # a quarter of the seeds
        assert all(c["n_groups"] > c["table_slots"] for c in spill)
    else:
        assert met("key_dtypes") == set(pf.JOIN_KEY_DTYPES)
        assert met("join_types") == set(pf.JOIN_TYPES)
    if template == "join_join_agg":
        assert sum(c["same_key"] for c in cover) == 6  # and 6 repartition the first result
    assert met("ops") == set(pf.OPS)
    assert any(c["nullable_key"] for c in cover)
    assert any(c["empty_table"] for c in cover)
    ps = {case["P"] for case, _, _ in runs}
    assert ps <= set(pf.P_CHOICES) and ps & {3, 7, 61}, "no P that is not a power of two"
    assert {case["exchange"] for case, _, _ in runs} == {"comm", "part"}
    # a partition with rows on exactly one side of a join (agg: a partition of the
    # partials' shuffle without rows beside one with rows)
    assert any(model["stats"]["one_sided"] for _, _, model in runs)
    assert sum(len(ref["rows"]) == 0 for _, ref, _ in runs) <= 2
    # the joins are not all trivial either
    if template != "agg":
        assert sum(max(len(j) for j in ref["joined"]) >= 1000 for _, ref, _ in runs) >= 6
