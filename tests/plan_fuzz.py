"""plan_fuzz.py — random operator chains above the shuffle, three executors, one normal form
(DESIGN.md §21). A plain helper module: tests import it as tests.plan_fuzz.

gen_case(template, seed) draws host tables and a plan tree of four node kinds:

    {"op": "scan", "table": i}
    {"op": "shuffle", "input": node, "keys": [...]}            hash repartition into P
    {"op": "join", "build": node, "probe": node, "type", "bkeys", "pkeys", "bproj", "pproj"}
    {"op": "agg", "input": node, "group": [...], "aggs": [(col | None, op)]}   the root

run_reference executes the tree in pyarrow alone and knows nothing of partitions.
run_model executes it on the CPU through the project's models, segment layouts included.
run_device executes it through api.py on the GPU, every operator consuming the device view
and the layout the one before it returned.

Normal form. Each executor returns {"rows": the final result, "joined": [the output of every
join, in post-order]} as sorted lists of row tuples: NULL is None, a bool is 0 / 1, a decimal
is the Python int of its unscaled value, a float is a Python float. A final row is the group
key values followed, per aggregate, by (count,) for "count" and by (value, nn) for every
other op: nn is count(col), and the value is None when nn is 0. Row order, the order of an
inner pair's matches and duplicate partial groups do not survive the normal form: the API
leaves them unspecified.

The model and the device also return "joined_parts" and "final_parts": the unsorted rows
with the partition each sat in. check_partitions holds them to the hash-partition
guarantee: a row sits in partition oracle.pids(oracle.hash_cols(key), P) of its join key or
group key. A segment handed on with the wrong seg_part fails this even when the row multiset
is right.

Every comparison is exact. Aggregates are restricted to inputs on which every order of
evaluation gives the same bits: integer sums far from 2^63, decimal sums of precision 20,
min / max of finite nonzero doubles, and sum_f64 over integer-valued doubles whose absolute
values sum below 2^53.
"""

import decimal
import math
from collections import Counter

import numpy as np

import oracle
from datafusion_distributed_amd import decagg, finalagg, hashjoin
from oracle import reduce_ref as rr

TEMPLATES = ("agg", "join_agg", "join_join_agg")
P_CHOICES = (1, 2, 3, 7, 16, 61, 128)
ROW_CHOICES = (0, 1, 63, 700, 2049, 6000)
ROW_WEIGHTS = (0.08, 0.08, 0.14, 0.25, 0.25, 0.20)  # the two degenerate sizes more rarely
JOIN_TYPES = ("inner", "left_semi", "left_anti", "right_semi", "right_anti", "left", "right",
              "full")
JOIN_KEY_DTYPES = ("u8", "bool", "i16", "i32", "i64")
AGG_KEY_DTYPES = JOIN_KEY_DTYPES + ("f32", "f64")
FLOAT_KEY_VALUES = (-2.5, -1.0, -0.125, 0.5, 1.0, 3.25, 1024.0)  # finite, nonzero, exact in f32
OPS = ("count", "sum_i64", "min_i64", "max_i64", "sum_f64", "min_f64", "max_f64", "sum_dec128")
DEC_PRECISION, DEC_SCALE = 20, 2
MAX_JOIN_ROWS = 40_000  # inner pairs of one join: keeps a case at a second or two
NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64,
      "f32": np.float32, "f64": np.float64}

_CTX = decimal.Context(prec=60)  # wider than 38 digits: scaleb never rounds


# ---------------- generator ----------------

def _field(name, dtype, role):
    """role: "key" (a join or group key), "rid" (the table's row id, never NULL) or "pay"."""
    return {"name": name, "dtype": dtype, "role": role}


def _valid(rng, n, nullable, frac):
    return (rng.random(n) >= frac).astype(np.uint8) if nullable else None


def _n_rows(rng):
    return int(rng.choice(ROW_CHOICES, p=ROW_WEIGHTS))


def _pool(rng, dtype, n_values):
    if dtype == "bool":
        return rng.integers(0, 2, n_values).astype(np.uint8)
    if dtype in ("f32", "f64"):
        return rng.choice(np.array(FLOAT_KEY_VALUES, dtype=NP[dtype]), n_values)
    info = np.iinfo(NP[dtype])
    return rng.integers(info.min, info.max, n_values, dtype=NP[dtype], endpoint=True)


def _key_cols(rng, dtypes, sizes, n_values):
    """Per table (one per entry of sizes) the key columns: key TUPLES come from one pool of
    n_values tuples, so every table repeats them and the tables meet. Each key of each
    table is nullable with probability 1/2; a nullable key has about 10 % NULLs."""
    picks = [rng.integers(0, n_values, n) for n in sizes]
    out = [[] for _ in sizes]
    for dt in dtypes:
        pool = _pool(rng, dt, n_values)
        for side, pick in zip(out, picks):
            side.append({"dtype": dt, "data": np.ascontiguousarray(pool[pick]),
                         "valid": _valid(rng, len(pick), rng.random() < 0.5, 0.1)})
    return out


def _payload_col(rng, dtype, n):
    valid = _valid(rng, n, rng.random() < 0.5, 0.2)
    if dtype == "u8":
        data = rng.integers(0, 4, n).astype(np.uint8)  # few values: also a group key
    elif dtype == "i16":
        data = rng.integers(-2**15, 2**15, n).astype(np.int16)
    elif dtype == "i32":
        data = rng.integers(-2**31, 2**31, n).astype(np.int32)
    elif dtype == "f32":
        data = (rng.integers(-4000, 4000, n) / 4.0).astype(np.float32)
    elif dtype == "i64":
        data = rng.integers(-2**40, 2**40, n, dtype=np.int64)  # sums stay far from 2^63
    elif dtype == "f64":
        # integer-valued, nonzero, |x| < 2^20: sums of up to 2^33 of them are exact
        data = (rng.integers(1, 2**20, n) * rng.choice((-1, 1), n)).astype(np.float64)
    else:
        # |unscaled| < 10^20: most values need the high word, about half are negative
        hi = rng.integers(-10**10 + 1, 10**10, n).tolist()
        lo = rng.integers(0, 10**10, n).tolist()
        col = {"dtype": "dec128", "data": decagg.dec_words([h * 10**10 + l
                                                            for h, l in zip(hi, lo)]),
               "valid": valid, "precision": DEC_PRECISION, "scale": DEC_SCALE}
        return col
    return {"dtype": dtype, "data": data, "valid": valid}


def _table(rng, name, n, keys, pay_dtypes, extra=()):
    """keys, then extra (field, col) pairs, the row id, the payload columns."""
    schema = [_field(f"{name}_k{i}", c["dtype"], "key") for i, c in enumerate(keys)]
    cols = list(keys)
    for field, col in extra:
        schema.append(field)
        cols.append(col)
    schema.append(_field(f"{name}_rid", "i32", "rid"))
    cols.append({"dtype": "i32", "data": np.arange(n, dtype=np.int32), "valid": None})
    for i, dt in enumerate(pay_dtypes):
        schema.append(_field(f"{name}_p{i}_{dt}", dt, "pay"))
        cols.append(_payload_col(rng, dt, n))
    return {"name": name, "schema": schema, "cols": cols}


def _pay_dtypes(rng):
    """The three an aggregate can read, a u8 (also a group key), and one or two more."""
    rest = [str(d) for d in rng.choice(("i16", "i32", "f32"), int(rng.integers(1, 3)),
                                       replace=False)]
    return ["u8", "i64", "f64", "dec128"] + rest


def _identities(cols, key_idx):
    bits, keynull = rr.key_bits(cols, list(key_idx))
    return [None if m else tuple(b) for b, m in zip(bits.tolist(), keynull.tolist())]


def _key_counts(cols, key_idx):
    c = Counter(_identities(cols, key_idx))
    c.pop(None, None)
    return c


def schema_of(case, node):
    if node["op"] == "scan":
        return case["tables"][node["table"]]["schema"]
    if node["op"] == "shuffle":
        return schema_of(case, node["input"])
    b, p = schema_of(case, node["build"]), schema_of(case, node["probe"])
    return [b[i] for i in node["bproj"]] + [p[i] for i in node["pproj"]]


def join_nodes(node, out=None):
    """The join nodes of a plan in post-order (build subtree first): the order of
    "joined" and "joined_parts"."""
    out = [] if out is None else out
    if node["op"] in ("shuffle", "agg"):
        join_nodes(node["input"], out)
    elif node["op"] == "join":
        join_nodes(node["build"], out)
        join_nodes(node["probe"], out)
        out.append(node)
    return out


def _proj(rng, schema, keys):
    """A side's projection: its join keys, every key and row id column, then 2..3 payloads,
    one of them of a type an aggregate reads."""
    must = list(keys) + [i for i, f in enumerate(schema)
                         if f["role"] in ("key", "rid") and i not in keys]
    pay = [i for i, f in enumerate(schema) if f["role"] == "pay"]
    agg = [i for i in pay if schema[i]["dtype"] in ("i64", "f64", "dec128")]
    first = agg[int(rng.integers(len(agg)))]
    rest = [i for i in pay if i != first]
    more = rng.choice(rest, min(len(rest), int(rng.integers(1, 3))), replace=False)
    return must + sorted([first] + [int(i) for i in more])


def _join(rng, case, build, bkeys, probe, pkeys, join_type, null_routed):
    """A join node. null_routed: both inputs were shuffled on exactly these keys, so even
    a NULL-key row sits where the hash of its key says."""
    bs, ps = schema_of(case, build), schema_of(case, probe)
    bproj = [] if join_type.startswith("right_") else _proj(rng, bs, bkeys)
    pproj = [] if join_type.startswith("left_") else _proj(rng, ps, pkeys)
    node = {"op": "join", "build": build, "probe": probe, "type": join_type,
            "bkeys": list(bkeys), "pkeys": list(pkeys), "bproj": bproj, "pproj": pproj,
            "null_routed": null_routed}
    out = schema_of(case, node)
    nb = len(bproj)
    # where the partition check finds each side's key and row ids in an output row
    node["out_bkey"] = [bproj.index(k) for k in bkeys] if bproj else None
    node["out_pkey"] = [nb + pproj.index(k) for k in pkeys] if pproj else None
    node["out_brid"] = [i for i in range(nb) if out[i]["role"] == "rid"]
    node["out_prid"] = [i for i in range(nb, len(out)) if out[i]["role"] == "rid"]
    return node


def _agg(rng, case, node):
    """The root: group by 1..2 key-like output columns (key columns of either side, a
    NULL-extended one included, or a u8 payload), 1..8 distinct aggregates."""
    schema = schema_of(case, node)
    gcand = [i for i, f in enumerate(schema)
             if f["role"] == "key" or (f["role"] == "pay" and f["dtype"] == "u8")]
    group = [int(i) for i in rng.choice(gcand, int(rng.integers(1, min(2, len(gcand)) + 1)),
                                        replace=False)]
    return {"op": "agg", "input": node, "group": group, "aggs": _choose_aggs(rng, schema)}


def _choose_aggs(rng, schema):
    cand = [(None, "count")]
    for i, f in enumerate(schema):
        if f["role"] != "pay":
            continue
        if f["dtype"] == "i64":
            cand += [(i, "sum_i64"), (i, "min_i64"), (i, "max_i64")]
        elif f["dtype"] == "f64":
            cand += [(i, "sum_f64"), (i, "min_f64"), (i, "max_f64")]
        elif f["dtype"] == "dec128":
            cand.append((i, "sum_dec128"))
    k = int(rng.integers(1, min(8, len(cand)) + 1))
    return [cand[i] for i in sorted(rng.choice(len(cand), k, replace=False).tolist())]


def _pool_size(*sizes, product_cap=20_000):
    """Pool small enough that the sides repeat and large enough that the join stays small."""
    live = [n for n in sizes if n]
    if len(live) < 2:
        return 3
    return max(3, min(live) // 4, math.ceil(math.prod(live[:2]) / product_cap))


def _gen_agg(rng, case, seed):
    from datafusion_distributed_amd import api

    spill = seed % 4 == 3  # a quarter of the seeds: more groups than the LDS table has slots
    n = int(rng.choice((2049, 6000))) if spill else _n_rows(rng)
    dtypes = [str(d) for d in rng.choice(AGG_KEY_DTYPES, int(rng.integers(1, 5)))]
    slots = api.partial_reduce_geometry(n)["table_slots"]
    if spill:
        dtypes[0] = str(rng.choice(("i16", "i32", "i64")))
    n_values = 3 * slots if spill else int(rng.choice((3, 40, 300)))
    keys = _key_cols(rng, dtypes, [n], n_values)[0]
    pay = ["u8", "i64", "i64", "f64", "f64", "dec128", "dec128", "i16", "f32", "i32"]
    case["tables"] = [_table(rng, "a", n, keys, pay)]
    schema = case["tables"][0]["schema"]
    case["plan"] = {"op": "agg", "input": {"op": "scan", "table": 0},
                    "group": list(range(len(keys))), "aggs": _choose_aggs(rng, schema)}
    bits, keynull = rr.key_bits(case["tables"][0]["cols"], case["plan"]["group"])
    groups = set(zip(map(tuple, bits.tolist()), keynull.tolist()))
    case["cover"].update(spill=spill, table_slots=slots, n_groups=len(groups))


def _gen_two_tables(rng):
    """Two tables over one key pool whose inner join has at most MAX_JOIN_ROWS pairs."""
    for _ in range(200):
        nb, npr = _n_rows(rng), _n_rows(rng)
        dtypes = [str(d) for d in rng.choice(JOIN_KEY_DTYPES, int(rng.integers(1, 5)))]
        bk, pk = _key_cols(rng, dtypes, [nb, npr], _pool_size(nb, npr))
        nk = list(range(len(dtypes)))
        cb, cp = _key_counts(bk, nk), _key_counts(pk, nk)
        pairs = sum(c * cp.get(k, 0) for k, c in cb.items())
        if pairs <= MAX_JOIN_ROWS:
            return nb, npr, dtypes, bk, pk, pairs
    raise AssertionError("no bounded join drawn")


def _gen_join_agg(rng, case, seed):
    nb, npr, dtypes, bk, pk, _ = _gen_two_tables(rng)
    case["tables"] = [_table(rng, "a", nb, bk, _pay_dtypes(rng)),
                      _table(rng, "b", npr, pk, _pay_dtypes(rng))]
    keys = list(range(len(dtypes)))
    sides = [{"op": "shuffle", "input": {"op": "scan", "table": t}, "keys": keys}
             for t in (0, 1)]
    j = _join(rng, case, sides[0], keys, sides[1], keys, JOIN_TYPES[seed % 8], True)
    case["plan"] = _agg(rng, case, j)


def _gen_join_join_agg(rng, case, seed):
    t1 = JOIN_TYPES[seed % 8]
    same_key = (seed // 8) % 2 == 0  # half the seeds, whatever the first join's type
    for _ in range(200):
        nb, npr, dtypes, bk, pk, pairs = _gen_two_tables(rng)
        nc = _n_rows(rng)
        nk = list(range(len(dtypes)))
        est1 = pairs + nb + npr  # an outer join's rows at the most
        if same_key:
            # C draws its key tuples from the two tables' own rows, so all three meet
            src = bk if nb >= npr else pk
            n_src = max(nb, npr)
            pick = rng.integers(0, max(n_src, 1), nc if n_src else 0)
            if not n_src:
                nc = 0
            ck = [{"dtype": c["dtype"], "data": np.ascontiguousarray(c["data"][pick]),
                   "valid": _valid(rng, nc, rng.random() < 0.5, 0.1)} for c in src]
            cb, cp, cc = _key_counts(bk, nk), _key_counts(pk, nk), _key_counts(ck, nk)
            triples = sum(c * cp.get(k, 0) * cc.get(k, 0) for k, c in cb.items())
            one_side = max(sum(c * cc.get(k, 0) for k, c in cb.items()),
                           sum(c * cc.get(k, 0) for k, c in cp.items()))
            if max(triples, one_side) > MAX_JOIN_ROWS:
                continue
            extras = ([], [])
        else:
            # the second join's key: one more column on A and on B, one key column on C
            dt2 = str(rng.choice(("i32", "i64")))
            nv2 = _pool_size(est1, nc, product_cap=15_000)
            xa, xb, xc = (c[0] for c in _key_cols(rng, [dt2], [nb, npr, nc], nv2))
            ck = [xc]
            extras = ([(_field("a_x", dt2, "key"), xa)], [(_field("b_x", dt2, "key"), xb)])
        break
    else:
        raise AssertionError("no bounded pair of joins drawn")
    case["tables"] = [_table(rng, "a", nb, bk, _pay_dtypes(rng), extras[0]),
                      _table(rng, "b", npr, pk, _pay_dtypes(rng), extras[1]),
                      _table(rng, "c", nc, ck, _pay_dtypes(rng))]
    sides = [{"op": "shuffle", "input": {"op": "scan", "table": t}, "keys": nk}
             for t in (0, 1)]
    j1 = _join(rng, case, sides[0], nk, sides[1], nk, t1, True)
    s1 = schema_of(case, j1)
    t2 = JOIN_TYPES[int(rng.integers(8))]
    if same_key:
        # J1's key columns from a side the first join never NULL-extends (full: the build
        # side; a row without it has a NULL key and matches nothing)
        jk = j1["out_pkey"] if t1 in ("right", "right_semi", "right_anti") else j1["out_bkey"]
        first, ckeys, routed = j1, nk, False
    else:
        xs = [i for i, f in enumerate(s1) if f["name"] in ("a_x", "b_x")]
        jk = [xs[int(rng.integers(len(xs)))]]
        first = {"op": "shuffle", "input": j1, "keys": jk}
        ckeys, routed = [0], True
    third = {"op": "shuffle", "input": {"op": "scan", "table": 2}, "keys": ckeys}
    if rng.integers(2):  # the first join's output as the build side
        j2 = _join(rng, case, first, jk, third, ckeys, t2, routed)
    else:
        j2 = _join(rng, case, third, ckeys, first, jk, t2, routed)
    case["plan"] = _agg(rng, case, j2)
    case["cover"].update(same_key=same_key)


def gen_case(template, seed):
    """Deterministic in (template, seed). Returns {"template", "seed", "P", "exchange":
    "comm" (Comm.exchange at one rank) or "part" (partitioned_batch), "tables": [{"name",
    "schema", "cols"}], "plan": the tree, "cover": what the case exercises}."""
    rng = np.random.default_rng([TEMPLATES.index(template), seed])
    case = {"template": template, "seed": seed, "P": int(rng.choice(P_CHOICES)),
            "exchange": "comm" if rng.integers(2) else "part", "cover": {}}
    {"agg": _gen_agg, "join_agg": _gen_join_agg,
     "join_join_agg": _gen_join_join_agg}[template](rng, case, seed)
    plan = case["plan"]
    key_fields = []
    if template == "agg":
        key_fields = [(case["tables"][0], i) for i in plan["group"]]
    else:
        for t in case["tables"]:
            key_fields += [(t, i) for i, f in enumerate(t["schema"]) if f["role"] == "key"]
    case["cover"].update(
        join_types=[j["type"] for j in join_nodes(plan)],
        key_dtypes=sorted({t["schema"][i]["dtype"] for t, i in key_fields}),
        nullable_key=any(t["cols"][i]["valid"] is not None and not t["cols"][i]["valid"].all()
                         for t, i in key_fields),
        ops=sorted({op for _, op in plan["aggs"]}),
        empty_table=any(hashjoin.n_rows_of(t["cols"]) == 0 for t in case["tables"]))
    return case


# ---------------- the normal form ----------------

def sort_rows(rows):
    return sorted(rows, key=lambda r: tuple((v is None, 0 if v is None else v) for v in r))


def rows_of(cols, schema):
    """Row tuples of host column dicts (a "valid" entry may be missing or None)."""
    lists = []
    for c, f in zip(cols, schema):
        if f["dtype"] == "dec128":
            vals = decagg.dec_ints(c)
        else:
            vals = np.asarray(c["data"]).tolist()
        if c.get("valid") is not None:
            vals = [v if ok else None for v, ok in zip(vals, np.asarray(c["valid"]).tolist())]
        lists.append(vals)
    return list(zip(*lists))


def _key_value(bits, dtype):
    """A canonical u64 key word (oracle.reduce_ref.key_bits) back as the value."""
    if dtype in ("u8", "bool"):
        return int(bits)
    w = {"i16": np.uint16, "i32": np.uint32, "f32": np.uint32, "i64": np.uint64,
         "f64": np.uint64}[dtype]
    return np.array([bits], dtype=np.uint64).astype(w).view(NP[dtype])[0].item()


def _f64_of_bits(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def _agg_layout(case):
    """(group key dtypes, ops) of the plan's root."""
    plan = case["plan"]
    schema = schema_of(case, plan["input"])
    return [schema[i]["dtype"] for i in plan["group"]], [op for _, op in plan["aggs"]]


# ---------------- executor 1: pyarrow ----------------

_PA_JOIN = {"inner": "inner", "left_semi": "left semi", "left_anti": "left anti",
            "right_semi": "right semi", "right_anti": "right anti", "left": "left outer",
            "right": "right outer", "full": "full outer"}
_PA_FUNC = {"sum_i64": "sum", "min_i64": "min", "max_i64": "max", "sum_f64": "sum",
            "min_f64": "min", "max_f64": "max", "sum_dec128": "sum"}


def _arrow_array(pa, col):
    valid = col.get("valid")
    mask = None if valid is None else ~np.asarray(valid).astype(bool)
    if col["dtype"] == "dec128":
        ints = decagg.dec_ints(col)
        vals = [None if mask is not None and mask[i] else
                _CTX.scaleb(decimal.Decimal(v), -col["scale"]) for i, v in enumerate(ints)]
        return pa.array(vals, type=pa.decimal128(col["precision"], col["scale"]))
    data = np.asarray(col["data"])
    if col["dtype"] == "bool":
        data = data.astype(bool)
    return pa.array(data, mask=mask)


def _plain(v):
    """A pyarrow scalar's Python value in the normal form."""
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, decimal.Decimal):
        return int(_CTX.scaleb(v, DEC_SCALE))
    return v


def _arrow_rows(t):
    return [tuple(_plain(v) for v in row) for row in zip(*(t[n].to_pylist()
                                                          for n in t.column_names))]


def run_reference(case):
    """The plan in pyarrow alone: Table.join and group_by over the whole tables."""
    import pyarrow as pa

    joined = []

    def ev(node):
        if node["op"] == "scan":
            t = case["tables"][node["table"]]
            return pa.table({f["name"]: _arrow_array(pa, c)
                             for f, c in zip(t["schema"], t["cols"])})
        if node["op"] == "shuffle":
            return ev(node["input"])
        left, right = ev(node["build"]), ev(node["probe"])
        t = left.join(right, keys=[left.column_names[k] for k in node["bkeys"]],
                      right_keys=[right.column_names[k] for k in node["pkeys"]],
                      join_type=_PA_JOIN[node["type"]], coalesce_keys=False,
                      use_threads=False)
        t = t.select([f["name"] for f in schema_of(case, node)])
        joined.append(sort_rows(_arrow_rows(t)))
        return t

    plan = case["plan"]
    t = ev(plan["input"])
    names = t.column_names
    specs = []
    for ci, op in plan["aggs"]:
        for s in ([([], "count_all")] if op == "count" else
                  [(names[ci], _PA_FUNC[op]), (names[ci], "count")]):
            if s not in specs:
                specs.append(s)
    res = t.group_by([names[i] for i in plan["group"]], use_threads=False).aggregate(specs)
    got = {n: res[n].to_pylist() for n in res.column_names}
    rows = []
    for r in range(res.num_rows):
        row = [_plain(got[names[i]][r]) for i in plan["group"]]
        for ci, op in plan["aggs"]:
            if op == "count":
                row.append(got["count_all"][r])
            else:
                row += [_plain(got[f"{names[ci]}_{_PA_FUNC[op]}"][r]),
                        got[f"{names[ci]}_count"][r]]
        rows.append(tuple(row))
    return {"rows": sort_rows(rows), "joined": joined}


# ---------------- executor 2: the project's models ----------------

def _parts_of(layout):
    return np.repeat(np.asarray(layout["seg_part"], dtype=np.int64),
                     np.diff(np.asarray(layout["seg_offsets"], dtype=np.int64))).tolist()


def _part_counts(layout):
    return np.bincount(np.asarray(layout["seg_part"], dtype=np.int64),
                       weights=np.diff(np.asarray(layout["seg_offsets"], dtype=np.int64)),
                       minlength=layout["n_parts"])


def _host_data(col):
    if col["dtype"] == "dec128":
        return np.asarray(col["data"]).reshape(-1, 2)
    return np.asarray(col["data"])


def _take(col, idx, null_extended):
    """col[idx] with idx == -1 the absent side: validity 0, value bytes 0."""
    data = _host_data(col)
    absent = idx < 0
    if len(data):
        out = data[np.maximum(idx, 0)]
        out[absent] = 0
    else:
        out = np.zeros((len(idx),) + data.shape[1:], dtype=data.dtype)
    valid = None
    if null_extended or col.get("valid") is not None:
        src = (np.asarray(col["valid"], dtype=np.uint8) if col.get("valid") is not None
               else np.ones(len(data), dtype=np.uint8))
        valid = src[np.maximum(idx, 0)] if len(data) else np.zeros(len(idx), dtype=np.uint8)
        valid[absent] = 0
    return {"dtype": col["dtype"], "data": out, "valid": valid}


def _shuffle_host(cols, key_idx, P):
    """oracle.repartition; a dec128 column (never a key here) rides on the row order it
    returns."""
    plain = [i for i, c in enumerate(cols) if c["dtype"] != "dec128"]
    pos = {i: j for j, i in enumerate(plain)}
    ref = oracle.repartition([cols[i] for i in plain], [pos[k] for k in key_idx], P)
    order = np.asarray(ref["order"], dtype=np.int64)
    out = []
    for i, c in enumerate(cols):
        if i in pos:
            oc = ref["cols"][pos[i]]
            out.append({"dtype": c["dtype"], "data": oc["data"], "valid": oc.get("valid")})
        else:
            v = c.get("valid")
            out.append({"dtype": "dec128", "data": _host_data(c)[order],
                        "valid": None if v is None else np.asarray(v)[order]})
    return out, {"seg_offsets": np.asarray(ref["part_offsets"], dtype=np.int64),
                 "seg_part": np.arange(P, dtype=np.int32), "n_parts": P}


def _slice(cols, a, b):
    return [{"dtype": c["dtype"], "data": np.ascontiguousarray(_host_data(c)[a:b]),
             "valid": None if c.get("valid") is None else np.asarray(c["valid"])[a:b]}
            for c in cols]


def _entry_value(e):
    """An entry of the models' group dicts in the normal form: (count,) or (value, nn)."""
    v, op = e["value"], e["op"]
    if op == "count":
        return (int(v),)
    if v is not None and op in ("min_f64", "max_f64"):
        v = _f64_of_bits(v)
    elif v is not None:
        v = float(v) if op == "sum_f64" else int(v)
    return (v, int(e["nn"]))


def run_model(case):
    """The plan on the CPU through the project's own pieces: oracle.repartition for every
    shuffle, hash_join_ref / outer_join_ref over the segment layouts, reduce_ref (through
    decagg.reduce_dec_ref, which adds the decimal sum) for the partial aggregate,
    partial_state_cols + final_merge_ref for the final one. Also returns "stats":
    {"one_sided": a partition held rows of exactly one side of a join (agg: of the
    partials' shuffle, a partition without rows beside one with rows)}."""
    P = case["P"]
    joined, joined_parts = [], []
    stats = {"one_sided": False}

    def ev(node):
        if node["op"] == "scan":
            return case["tables"][node["table"]]["cols"], None
        if node["op"] == "shuffle":
            return _shuffle_host(ev(node["input"])[0], node["keys"], P)
        (bcols, blay), (pcols, play) = ev(node["build"]), ev(node["probe"])
        cb, cp = _part_counts(blay), _part_counts(play)
        stats["one_sided"] |= bool(((cb > 0) != (cp > 0)).any())
        jt = node["type"]
        if jt in hashjoin.OUTER_JOIN_TYPES:
            segs = hashjoin.outer_join_ref(bcols, node["bkeys"], pcols, node["pkeys"], jt,
                                           blay, play)
        else:
            segs = hashjoin.hash_join_ref(bcols, node["bkeys"], pcols, node["pkeys"], jt,
                                          blay, play)
            if jt != "inner":
                left = jt.startswith("left_")
                segs = [[(r, None) if left else (None, r) for r in seg] for seg in segs]
        flat = [x for seg in segs for x in seg]
        bi = np.array([-1 if b is None else b for b, _ in flat], dtype=np.int64)
        pi = np.array([-1 if p is None else p for _, p in flat], dtype=np.int64)
        cols = [_take(bcols[c], bi, jt in ("right", "full")) for c in node["bproj"]] + \
               [_take(pcols[c], pi, jt in ("left", "full")) for c in node["pproj"]]
        if jt in ("left", "full"):
            seg_part = np.concatenate([play["seg_part"], blay["seg_part"]])
        else:
            seg_part = (blay if jt.startswith("left_") else play)["seg_part"]
        layout = {"seg_offsets": hashjoin.seg_offsets_of(segs),
                  "seg_part": np.asarray(seg_part, dtype=np.int32), "n_parts": P}
        rows = rows_of(cols, schema_of(case, node))
        joined.append(sort_rows(rows))
        joined_parts.append((rows, _parts_of(layout)))
        return cols, layout

    plan = case["plan"]
    cols, _ = ev(plan["input"])
    key_dtypes, ops = _agg_layout(case)
    n = hashjoin.n_rows_of(cols)
    # two blocks of rows, reduced apart: duplicate partial groups, as the device leaves them
    blocks = [(0, n // 2), (n // 2, n)]
    partials = finalagg.groups_as_partials(
        [decagg.reduce_dec_ref(_slice(cols, a, b), plan["group"], plan["aggs"])
         for a, b in blocks if b > a], len(plan["group"]), ops)
    pcols, kidx, faggs = finalagg.partial_state_cols(partials, key_dtypes, ops)
    scols, lay = _shuffle_host(pcols, kidx, P)
    if case["template"] == "agg":
        cnt = _part_counts(lay)
        stats["one_sided"] = bool((cnt == 0).any() and (cnt > 0).any())
    merged = finalagg.final_merge_ref(scols, kidx, faggs, **lay)
    rows, parts = [], []
    for p, groups in enumerate(merged):
        for (bits, mask), entries in groups.items():
            row = [None if (mask >> k) & 1 else _key_value(b, dt)
                   for k, (b, dt) in enumerate(zip(bits, key_dtypes))]
            for e in entries:
                row += _entry_value(e)
            rows.append(tuple(row))
            parts.append(p)
    return {"rows": sort_rows(rows), "joined": joined, "joined_parts": joined_parts,
            "final_parts": (rows, parts), "stats": stats}


# ---------------- executor 3: the device ----------------

def run_device(case):
    """The plan through api.py on the GPU. Every operator reads the non-owning device view
    and the layout of the one before it: Partitioner, then Comm.exchange at one rank +
    exchanged_batch or partitioned_batch (case["exchange"]; a shuffle of a join's output is
    always Partitioner + partitioned_batch), hash_join / outer_join, Joined.batch(),
    partial_reduce, partial_state_cols re-uploaded, Partitioner on the group keys,
    final_merge(view, ..., **layout). Every handle is destroyed in a finally."""
    from datafusion_distributed_amd import api

    P = case["P"]
    undo = []  # callables, run in reverse
    joined, joined_parts = [], []
    comm = []

    def upload(cols):
        batch = api.DeviceBatch(cols)
        undo.append(batch.free)
        return batch

    def shuffle(batch, keys, exchange):
        part = api.Partitioner(batch, keys, P)
        undo.append(part.destroy)
        part.run()
        part.sync()
        if exchange != "comm":
            return api.partitioned_batch(part)
        ex = comm[0].exchange(part)
        undo.append(ex.destroy)
        return api.exchanged_batch(ex)

    def ev(node):
        if node["op"] == "scan":
            return upload(case["tables"][node["table"]]["cols"]), None
        if node["op"] == "shuffle":
            scan = node["input"]["op"] == "scan"
            return shuffle(ev(node["input"])[0], node["keys"],
                           case["exchange"] if scan else "part")
        (bview, blay), (pview, play) = ev(node["build"]), ev(node["probe"])
        assert blay["n_parts"] == play["n_parts"] == P
        run = api.outer_join if node["type"] in api.OUTER_JOIN_TYPES else api.hash_join
        j = run(bview, node["bkeys"], pview, node["pkeys"], node["type"], blay, play,
                build_proj=node["bproj"], probe_proj=node["pproj"])
        undo.append(j.destroy)
        view, layout = j.batch()
        off = layout["seg_offsets"]
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == j.n_rows == view.n_rows
        rows = rows_of([j.col(i) for i in range(len(j._out_cols))], schema_of(case, node))
        joined.append(sort_rows(rows))
        joined_parts.append((rows, _parts_of(layout)))
        return view, layout

    try:
        if case["exchange"] == "comm":
            comm.append(api.Comm(api.Comm.unique_id(), 0, 1))
            undo.append(comm[0].destroy)
        plan = case["plan"]
        view, _ = ev(plan["input"])
        key_dtypes, ops = _agg_layout(case)
        res = api.partial_reduce(view, plan["group"], plan["aggs"])
        pcols, kidx, faggs = finalagg.partial_state_cols(res, key_dtypes, ops)
        sview, lay = shuffle(upload(pcols), kidx, case["exchange"])
        fm = api.final_merge(sview, kidx, faggs, **lay)
    finally:
        for f in reversed(undo):
            f()

    goff = fm["group_offsets"]
    assert goff[0] == 0 and (np.diff(goff) >= 0).all() and goff[-1] == len(fm["keynull"])
    parts = np.repeat(np.arange(P), np.diff(goff)).tolist()
    lo = np.ascontiguousarray(fm["aggs"]).view(np.uint64).tolist()
    hi, nn = fm["aggs_hi"].tolist(), fm["nn"].tolist()
    rows = []
    for r, (bits, mask) in enumerate(zip(fm["keys"].tolist(), fm["keynull"].tolist())):
        row = [None if (mask >> k) & 1 else _key_value(b, dt)
               for k, (b, dt) in enumerate(zip(bits, key_dtypes))]
        for g, op in enumerate(ops):
            if op == "count":
                row.append(rr.to_signed64(lo[r][g]))
                continue
            if nn[r][g] == 0:
                v = None  # SQL NULL: the value slot is unspecified
            elif op == "sum_dec128":
                v = decagg.to_signed128(lo[r][g] | (hi[r][g] << 64))
            elif op.endswith("f64"):
                v = _f64_of_bits(lo[r][g])
            else:
                v = rr.to_signed64(lo[r][g])
            row += [v, nn[r][g]]
        rows.append(tuple(row))
    return {"rows": sort_rows(rows), "joined": joined, "joined_parts": joined_parts,
            "final_parts": (rows, parts)}


# ---------------- the hash-partition guarantee ----------------

def _expected_pids(rows, idx, dtypes, P):
    cols = []
    for i, dt in zip(idx, dtypes):
        vals = [r[i] for r in rows]
        valid = np.array([v is not None for v in vals], dtype=np.uint8)
        data = np.array([0 if v is None else v for v in vals], dtype=NP[dt])
        cols.append({"dtype": dt, "data": data, "valid": None if valid.all() else valid})
    return oracle.pids(oracle.hash_cols(cols, len(rows)), P).tolist()


def check_partitions(case, out):
    """Assert the hash-partition guarantee on a model or device result.

    A final row sits in the partition of its group key, NULL components included. A join's
    output row sits in the partition of its probe side's join key, or of its build side's
    where the probe side is absent (a side is present when one of its row ids is not NULL).
    A row whose key has a NULL component is checked only where both inputs of the join were
    shuffled on exactly the join keys (node["null_routed"]); it matches nothing wherever it
    sits. Returns the number of rows checked."""
    P = case["P"]
    checked = 0
    nodes = join_nodes(case["plan"])
    assert len(nodes) == len(out["joined_parts"])
    for node, (rows, parts) in zip(nodes, out["joined_parts"]):
        assert len(rows) == len(parts)
        schema = schema_of(case, node)
        by_side = {}
        for r, (row, p) in enumerate(zip(rows, parts)):
            probe = node["out_pkey"] is not None and \
                any(row[i] is not None for i in node["out_prid"])
            assert probe or any(row[i] is not None for i in node["out_brid"]), \
                f"join row {r} has neither side: {row}"
            key = node["out_pkey"] if probe else node["out_bkey"]
            if not node["null_routed"] and any(row[i] is None for i in key):
                continue
            by_side.setdefault(tuple(key), []).append((row, p))
        for key, items in by_side.items():
            want = _expected_pids([row for row, _ in items], key,
                                  [schema[i]["dtype"] for i in key], P)
            for (row, p), w in zip(items, want):
                assert p == w, f"join {node['type']}: row {row} sits in partition {p}, " \
                               f"its key hashes to {w}"
            checked += len(items)
    rows, parts = out["final_parts"]
    key_dtypes, _ = _agg_layout(case)
    if rows:
        want = _expected_pids(rows, range(len(key_dtypes)), key_dtypes, P)
        for row, p, w in zip(rows, parts, want):
            assert p == w, f"group {row} sits in partition {p}, its key hashes to {w}"
        assert len(set(r[:len(key_dtypes)] for r in rows)) == len(rows), \
            "a group came out of two partitions or twice"
    return checked + len(rows)
