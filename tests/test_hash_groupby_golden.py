"""tests/golden/hash_groupby.json -- the general GROUP BY as the reference answers it (make_golden_hashagg.py) -- against
the numpy restatement over the oracle's join result; the device is checked against the same fixture in
tests/test_gpu_sink_matrix.py."""
import os

import numpy as np

from common import GOLDEN, load_golden, orc
from joinref import HASHAGG_SQL, hashagg_groups, hashagg_inputs


def test_fixture_against_the_oracle_join():
    gold = load_golden("hash_groupby")
    assert gold["sql"] == HASHAGG_SQL and os.path.getsize(os.path.join(GOLDEN, "hash_groupby.json")) < 50_000
    fact, fact_valid, dim, dim_valid = hashagg_inputs(**gold["shape"])
    ht = orc.HashTable([dim["dk"]], [dim["g2"]], payload_valid=[dim_valid["g2"]])
    pcols = [fact["fk"], fact["g1"], fact["x"]]
    pvalid = [None, fact_valid["g1"], fact_valid["x"]]
    o = orc.run_pipeline(pcols, [orc.JoinSpec(ht, [(-1, 0)])], [[0]], routing="default_path", probe_valid=pvalid)
    rows = o["out_rows"]
    p, b = rows[:, 0], rows[:, 1]
    want = hashagg_groups(fact["g1"][p], fact_valid["g1"][p].astype(bool), dim["g2"][b], dim_valid["g2"][b].astype(bool),
                          fact["x"][p], fact_valid["x"][p].astype(bool))
    got = {(r[0], r[1]): r[2:] for r in gold["rows"]}
    assert len(got) == len(gold["rows"]) == len(want)
    assert got == want
    # the fixture has what it is for: NULL groups on both columns, sums beyond int64 on both sides
    assert any(k[0] is None for k in got) and any(k[1] is None for k in got)
    sums = [v[2] for v in got.values() if v[2] is not None]
    assert min(sums) < -(1 << 64) and max(sums) > (1 << 64)
    assert sum(v[0] for v in got.values()) == len(rows) and len(rows) > 10_000
