#!/usr/bin/env python3
"""tests/golden/make_golden_many_orders.py -- the routing code with a FULL bank, from THE REFERENCE ITSELF: SSB-skew Q4.1
(4 joins) on the shape of ssb_skew_sample.json with `max_join_orders` 24 and an enumerator that fills the bank, so the
multiplexer routes over all 24 join orders.

  ALTERNATE matrix -> which join order sits at which index of the bank (each column equals the per-chunk intermediates of
                      exactly one permutation, identified with the oracle); kept as column sums + SHA-1, COUNT(*)
  routing traces   -> per-round intermediates of the six deterministic strategies, totals, per-path tuple counts
Should the reference refuse or fail at 24 orders, that is recorded instead ("refused": its message), and the fixture
holds no trace.  Build container only (needs oracle/_ref).  Output: tests/golden/many_join_orders.json"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ssb_skew as g  # noqa: E402  (run(): one reference run, its logs parsed; SHAPE; ROUTINGS)
from polr_amd import ssb_skew  # noqa: E402
import common  # noqa: E402

QUERY = "q4.1"
MAX_JOIN_ORDERS = 24
ENUMERATORS = ["dfs_min_card", "bfs_min_card", "dfs_random", "bfs_random"]  # the first that fills the bank is used


def digest(m):
    m = np.ascontiguousarray(m, dtype=np.uint64)
    return {"n_rows": int(m.shape[0]), "column_sums": [int(x) for x in m.sum(axis=0)],
            "sha1": hashlib.sha1(m.tobytes()).hexdigest()}


def main():
    wl = ssb_skew.workload(QUERY, **g.SHAPE)
    ref = wl["ref"]
    gold = {"shape": g.SHAPE, "query": QUERY, "max_join_orders": MAX_JOIN_ORDERS, "sql": ref["query"], "tried": {}}
    base = want = None
    for enumerator in ENUMERATORS:
        base = ["PRAGMA enable_polr", "PRAGMA enable_log_tuples_routed", "PRAGMA disable_caching",
                "SET join_enumerator TO '%s'" % enumerator, "SET max_join_orders TO %d" % MAX_JOIN_ORDERS]
        try:
            log, intms, counts, answer = g.run(ref, base + ["SET multiplexer_routing TO 'alternate'"])
        except RuntimeError as e:
            gold["tried"][enumerator] = {"refused": str(e)[-400:]}
            continue
        n_orders = 0 if log is None else len(g.parse_alt(log)[0])
        gold["tried"][enumerator] = {"n_join_orders": n_orders}
        if n_orders == MAX_JOIN_ORDERS:
            want = np.asarray(g.parse_alt(log), dtype=np.uint64)
            gold.update(join_enumerator=enumerator, count_star=answer, alternate={"digest": digest(want), "intms": intms})
            break
    path = os.path.join(HERE, "many_join_orders.json")
    if want is None:
        gold["refused"] = "no enumerator of the reference gave %d join orders" % MAX_JOIN_ORDERS
        json.dump(gold, open(path, "w"), separators=(",", ":"))
        print("wrote", path, "(the reference did not fill the bank)", gold["tried"])
        return
    pcols, pvalid, ojoins = common.oracle_joins(wl)
    k = len(ojoins)
    found = {}
    for perm in itertools.permutations(range(k)):
        res = common.orc.run_pipeline(pcols, ojoins, [list(perm)], routing="alternate", caching=False,
                                      collect_output=False)
        col = res["alt_matrix"][:, 0]
        for p in range(want.shape[1]):
            if np.array_equal(col, want[:, p]):
                found.setdefault(p, []).append(list(perm))
    assert all(len(found.get(p, [])) == 1 for p in range(want.shape[1])), found
    gold["paths"] = [found[p][0] for p in range(want.shape[1])]
    gold["routing"] = {}
    for routing in g.ROUTINGS:
        log, intms, counts, ans = g.run(ref, base + ["SET multiplexer_routing TO '%s'" % routing])
        assert ans == gold["count_star"]
        gold["routing"][routing] = {"rounds": g.parse_rounds(log), "intms": intms, "tuple_counts": counts}
        print(routing, len(gold["routing"][routing]["rounds"]), "rounds", intms, "intermediates", flush=True)
    json.dump(gold, open(path, "w"), separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes; enumerator", gold["join_enumerator"])


if __name__ == "__main__":
    main()
