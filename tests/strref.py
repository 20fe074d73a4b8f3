"""What the VARCHAR GROUP BY tests share: the nation names of the SSB-skew Q4.1 fixture with a real VARCHAR c_nation
(tests/golden/ssb_q41_varchar.json, made by tests/golden/make_golden_q41_varchar.py) and exact Python grouping by bytes."""
import numpy as np

# nation code -> name.  The five nations of region 1 (AMERICA, codes 5..9: the only ones Q4.1 keeps) hold what the string
# sink has to tell apart: names of at most 12 bytes (inline cells), names longer than 12 bytes (heap cells) that share the
# prefix "UNITED ST", and the 9-byte prefix itself as an inline name.
AMERICA = {5: b"ARGENTINA", 6: b"BRAZIL", 7: b"UNITED ST", 8: b"UNITED STATES", 9: b"UNITED STATES MINOR OUTLYING ISLANDS"}
NATION_NAMES = {c: AMERICA.get(c, b"NATION %02d OF REGION %d" % (c, c // 5)) for c in range(64)}  # (25 + the extra OCEANIA codes of load.sql)
NATION_CODES = {v: k for k, v in NATION_NAMES.items()}
NULL_EVERY = 37  # the `rows_nulls` run: c_nation IS NULL for every customer whose c_custkey is a multiple of this


def nation_names(codes):
    """c_nation codes -> the VARCHAR column (bytes per row)"""
    return [NATION_NAMES[int(c)] for c in np.asarray(codes).tolist()]


def nation_valid(custkeys):
    """validity of c_nation in the `rows_nulls` run"""
    return (np.asarray(custkeys).astype(np.int64) % NULL_EVERY != 0).astype(np.uint8)


def group_sum(keys, values):
    """GROUP BY the key tuples (bytes / int / None per column), SUM(values) as Python ints -> {key: sum}"""
    out = {}
    for k, v in zip(keys, values):
        out[k] = out.get(k, 0) + int(v)
    return out
