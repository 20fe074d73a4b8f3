"""How the pool launch cuts a round into units, restated in Python (polr_pool_unit_size, duckdb-polr_amd/csrc/polr_pool_plan.h;
tests/test_pool_units.py holds it against the table the plan program prints), and the source size at which one executor's
DEFAULT_PATH round runs in units of a stated size -- what tests/test_gpu_pool_units.py sizes its sources with."""

UNIT_MAX = 65536


def unit_size(tuples, pool_waves, active, gran, hi_tuples, units_x, hi_unit):
    """-> (tuples per unit, units) of a round of `tuples` tuples while `active` executors are still routing"""
    if tuples <= hi_tuples:
        unit = hi_unit
    else:
        target = max(16, units_x * pool_waves // max(active, 1))
        per_wave = (tuples + target - 1) // target
        unit = min(UNIT_MAX, (per_wave + gran - 1) // gran * gran)
    return unit, (tuples + unit - 1) // unit


def unit_of(rows, info, active=1):
    """the unit size of a round of `rows` tuples in a run whose polr_mpx_pool_info is `info`"""
    return unit_size(rows, info["pool_waves"], active, info["gran"], info["hi_tuples"], info["units_x"], info["hi_unit"])[0]


def source_rows_for(unit, info, units_x=None):
    """the most rows of a source that ONE executor's DEFAULT_PATH round (its whole range) still cuts into units of exactly
    `unit` tuples: target x unit.  (Down to target x (unit - gran) + 1 rows the unit stays the same; a unit of `gran`
    tuples needs more than hi_tuples rows besides.)  info: capi.pool_info of the run; units_x: what info was taken under"""
    x = info["units_x"] if units_x is None else units_x
    assert x == info["units_x"], "pool_info was taken under another tuning"
    assert unit % info["gran"] == 0 and info["gran"] <= unit <= UNIT_MAX
    target = max(16, x * info["pool_waves"])
    rows = target * unit
    assert rows > info["hi_tuples"] and rows < 2**32 - 16
    return rows
