"""polr_pipeline_create as a user of the library meets it: what it refuses (status, the reason in last_error, and no device
memory left behind), and the tuple slots it plans -- 1 for joins keyed by probe columns, one more per build side a later
key is read through, one more for multiplicities -- on pipelines whose counts the pool launch then gets right.  The rules
themselves are checked without a GPU (tests/test_pipe_plan.py); build sides of 8 rows, a probe side of 16."""
import numpy as np
import pytest

from joinref import Join, Ref
from polr_amd import capi

pytestmark = pytest.mark.gpu

N = 16
C0 = (np.arange(N) % 10).astype(np.int32)         # keys of build side 0: 0..7 match, 8 and 9 do not
C1 = np.array([1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 1, 2, 3, 0], np.int32)
C2 = np.arange(N).astype(np.int64)
PCOLS = [C0, C1, C2]
B0 = Join(np.array([3, 0, 7, 1, 6, 2, 5, 4], np.int32), 0, payload=[np.array([10, 11, 12, 13, 14, 15, 99, 98], np.int32)])
B1 = Join(np.array([10, 11, 12, 13, 14, 15, 16, 17], np.int32), 3, payload=[np.arange(8).astype(np.int32)])  # (src: VIA0)
B2 = Join(np.array([1, 1, 2, 2, 2, 3, 5, 5], np.int32), 1)  # repeated keys
B3 = Join(np.array([1, 2, 3, 4, 9, 10, 11, 12], np.int32), 1)
B8 = Join(np.arange(8).astype(np.int64), 0)                 # an 8-byte key
# the column join 1 reads through join 0's build rows, spelled out per probe row (-1: no build row, no match either)
VIA0 = np.array([dict(zip(B0.keys.tolist(), B0.payload[0].tolist())).get(v, -1) for v in C0.tolist()], np.int32)

_state = {}


def _tables(ctx):
    if not _state:
        _state.update(b0=B0.device(ctx), b1=B1.device(ctx), b2=B2.device(ctx), b3=B3.device(ctx), b8=B8.device(ctx),
                      raw=capi.HashTable.from_columns(ctx, [B1.keys], B1.payload),
                      cond=B1.device(ctx))
        _state["cond"].preds = [("<", (-1, 2), 0)]  # an 8-byte probe column against the 4-byte payload column
        assert _state["b2"].info()["kind"] == 3
    return _state


def _probe_keyed(t):
    return [(t["b0"], [(-1, 0)]), (t["b2"], [(-1, 1)])]


def _chain(t):
    return [(t["b0"], [(-1, 0)]), (t["b1"], [(0, 0)])]


REFUSALS = [
    ("not_a_permutation", lambda t: (_probe_keyed(t), [[0, 0]]), capi.E_INVALID, "path 0 is not a permutation"),
    ("before_its_provider", lambda t: (_chain(t), [[0, 1], [1, 0]]), capi.E_INVALID,
     "path 1 probes join 1 before join 0 that provides its key"),
    ("not_finalized", lambda t: ([(t["b0"], [(-1, 0)]), (t["raw"], [(-1, 1)])], [[0, 1]]), capi.E_INVALID,
     "join 1: build side not finalized"),
    ("key_column_out_of_range", lambda t: ([(t["b0"], [(-1, 3)])], [[0]]), capi.E_INVALID,
     "join 0 key 0: probe column 3 out of range"),
    ("key_width_without_by_value", lambda t: ([(t["b0"], [(-1, 0)]), (t["b8"], [(-1, 1)])], [[0, 1]]), capi.E_INVALID,
     "join 1 key 0: probe key is 4 bytes, build key 8 bytes"),
    ("condition_width", lambda t: ([(t["cond"], [(-1, 0)])], [[0]]), capi.E_INVALID,
     "join 0 condition 0: left side is 8 bytes, right side 4 bytes"),
    ("nine_joins", lambda t: ([(t["b0"], [(-1, 0)])] * 9, [list(range(9))]), capi.E_UNSUPPORTED,
     "9 multiplexed joins not supported"),
    ("33_paths", lambda t: (_probe_keyed(t), [[0, 1], [1, 0]] * 16 + [[0, 1]]), capi.E_UNSUPPORTED,
     "33 join orders not supported"),
]


@pytest.mark.parametrize("make,code,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refused_and_nothing_leaks(gpu_ctx, make, code, text):
    joins, paths = make(_tables(gpu_ctx))
    live = capi.device_bytes_live()
    with pytest.raises(capi.PolrError) as e:
        capi.Pipeline(gpu_ctx, PCOLS, N, joins, paths)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)
    assert capi.device_bytes_live() == live


def test_tuple_slots_and_counts(gpu_ctx):
    t = _tables(gpu_ctx)
    ref_cols = PCOLS + [VIA0]
    cases = [
        # joins, the same joins for the reference, join orders (the run takes the first), tuple slots
        ([(t["b0"], [(-1, 0)]), (t["b3"], [(-1, 1)])], [B0, B3], [[1, 0], [0, 1]], 1),  # the probe row alone
        (_chain(t), [B0, B1], [[0, 1]], 2),                                             # + join 0's build row
        (_chain(t) + [(t["b2"], [(-1, 1)])], [B0, B1, B2], [[2, 0, 1], [0, 1, 2], [0, 2, 1]], 3),  # + multiplicity
        (_probe_keyed(t), [B0, B2], [[0, 1], [1, 0]], 2),                               # probe row + multiplicity
    ]
    for joins, rjoins, paths, slots in cases:
        pipe = capi.Pipeline(gpu_ctx, PCOLS, N, joins, paths)
        assert pipe.launch_info(False)["tuple_slots"] == slots, (paths, pipe.launch_info(False))
        want = Ref(ref_cols, None, rjoins).stage_counts(paths[0])
        assert want[-1] > 0
        m = capi.DeviceMultiplexer(pipe, "default_path")
        capi.run_resident([m], [(0, 1)], reset=True, finish=True)
        assert m.finish()["stage_out"][0] == want, paths
        m.close()
        pipe.close()
