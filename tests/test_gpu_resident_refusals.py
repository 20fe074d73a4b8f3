"""What the resident pool launch refuses, and that a refusal leaves nothing behind: every call below fails with its
status (and names the reason) before it has changed any multiplexer or enqueued anything -- the ordinary run that follows
on the same multiplexers gives the fixture's COUNT(*) and routes every tuple.  SSB-skew Q4.1 sample (the flat pipeline);
the generic pipeline of tests/manyorders.py for the executors that do not fit."""
import pytest

import manyorders as mo
from polr_amd import capi
from test_gpu_many_join_orders import pipeline_for
from test_gpu_router_placement import _ranges, _ssb

pytestmark = pytest.mark.gpu

N_EXEC = 3
_state = {}


def _setup(ctx):
    if not _state:
        s = _ssb(ctx)
        generic = pipeline_for(ctx, "generic", 9)
        li = generic.launch_info()
        assert li["flat"] == 0
        # a sixteenth of the device holds `capacity` workgroups; this many executors need all of them as router workgroups
        capacity = li["n_cus"] * li["workgroups_per_cu"] // 16
        n_fit = capacity * li["waves_per_workgroup"]
        assert capacity >= 2 and n_fit <= 4096
        _state.update(s=s, n_chunks=(s["n"] + 1023) // 1024, generic=generic, n_fit=n_fit,
                      mpxs=[capi.DeviceMultiplexer(s["pipe"], "adaptive_reinit") for _ in range(N_EXEC)],
                      gmpxs=[capi.DeviceMultiplexer(generic, "adaptive_reinit") for _ in range(n_fit)],
                      foreign_out=capi.Output(generic, 1024, 64))
    return _state


def _twice(t):
    capi.run_resident([t["mpxs"][0], t["mpxs"][1], t["mpxs"][0]], _ranges(t["n_chunks"], 3), reset=True, finish=True)


def _too_many(t):
    capi.run_resident([t["mpxs"][0]] * 4097, [(0, 1)] * 4097, reset=True, finish=True)


def _foreign_output(t):
    capi.run_resident(t["mpxs"], _ranges(t["n_chunks"], N_EXEC), out=t["foreign_out"], reset=True, finish=True)


def _range_past_the_end(t):
    ranges = _ranges(t["n_chunks"], N_EXEC)
    ranges[-1] = (ranges[-1][0], t["n_chunks"] + 1)
    capi.run_resident(t["mpxs"], ranges, reset=True, finish=True)


def _share_17(t):
    capi.run_resident(t["mpxs"], _ranges(t["n_chunks"], N_EXEC), reset=True, finish=True, share=17)


def _no_ranges(t):
    capi.run_resident_ranges(t["mpxs"], [[] for _ in range(N_EXEC)], reset=True, finish=True)


def _nine_ranges(t):
    capi.run_resident_ranges(t["mpxs"], [[(0, 1)] * 9 for _ in range(N_EXEC)], reset=True, finish=True)


def _no_morsel(t):
    capi.run_resident_morsels(t["mpxs"], 0, t["n_chunks"], morsel_chunks=0, reset=True, finish=True)


def _do_not_fit(t):
    n = t["n_fit"]
    capi.run_resident(t["gmpxs"], _ranges((mo.N + 1023) // 1024, n), reset=True, finish=True, share=16)


REFUSALS = [
    (_twice, capi.E_INVALID, "twice"),
    (_too_many, capi.E_UNSUPPORTED, "4096"),
    (_foreign_output, capi.E_INVALID, "another pipeline"),
    (_range_past_the_end, capi.E_INVALID, "outside"),
    (_share_17, capi.E_INVALID, "at most 16"),
    (_no_ranges, capi.E_INVALID, None),
    (_nine_ranges, capi.E_INVALID, None),
    (_no_morsel, capi.E_INVALID, None),
    (_do_not_fit, capi.E_UNSUPPORTED, "do not fit"),
]


def _refused(t, call, code, text):
    with pytest.raises(capi.PolrError) as e:
        call(t)
    assert e.value.code == code, (call.__name__, str(e.value))
    if text is not None:
        assert text in str(e.value), (call.__name__, str(e.value))


@pytest.mark.parametrize("call,code,text", REFUSALS, ids=[r[0].__name__.lstrip("_") for r in REFUSALS])
def test_refused(gpu_ctx, call, code, text):
    _refused(_setup(gpu_ctx), call, code, text)


def test_refusals_enqueue_nothing_and_change_nothing(gpu_ctx):
    t = _setup(gpu_ctx)
    s = t["s"]
    for call, code, text in REFUSALS:
        _refused(t, call, code, text)
    for _ in range(2):
        capi.run_resident(t["mpxs"], _ranges(t["n_chunks"], N_EXEC), reset=True, finish=True)
        stats = capi.finish_many(t["mpxs"])
        k = s["k"]
        assert sum(sum(st["stage_out"][p][k - 1] for p in range(s["n_paths"])) for st in stats) == s["count_star"]
        assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == s["n"]
    # ... and the executors that did not fit on a sixteenth of the device run on the whole of it
    g = t["gmpxs"][:7]
    capi.run_resident(g, _ranges((mo.N + 1023) // 1024, len(g)), reset=True, finish=True)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in capi.finish_many(g)) == mo.N
