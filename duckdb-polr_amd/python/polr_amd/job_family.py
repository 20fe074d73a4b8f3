"""BASELINE.json configs[3]: "Full JOB (imdb) 113 queries, independent POLR pipelines sharded across 8 GPUs".

The reference runs the 113 queries of the Join Order Benchmark over the IMDB snapshot (benchmark/imdb/*.benchmark,
SQL in benchmark/imdb_plan_cost/queries/*.sql); neither the data (fetched over the network by
benchmark/imdb/init/load.sql:1-21) nor the optimizer that turns each query into pipelines is available / in scope here.
What this module builds is the JOB-SHAPED FAMILY: for every one of the 113 queries ONE multiplexed pipeline that keeps
the query's join graph --

  * job_shapes.json (made from the SQL files by tools/make_job_shapes.py: tables, equi-join predicates, number and kind of
    filter predicates per table; no SQL text) gives the graph;
  * the probe side is the query's largest table (by IMDB cardinality); every other table that an equality chain
    connects to it becomes a hash join, keyed by a probe column where the equivalence class of the join column holds
    one, else by a build column of the join that leads to it (the dependent joins of
    POLARConfig::GenerateJoinOrders, src/parallel/polar_config.cpp:72-95), breadth first, at most 8 joins
    (POLR_MAX_JOINS; the reference multiplexes runs of consecutive joins inside one pipeline, a 17-table query is
    several pipelines there);
  * tables are synthetic at the IMDB cardinalities: dense ids, foreign keys power-law distributed over the parent's
    ids, filters thinned to a selectivity that depends only on the kinds of predicates the query puts on the table.

A query of more than 8 joins keeps all its tables in the CHAINED plan (chained_plan, run_chain_device): the same
breadth-first order cut into stages of at most 8 joins, the rows a stage emits being the source of the next
(polr_pipeline_from_output).  workload() and what bench.py runs are unchanged: the first eight joins.

Every pipeline is independent (own tables, own multiplexers): whole queries are dealt round-robin to the GPUs
(polr_amd.dist.shard_queries), nothing is exchanged.
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

CARD = {"title": 2_528_312, "cast_info": 36_244_344, "movie_info": 14_835_720, "movie_keyword": 4_523_930,
        "movie_companies": 2_609_129, "name": 4_167_491, "char_name": 3_140_339, "aka_name": 901_343,
        "aka_title": 361_472, "person_info": 2_963_664, "movie_info_idx": 1_380_035, "movie_link": 29_997,
        "complete_cast": 135_086, "keyword": 134_170, "company_name": 234_997, "info_type": 113, "kind_type": 7,
        "company_type": 4, "role_type": 12, "link_type": 18, "comp_cast_type": 4}
# foreign keys of the IMDB schema: (table, column) -> referenced table (its dense id)
FK = {("cast_info", "movie_id"): "title", ("cast_info", "person_id"): "name", ("cast_info", "person_role_id"): "char_name",
      ("cast_info", "role_id"): "role_type", ("movie_info", "movie_id"): "title",
      ("movie_info", "info_type_id"): "info_type", ("movie_info_idx", "movie_id"): "title",
      ("movie_info_idx", "info_type_id"): "info_type", ("movie_keyword", "movie_id"): "title",
      ("movie_keyword", "keyword_id"): "keyword", ("movie_companies", "movie_id"): "title",
      ("movie_companies", "company_id"): "company_name", ("movie_companies", "company_type_id"): "company_type",
      ("title", "kind_id"): "kind_type", ("aka_name", "person_id"): "name", ("aka_title", "movie_id"): "title",
      ("person_info", "person_id"): "name", ("person_info", "info_type_id"): "info_type",
      ("movie_link", "movie_id"): "title", ("movie_link", "linked_movie_id"): "title",
      ("movie_link", "link_type_id"): "link_type", ("complete_cast", "movie_id"): "title",
      ("complete_cast", "subject_id"): "comp_cast_type", ("complete_cast", "status_id"): "comp_cast_type"}
SMALL = 200  # tables of up to this many rows are enumerations: an equality keeps one of their rows
SEL = {"eq": 0.1, "like": 0.05, "notlike": 0.9, "ne": 0.95, "range": 0.3, "between": 0.2, "null": 0.1, "notnull": 0.9,
       "or": 0.15, "notin": 0.9}
MAX_JOINS = 8
SKEW = 1.4  # exponent of the foreign-key power law (1 = uniform)
_PRIMES = [2654435761, 2246822519, 3266489917, 668265263, 374761393, 2870177467, 1540483507, 2971215073]


def shapes():
    return json.load(open(os.path.join(_HERE, "job_shapes.json")))["queries"]


def _mix32(x, salt):
    """cheap deterministic hash -> [0, 1): which rows a filter keeps"""
    z = (x.astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    z ^= z >> np.uint64(31)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(29)
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def _salt(text):
    """process-independent salt of a name (Python's str hash is randomised per process)"""
    v = 7
    for ch in text:
        v = (v * 131 + ord(ch)) % 1_000_003
    return v + 3


def selectivity(table, n_rows, kinds):
    s = 1.0
    for kd in kinds:
        if kd.startswith("in"):
            n = int(kd[2:])
            s *= min(1.0, n / n_rows) if n_rows <= SMALL else min(0.05 * n, 0.5)
        elif kd == "eq" and n_rows <= SMALL:
            s *= 1.0 / n_rows
        else:
            s *= SEL[kd]
    return max(s, 1.0 / max(n_rows, 1))


class Tables:
    """the synthetic IMDB instance of one scale, columns made on demand and kept (every query reuses them)"""

    def __init__(self, scale=1.0, seed=1337):
        self.scale, self.seed = float(scale), int(seed)
        self._cols = {}

    def rows(self, table):
        n = CARD[table]
        return n if n <= SMALL else max(int(n * self.scale), 1000)

    def column(self, table, col):
        key = (table, col)
        if key in self._cols:
            return self._cols[key]
        n = self.rows(table)
        if col == "id":
            v = np.arange(1, n + 1, dtype=np.int32)
        elif key in FK:
            parent = self.rows(FK[key])
            rng = np.random.default_rng(np.random.SeedSequence([self.seed] + [ord(c) for c in table + "." + col]))
            idx = (parent * rng.random(n) ** SKEW).astype(np.int64)        # power law: few parents get most rows
            # scattered over the id space by a multiplier of the column's own (a bijection: the primes exceed every
            # table size), so that the hot parents of two referencing tables are different rows -- a join of two
            # foreign-key columns then fans out by about rows / parents, as in IMDB, not by hot x hot
            mult = _PRIMES[_salt(table + "." + col) % len(_PRIMES)]
            v = (1 + (idx * mult) % parent).astype(np.int32)
        else:
            # a join column that is not a declared foreign key (the queries equate e.g. two movie_id columns through
            # title): same construction over the table's own id space
            rng = np.random.default_rng(np.random.SeedSequence([self.seed] + [ord(c) for c in table + "." + col]))
            v = (1 + (n * rng.random(n) ** 2).astype(np.int64) % n).astype(np.int32)
        self._cols[key] = v
        return v

    def strings(self, table, col, rows=None):
        """a VARCHAR attribute column (title.title, name.name, movie_info.info ...): one string per row, a pure function
        of (table, column, row): lengths 3 .. 27 characters, so that both forms of a string_t cell occur (up to 12
        characters inline, longer ones through the heap); many rows share their first characters, so comparisons have
        to look past the 4-byte prefix.  rows: the row ids wanted (default: all)"""
        n = self.rows(table)
        ids = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        h = (_mix32(ids, _salt(table + "." + col)) * (1 << 24)).astype(np.int64)
        stem = (table[:2] + col[:2]).encode()
        words = [b"a", b"the", b"of", b"night", b"return", b"story", b"day", b"last"]
        out = []
        for i, x in zip(ids.tolist(), h.tolist()):
            v = stem + b"-" + words[x % 8] + b"-" + str(x % 9973).encode()
            if x & 0x100:
                v += b"-" + words[(x >> 9) % 8] + b"-" + str(i).encode()
            out.append(v)
        return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def pipeline_shape(q, max_joins=MAX_JOINS):
    """the multiplexed pipeline of one query shape: probe alias, its columns, and the ordered joins
    [(alias, build key column, key source ('probe', column) | (join index, column))]; max_joins=None: every table of
    the query, in the same breadth-first order (chained_plan cuts that order into pipelines)"""
    max_joins = len(q["tables"]) if max_joins is None else max_joins
    tables, joins = q["tables"], q["joins"]
    cols = sorted({(a, c) for j in joins for a, c in (tuple(j[0]), tuple(j[1]))})
    parent = {x: x for x in cols}
    for a, b in joins:
        ra, rb = _find(parent, tuple(a)), _find(parent, tuple(b))
        if ra != rb:
            parent[ra] = rb
    classes = {}
    for x in cols:
        classes.setdefault(_find(parent, x), []).append(x)
    probe = max(sorted(tables), key=lambda a: CARD[tables[a]])
    placed = {probe: -1}
    order = []
    frontier = True
    while frontier and len(order) < max_joins:
        frontier = False
        cands = []
        for cl in classes.values():
            inside = [x for x in cl if x[0] in placed]
            outside = [x for x in cl if x[0] not in placed]
            if not inside or not outside:
                continue
            # key source: a probe column of the class if there is one, else the earliest placed join's column
            src = min(inside, key=lambda x: (placed[x[0]], x[1]))
            for b in outside:
                cands.append((0 if src[0] == probe else 1, placed[src[0]], b[0], b[1], src))
        seen = set()
        for pri, _p, alias, bcol, src in sorted(cands):
            if alias in seen or alias in placed or len(order) >= max_joins:
                continue
            seen.add(alias)
            order.append((alias, bcol, src))
            placed[alias] = len(order) - 1
            frontier = True
    return probe, order


def workload(name, tables, q=None):
    """workload dict (the format of polr_amd.workloads) of query `name` over the synthetic instance `tables`"""
    q = q or shapes()[name]
    probe, order = pipeline_shape(q)
    if len(order) < 2:
        return None  # POLAR needs two consecutive joins (polar_config.cpp:44)
    ptable = q["tables"][probe]
    # probe columns: every probe column some join is keyed by, plus the filter column
    pcols = []
    for alias, bcol, src in order:
        if src[0] == probe and src[1] not in pcols:
            pcols.append(src[1])
    probe_cols = {c: tables.column(ptable, c) for c in pcols}
    n_probe = tables.rows(ptable)
    psel = selectivity(ptable, n_probe, q["filters"].get(probe, []))
    flt = None
    if psel < 1.0:
        f = (_mix32(np.arange(n_probe, dtype=np.int64), 17) * 1000).astype(np.int32)
        probe_cols["f"] = f
        cut = max(int(round(psel * 1000)), 1)
        flt = [("f", "<", cut)]
    names = list(probe_cols.keys())
    # payload columns of every join: the columns dependents are keyed by
    payload_cols = {a: [] for a, _b, _s in order}
    for alias, bcol, src in order:
        if src[0] != probe and src[1] not in payload_cols[src[0]]:
            payload_cols[src[0]].append(src[1])
    index_of = {a: i for i, (a, _b, _s) in enumerate(order)}
    joins = []
    for alias, bcol, src in order:
        t = q["tables"][alias]
        n = tables.rows(t)
        sel = selectivity(t, n, q["filters"].get(alias, []))
        keep = np.ones(n, dtype=bool) if sel >= 1.0 else (_mix32(np.arange(n, dtype=np.int64), _salt(alias)) < sel)
        if not keep.any():
            keep[0] = True
        key = tables.column(t, bcol)[keep]
        payload = {c: tables.column(t, c)[keep] for c in payload_cols[alias]}
        if src[0] == probe:
            key_src = [(-1, names.index(src[1]))]
        else:
            key_src = [(index_of[src[0]], payload_cols[src[0]].index(src[1]))]
        joins.append({"name": alias, "table": t, "keys": [key], "key_names": [bcol], "payload": payload,
                      "key_src": key_src, "perfect": None, "kept_rows": np.nonzero(keep)[0]})
    # BoundReference index of every join's probe-side condition in the original column layout
    cond_left = []
    for j in joins:
        sj, sc = j["key_src"][0]
        if sj < 0:
            cond_left.append([sc])
        else:
            cond_left.append([len(names) + sum(len(joins[i]["payload"]) for i in range(sj)) + sc])
    wl = {"name": "job_" + name, "probe": {"name": ptable, "cols": probe_cols}, "joins": joins,
          "cond_left_index": cond_left}
    # the query's select list, MIN(alias.column) ...: the columns of it that this pipeline's tables own, as VARCHAR columns
    # (wl["select"]: (join index or -1 for the probe table, column name); the strings of the rows kept, in "strings")
    select = []
    for alias, col in q.get("select", []):
        t = q["tables"][alias]
        if alias == probe:
            wl["probe"].setdefault("strings", {})[col] = tables.strings(t, col)
            select.append((-1, col))
        elif alias in index_of:
            j = joins[index_of[alias]]
            if col not in j.setdefault("strings", {}):
                j["strings"][col] = tables.strings(t, col, rows=j["kept_rows"])
            select.append((index_of[alias], col))
    wl["select"] = select
    if flt:
        wl["probe"]["filter"] = flt
        wl["probe"]["filter_sel"] = np.nonzero(probe_cols["f"] < flt[0][2])[0].astype(np.uint32)
    wl["ref"] = _reference_form(probe, probe_cols, flt, order, joins, select, wl["probe"].get("strings"))
    return wl


def _reference_form(probe, probe_cols, flt, order, joins, select=(), probe_strings=None):
    """how the same pipeline reads for the reference (as SQL over uploaded tables): one table per alias -- the probe table with its
    filter column, every build side with the rows its filters keep -- and the joins as a left-deep chain in pipeline order,
    pinned with `SET disabled_optimizers TO 'join_order,...'`: the plan the reference executes is then one pipeline whose
    source is the probe table and whose consecutive INNER hash joins are exactly these joins, so POLARConfig
    (src/parallel/polar_config.cpp:19-71) multiplexes all of them."""
    def tname(alias):
        return "t_" + alias

    def cname(alias, col):
        return "%s__%s" % (alias, col)

    tables = {tname(probe): {cname(probe, c): a for c, a in probe_cols.items()}}
    for c, vals in (probe_strings or {}).items():
        tables[tname(probe)][cname(probe, c)] = vals
    sql = "SELECT COUNT(*) FROM %s" % tname(probe)
    for (alias, bcol, src), j in zip(order, joins):
        cols = {cname(alias, bcol): j["keys"][0]}
        for c, a in j["payload"].items():
            if c != bcol:
                cols[cname(alias, c)] = a
        for c, vals in j.get("strings", {}).items():
            cols[cname(alias, c)] = vals
        tables[tname(alias)] = cols
        sql += " JOIN %s ON %s = %s" % (tname(alias), cname(src[0], src[1]), cname(alias, bcol))
    if flt:
        sql += " WHERE " + " AND ".join("%s %s %d" % (cname(probe, c), op, const) for c, op, const in flt)
    # (statistics propagation is switched off with the join order optimizer: on a reduced instance it finds build sides
    # whose key ranges miss the probe side's, and replaces such a join -- and with it the pipeline -- by an empty result)
    out = {"tables": tables, "pk": {}, "query": sql,
           "settings": ["SET disabled_optimizers TO 'join_order,statistics_propagation'"]}
    if select:
        aliases = [probe] + [a for a, _b, _s in order]
        out["query_select"] = sql.replace("SELECT COUNT(*)", "SELECT " + ", ".join(
            "MIN(%s)" % cname(aliases[1 + sj], c) for sj, c in select))
    return out


# ---- the query's own sink, fused into the run ------------------------------------------------------------------------------------
def fused_select_on_build_sides(wl):
    """the whole select list of the workload lies on build sides (a probe-side VARCHAR column has no code column: such a
    query keeps the materialising route and polr_out_aggregate_string)"""
    return all(sj >= 0 for sj, _c in wl["select"])


def run_fused_device(ctx, wl, paths, routing="adaptive_reinit", chunk_capacity=1024, probe_dictionary=False):
    """SELECT COUNT(*), MIN(a), MIN(b), ... of a workload whose select list lies on build sides, in ONE pool launch and
    without an output to size: every select column becomes a sorted dictionary code column of its build side (DICT_SORTED |
    DICT_NULL_INVALID: the order of the codes is the order of the strings, a NULL string an invalid code), the output
    carries a fused ungrouped sink -- COUNT(*) and MIN(code column) per select column --, one resident run fills it, and
    the winning codes are turned back into strings (HashTable.dictionary_strings).
    probe_dictionary=True: a select column of the PROBE table is uploaded as a string probe column and, after the scan
    filter, encoded over the selection in force (Pipeline.encode_dictionary: DICT_SORTED | DICT_NULL_INVALID |
    DICT_SELECTED); its MIN is the MIN of that code column, turned back by Pipeline.dictionary_strings.  Without it such a
    workload is refused, as before.
    -> {"count_star": int, "select_min": [bytes or None] in the order of wl["select"], "rows_written": rows of the output}"""
    from . import capi
    if not probe_dictionary and not fused_select_on_build_sides(wl):
        raise ValueError("the select list names a probe-side column: polr_out_aggregate_string over emitted row ids")
    # (the caller's workload stays as it is: the joins are shallow copies that carry the dictionary request)
    wl = dict(wl, joins=[dict(j) for j in wl["joins"]])
    for j in wl["joins"]:
        j["dictionary"] = list(j.get("dictionary") or [])
        j["dictionary_flags"] = dict(j.get("dictionary_flags") or {})
    for sj, col in wl["select"]:
        if sj < 0:
            continue
        j = wl["joins"][sj]
        if col not in j["dictionary"]:
            j["dictionary"].append(col)
        j["dictionary_flags"][col] = capi.DICT_SORTED | capi.DICT_NULL_INVALID
    handles = []  # everything made here, closed in reverse order whatever happens
    try:
        joins = capi.build_joins(ctx, wl, auto=True)
        handles += [ht for ht, _ in joins]
        cols = list(wl["probe"]["cols"].values())
        names = list(wl["probe"]["cols"].keys())
        # the probe table's select columns: string_t cells behind the key columns, and their heaps
        pstr = {c: capi.string_cells(wl["probe"]["strings"][c]) for c in dict.fromkeys(c for sj, c in wl["select"] if sj < 0)}
        pipe = capi.Pipeline(ctx, cols + [cells for cells, _h in pstr.values()], len(cols[0]), joins, paths)
        handles.append(pipe)
        for i, (_cells, heap) in enumerate(pstr.values()):
            pipe.set_probe_heap(len(cols) + i, heap)
        flt = wl["probe"].get("filter")
        if flt:
            _n, n_chunks = pipe.scan_filter([(names.index(c), op, const) for c, op, const in flt])
        else:
            n_chunks = (len(cols[0]) + 1023) // 1024
        # ... encoded over the rows the filter kept, and no others
        pcode = {c: pipe.encode_dictionary(len(cols) + i, sorted=True, null_invalid=True, selected=True)[0] for i, c in enumerate(pstr)}
        out = capi.Output(pipe, chunk_capacity, 1)  # (nothing is written: the smallest output there is)
        handles.append(out)
        code_cols = [pcode[col] if sj < 0 else capi.dictionary_payload_index(wl["joins"][sj], col)[0] for sj, col in wl["select"]]
        out.fuse_aggregate([("count_star", -1, 0)] + [("min", sj, cc) for (sj, _c), cc in zip(wl["select"], code_cols)])
        mpx = capi.DeviceMultiplexer(pipe, routing)
        handles.append(mpx)
        if flt:
            mpx.use_scan_chunks()
        capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
        mpx.finish()
        res = out.fused_aggregate_result()
        mins = []
        for (sj, _c), cc, code in zip(wl["select"], code_cols, res[1:]):
            holder = pipe if sj < 0 else joins[sj][0]
            mins.append(None if code is None else holder.dictionary_strings(cc, [code])[0])
        return {"count_star": res[0], "select_min": mins, "rows_written": out.stats()[0]}
    finally:
        for h in reversed(handles):
            h.close()


# ---- chained plan: a query of more than MAX_JOINS joins as several pipelines --------------------------------------------------
def chained_plan(q, max_joins=MAX_JOINS):
    """The whole query as STAGES of at most max_joins joins each, in the family's breadth-first order: stage 0 probes the
    query's largest table, the rows a stage emits are the source of the next (polr_pipeline_from_output), so every table of
    the query is joined.  Each stage is multiplexed on its own.  ->
      {"probe": alias, "order": [(alias, build key column, (source alias, column))] over all joins, "select": [(alias, col)],
       "stages": [{"joins":   indices into order,
                   "source":  [(alias, column, "int" | "str")] the stage's probe-side columns -- columns of the probe table
                              for stage 0, the columns carried out of the previous stage otherwise,
                   "key_src": per join (-1, source column index) or (local join index, payload column index),
                   "payload": per join [(column, "int" | "str")] the build columns it carries,
                   "carry":   [(-1 | local join index, column index)] the columns handed to the next stage, in the order of
                              its "source"; for the last stage the select-list columns}],
       "final": [(alias, column, "str")] what the last stage's "carry" names: the select list, each column once, sorted}
    Carried are the key columns of later stages (probe columns or build columns of earlier joins) and the select-list
    columns ("str": VARCHAR).  A query of at most max_joins joins is one stage whose joins and keys are pipeline_shape's."""
    probe, order = pipeline_shape(q, None)
    select = [(a, c) for a, c in q.get("select", []) if a == probe or any(a == o[0] for o in order)]
    stage_of = {probe: -1}
    for i, (alias, _b, _s) in enumerate(order):
        stage_of[alias] = i // max_joins
    n_stages = max((len(order) + max_joins - 1) // max_joins, 1)
    # what is read of every alias, and by the stage that reads it last: keys (int) and select-list columns (str, read "after" the last stage)
    needs = {}
    for i, (_alias, _b, src) in enumerate(order):
        needs.setdefault((src[0], src[1], "int"), []).append(i // max_joins)
    for a, c in select:
        needs.setdefault((a, c, "str"), []).append(n_stages)
    stages = []
    source = sorted(x for x in needs if x[0] == probe)
    for s in range(n_stages):
        idx = list(range(s * max_joins, min((s + 1) * max_joins, len(order))))
        local = {order[i][0]: j for j, i in enumerate(idx)}
        payload = [sorted((c, kd) for (a, c, kd), users in needs.items() if a == order[i][0] and max(users) >= s) for i in idx]
        key_src = []
        for i in idx:
            a, c = order[i][2]
            key_src.append((-1, source.index((a, c, "int"))) if stage_of[a] < s else (local[a], payload[local[a]].index((c, "int"))))
        nxt = sorted(x for x, users in needs.items() if stage_of[x[0]] <= s and max(users) > s)
        carry = [(-1, source.index(x)) if stage_of[x[0]] < s else (local[x[0]], payload[local[x[0]]].index((x[1], x[2]))) for x in nxt]
        stages.append({"joins": idx, "source": source, "key_src": key_src, "payload": payload, "carry": carry})
        source = nxt
    return {"probe": probe, "order": order, "select": select, "stages": stages, "final": source}


def chain_data(plan, tables, q, sel_floor=0.0):
    """the tables of a chained plan over the synthetic instance: the probe table's columns and filter selection, and per
    join the rows its filters keep, its key and the columns it carries -- exactly as workload() thins them.  sel_floor: no
    table's filters keep less than this fraction of its rows -- for reduced instances, where the product of a dozen
    selectivities over tables of a thousand rows would leave no row at all"""
    probe = plan["probe"]
    ptable = q["tables"][probe]
    n_probe = tables.rows(ptable)
    psel = max(selectivity(ptable, n_probe, q["filters"].get(probe, [])), sel_floor)
    sel = None
    if psel < 1.0:
        f = (_mix32(np.arange(n_probe, dtype=np.int64), 17) * 1000).astype(np.int32)
        sel = np.nonzero(f < max(int(round(psel * 1000)), 1))[0].astype(np.uint32)
    src0 = []
    for a, c, kd in plan["stages"][0]["source"]:
        src0.append(tables.column(ptable, c) if kd == "int" else tables.strings(ptable, c))
    joins = []
    for st in plan["stages"]:
        for i, pay in zip(st["joins"], st["payload"]):
            alias, bcol, _src = plan["order"][i]
            t = q["tables"][alias]
            n = tables.rows(t)
            s = max(selectivity(t, n, q["filters"].get(alias, [])), sel_floor)
            keep = np.ones(n, dtype=bool) if s >= 1.0 else (_mix32(np.arange(n, dtype=np.int64), _salt(alias)) < s)
            if not keep.any():
                keep[0] = True
            rows = np.nonzero(keep)[0]
            joins.append({"alias": alias, "table": t, "kept_rows": rows, "key": tables.column(t, bcol)[keep],
                          "payload": [tables.column(t, c)[keep] if kd == "int" else tables.strings(t, c, rows=rows) for c, kd in pay]})
    return {"n_probe": n_probe, "sel": sel, "source": src0, "joins": joins}


def run_chain_host(plan, data, run_stage):
    """the stages one by one on the host: run_stage(int source columns, [(build key, [int payload columns], (src_join,
    src_col))], selection or None) -> (rows [n_out, 1 + k]: source row and the build row of every join, intermediates) runs one
    pipeline (the tests pass the oracle); the carried columns are gathered in numpy between the stages ->
    {"count": COUNT(*), "mins": the select list's MINs in the order of plan["final"] (bytes, None without a row),
     "int_mins": MIN of every integer source column of the last stage -- the carried keys -- over the result rows,
     "intermediates": per stage, "stage_rows": output rows per stage}"""
    source = [np.asarray(c, dtype=object) if isinstance(c, list) else c for c in data["source"]]
    sel = data["sel"]
    inter, stage_rows = [], []
    for st in plan["stages"]:
        kinds = [kd for _a, _c, kd in st["source"]]
        int_at = [i for i, kd in enumerate(kinds) if kd == "int"]  # the pipeline sees the integer columns only
        int_pay = [[x for x, (_n, kd) in enumerate(pay) if kd == "int"] for pay in st["payload"]]
        joins = []
        for j, i in enumerate(st["joins"]):
            d = data["joins"][i]
            sj, sc = st["key_src"][j]
            joins.append((d["key"], [d["payload"][x] for x in int_pay[j]],
                          (-1, int_at.index(sc)) if sj < 0 else (sj, int_pay[sj].index(sc))))
        rows, n_inter = run_stage([source[i] for i in int_at], joins, sel)
        inter.append(int(n_inter))
        stage_rows.append(len(rows))
        nxt = []
        for sj, sc in st["carry"]:
            if sj < 0:
                nxt.append(source[sc][rows[:, 0]])
            else:
                col = data["joins"][st["joins"][sj]]["payload"][sc]
                col = np.asarray(col, dtype=object) if isinstance(col, list) else col
                nxt.append(col[rows[:, 1 + sj]])
        if st is plan["stages"][-1]:
            int_mins = [int(source[i][rows[:, 0]].min()) if len(rows) else None for i in int_at]
        source, sel = nxt, None
    mins = [min(c.tolist()) if len(c) else None for c in source]
    return {"count": stage_rows[-1], "mins": mins, "int_mins": int_mins, "intermediates": inter, "stage_rows": stage_rows}


def run_chain_device(ctx, plan, data, chunk_capacity=1024):
    """the stages on the device: stage 0 is an ordinary pipeline over the probe table, every later stage is
    Pipeline.from_output of the stage before it over its carried columns; the select list's MINs come from the string sink of
    the last stage's output.  Each stage runs its first join order over all its tuples (polr_probe_rounds): once counting,
    which sizes the output, once emitting.  -> as run_chain_host, plus "flat": polr_pipeline_launch_info per stage"""
    from . import capi
    out = pipe = None
    hts = []
    keep = []
    n_tuples = len(data["sel"]) if data["sel"] is not None else data["n_probe"]
    inter, stage_rows, flat = [], [], []
    for s, st in enumerate(plan["stages"]):
        joins = []
        for j, i in enumerate(st["joins"]):
            d = data["joins"][i]
            cols, heaps = [], {}
            for x, (c, (_n, kd)) in enumerate(zip(d["payload"], st["payload"][j])):
                if kd == "str":
                    cells, heap = capi.string_cells(c)
                    keep.append((cells, heap))
                    heaps[x] = heap
                    c = cells
                cols.append(c)
            ht = capi.HashTable.from_columns(ctx, [d["key"]], cols)
            for x, heap in heaps.items():
                ht.set_payload_heap(x, heap)
            ht.finalize_auto(int(d["key"].min()), int(d["key"].max()))
            joins.append((ht, [st["key_src"][j]]))
        k = len(joins)
        paths = [list(range(k))]
        if s == 0:
            cols, heaps = [], {}
            for x, c in enumerate(data["source"]):
                if isinstance(c, list):
                    cells, heap = capi.string_cells(c)
                    keep.append((cells, heap))
                    heaps[x] = heap
                    c = cells
                cols.append(c)
            new = capi.Pipeline(ctx, cols, data["n_probe"], joins, paths)
            for x, heap in heaps.items():
                new.set_probe_heap(x, heap)
            if data["sel"] is not None:
                new.set_selection(data["sel"])
        else:
            new = capi.Pipeline.from_output(out, plan["stages"][s - 1]["carry"], joins, paths)
            # the stage before it is done with: the new pipeline owns its source
            out.close()
            pipe.close()
            for h in hts:
                h.close()
        pipe, hts = new, [h for h, _ in joins]
        flat.append(pipe.launch_info()["flat"])
        n_out = n_inter = 0
        if n_tuples:
            counts = pipe.probe_rounds([(0, n_tuples, 0, 0)])
            n_out, n_inter = int(counts[0][k - 1]), int(counts.sum())
        out = capi.Output(pipe, chunk_capacity, n_out // chunk_capacity + 1 + 8192)  # (a partly filled chunk per emitting wave)
        if n_tuples:
            pipe.probe_rounds([(0, n_tuples, 0, 1)], out=out)
        if out.stats()[0] != n_out:
            raise RuntimeError("stage %d: %d rows emitted, %d counted" % (s, out.stats()[0], n_out))
        inter.append(n_inter)
        stage_rows.append(n_out)
        n_tuples = n_out
    mins = [out.aggregate_string("min", sj, sc) if n_tuples else None for sj, sc in plan["stages"][-1]["carry"]]
    ints = [("min", -1, i) for i, (_a, _c, kd) in enumerate(plan["stages"][-1]["source"]) if kd == "int"]
    int_mins = out.aggregate(ints) if n_tuples and ints else [None] * len(ints)
    out.close()
    pipe.close()
    for h in hts:
        h.close()
    return {"count": stage_rows[-1], "mins": mins, "int_mins": int_mins, "intermediates": inter, "stage_rows": stage_rows,
            "flat": flat}


def run_chain_fused_device(ctx, plan, data, chunk_capacity=1024, routing="adaptive_reinit"):
    """run_chain_device with the LAST stage fused: its carried select columns become sorted code columns (DICT_SORTED |
    DICT_NULL_INVALID) -- a column of one of the stage's build sides through HashTable.encode_dictionary before the table is
    finalized, a column carried into the stage through Pipeline.encode_dictionary on the pipeline from_output made -- and
    the stage's output carries a fused ungrouped sink: COUNT(*) and MIN(code column) per select column.  ONE pool launch
    runs that stage: no counting run, no sized output, no string sink.  The stages before it run as in run_chain_device.
    -> {"count", "mins" in the order of plan["final"], "stage_rows" (the last: COUNT(*)), "intermediates" (of the last stage:
    what the multiplexer counted), "rows_written": rows in the last stage's output (0)}"""
    from . import capi
    last = len(plan["stages"]) - 1
    if 1 + len(plan["stages"][-1]["carry"]) > 8:
        raise ValueError("a fused sink holds 8 aggregates: COUNT(*) and at most 7 select columns")
    out = pipe = None
    hts, keep = [], []
    n_tuples = len(data["sel"]) if data["sel"] is not None else data["n_probe"]
    inter, stage_rows = [], []
    try:
        for s, st in enumerate(plan["stages"]):
            fused = s == last
            encode = {sj: {} for sj, _sc in st["carry"] if sj >= 0} if fused else {}  # join -> {payload column: code column}
            joins = []
            for j, i in enumerate(st["joins"]):
                d = data["joins"][i]
                cols, heaps = [], {}
                for x, (c, (_n, kd)) in enumerate(zip(d["payload"], st["payload"][j])):
                    if kd == "str":
                        cells, heap = capi.string_cells(c)
                        keep.append((cells, heap))
                        heaps[x] = heap
                        c = cells
                    cols.append(c)
                ht = capi.HashTable.from_columns(ctx, [d["key"]], cols)
                hts.append(ht)
                for x, heap in heaps.items():
                    ht.set_payload_heap(x, heap)
                for sj, sc in st["carry"] if fused else ():
                    if sj == j and sc not in encode[j]:
                        encode[j][sc] = ht.encode_dictionary(sc, sorted=True, null_invalid=True)[0]
                ht.finalize_auto(int(d["key"].min()), int(d["key"].max()))
                joins.append((ht, [st["key_src"][j]]))
            k = len(joins)
            paths = [list(range(k))]
            if s == 0:
                cols, heaps = [], {}
                for x, c in enumerate(data["source"]):
                    if isinstance(c, list):
                        cells, heap = capi.string_cells(c)
                        keep.append((cells, heap))
                        heaps[x] = heap
                        c = cells
                    cols.append(c)
                new = capi.Pipeline(ctx, cols, data["n_probe"], joins, paths)
                for x, heap in heaps.items():
                    new.set_probe_heap(x, heap)
                if data["sel"] is not None:
                    new.set_selection(data["sel"])
            else:
                new = capi.Pipeline.from_output(out, plan["stages"][s - 1]["carry"], joins, paths)
                # the stage before it is done with: the new pipeline owns its source
                out.close()
                pipe.close()
                for h in hts[:-k]:
                    h.close()
                hts = hts[-k:]
            pipe, out = new, None
            if not fused:
                n_out = n_inter = 0
                if n_tuples:
                    counts = pipe.probe_rounds([(0, n_tuples, 0, 0)])
                    n_out, n_inter = int(counts[0][k - 1]), int(counts.sum())
                out = capi.Output(pipe, chunk_capacity, n_out // chunk_capacity + 1 + 8192)  # (a partly filled chunk per emitting wave)
                if n_tuples:
                    pipe.probe_rounds([(0, n_tuples, 0, 1)], out=out)
                if out.stats()[0] != n_out:
                    raise RuntimeError("stage %d: %d rows emitted, %d counted" % (s, out.stats()[0], n_out))
                inter.append(n_inter)
                stage_rows.append(n_out)
                n_tuples = n_out
                continue
            # the last stage: the carried select columns as code columns, COUNT(*) and their MINs folded inside one launch
            if not n_tuples:  # (no row reached it: nothing to launch)
                return {"count": 0, "mins": [None] * len(st["carry"]), "intermediates": inter + [0], "stage_rows": stage_rows + [0],
                        "rows_written": 0}
            pcode = {}
            for sj, sc in st["carry"]:
                if sj < 0 and sc not in pcode:
                    pcode[sc] = pipe.encode_dictionary(sc, sorted=True, null_invalid=True, selected=True)[0]
            code_cols = [pcode[sc] if sj < 0 else encode[sj][sc] for sj, sc in st["carry"]]
            out = capi.Output(pipe, chunk_capacity, 1)  # (nothing is written: the smallest output there is)
            out.fuse_aggregate([("count_star", -1, 0)] + [("min", sj, cc) for (sj, _sc), cc in zip(st["carry"], code_cols)])
            mpx = capi.DeviceMultiplexer(pipe, routing)
            try:
                capi.run_resident([mpx], [(0, (n_tuples + 1023) // 1024)], out=out, reset=True, finish=True)
                inter.append(int(mpx.finish()["num_intermediates"]))
            finally:
                mpx.close()
            res = out.fused_aggregate_result()
            mins = []
            for (sj, _sc), cc, code in zip(st["carry"], code_cols, res[1:]):
                holder = pipe if sj < 0 else joins[sj][0]
                mins.append(None if code is None else holder.dictionary_strings(cc, [code])[0])
            stage_rows.append(int(res[0]))
            return {"count": stage_rows[-1], "mins": mins, "intermediates": inter, "stage_rows": stage_rows,
                    "rows_written": out.stats()[0]}
    finally:
        for h in [out, pipe] + hts:
            if h is not None:
                h.close()
