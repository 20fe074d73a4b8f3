// tests/pipeplan/pipe_plan_main.cpp -- the plan behind polr_pipeline_create (duckdb-polr_amd/csrc/polr_pipeline_plan.h) as
// a stand-alone host program: known answers, worked out by hand from the rules as they stood inside polr_pipeline_create,
// build_stage_descs and plan_flat before the plan became a function of its own; every refusal with its code and its
// whole message; and the invariants the device code relies on over a seeded sweep of random valid pipelines.  Prints one
// line per check group and "ok"; any mismatch is printed and makes the exit status 1.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_pipeline_plan.h"

static int failures = 0;
static unsigned checks = 0;

#define CHECK(cond_, ...)                                                                                              \
	do {                                                                                                               \
		checks++;                                                                                                      \
		if (!(cond_)) {                                                                                                \
			printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond_);                                                   \
			printf(__VA_ARGS__);                                                                                       \
			printf("\n");                                                                                              \
			failures++;                                                                                                \
		}                                                                                                              \
	} while (0)

static unsigned group_done(const char *name) {
	const unsigned n = checks;
	printf("%s: %u checks\n", name, n);
	checks = 0;
	return n;
}

// ---- building inputs -------------------------------------------------------------------------------------------------
static const void *fresh_table() {
	static uintptr_t n = 0;
	return (const void *)(++n * 4096);
}

// a finalized build side with one signed 4-byte key read from probe column `col`; payload: column 0 of 4 bytes, column 1
// of 8 bytes, column 2 of 16 bytes (strings).  Perfect: keys 0..99.  Hash: 1024 slots; S16: runs of up to 3 rows
static PipePlanJoin join_on_probe(uint32_t kind, int32_t col) {
	PipePlanJoin t = PipePlanJoin();
	t.kind = kind;
	t.n_keys = 1;
	t.key_width[0] = 4;
	t.key_signed = 1;
	t.cols = {{4, 1}, {8, 1}, {16, 0}};
	if (kind == KIND_PERFECT) {
		t.max_value = 99;
		t.range = 99;
	} else {
		t.capacity = 1024;
		t.max_run = kind == KIND_S16 ? 3 : 1;
	}
	t.table = fresh_table();
	t.desc.n_keys = 1;
	t.desc.key_src_join[0] = -1;
	t.desc.key_src_col[0] = col;
	return t;
}

static PipePlanJoin perfect_range(int32_t col, uint64_t range) {
	PipePlanJoin t = join_on_probe(KIND_PERFECT, col);
	t.max_value = (int64_t)range;
	t.range = range;
	return t;
}

static void key_from(PipePlanJoin &t, int32_t sj, int32_t sc) {
	t.desc.key_src_join[0] = sj;
	t.desc.key_src_col[0] = sc;
}

static void add_pred(PipePlanJoin &t, uint32_t op, int32_t sj, int32_t sc, uint32_t build_col) {
	const uint32_t c = t.desc.n_preds++;
	t.desc.pred_op[c] = op;
	t.desc.pred_src_join[c] = sj;
	t.desc.pred_src_col[c] = sc;
	t.desc.pred_build_col[c] = build_col;
}

struct Pipe {
	PipePlanInput in;
	std::vector<int32_t> paths;
	PipePlan plan;
	int run() {
		in.paths = paths.data();
		return polr_pipeline_plan(in, plan);
	}
};

// probe columns 0..2: 4 bytes signed, 3: 8 bytes signed, 4: 16 bytes (strings), 5: 2 bytes signed; 16 rows; one path,
// the joins in index order; 4 KB of LDS queues per wave of the flat kernel
static Pipe pipe_of(const std::vector<PipePlanJoin> &joins) {
	Pipe p;
	p.in = PipePlanInput();
	p.in.probe_cols = {{4, 1}, {4, 1}, {4, 1}, {8, 1}, {16, 0}, {2, 1}};
	p.in.n_probe_rows = 16;
	p.in.k = (uint32_t)joins.size();
	p.in.n_paths = 1;
	p.in.joins = joins;
	p.in.flat_wave_bytes = 4096;
	for (uint32_t j = 0; j < p.in.k; j++) {
		p.paths.push_back((int32_t)j);
	}
	return p;
}

static bool slots_are(const PipeSlots &s, uint32_t W, std::vector<int32_t> want) {
	want.resize(POLR_KMAX, -1);
	bool same = s.W == W;
	for (uint32_t j = 0; j < POLR_KMAX; j++) {
		same = same && s.slot_of_join[j] == want[j];
	}
	return same;
}

// ---- known answers ---------------------------------------------------------------------------------------------------
static void slots() {
	{ // three joins keyed by probe columns: nothing is carried
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_S8, 1), join_on_probe(KIND_S16, 2)});
		CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
		CHECK(slots_are(p.plan.count, 1, {-1, -1, -1}), "W %u", p.plan.count.W);
		CHECK(slots_are(p.plan.mat, 4, {1, 2, 3}), "W %u", p.plan.mat.W);
	}
	{ // join 1 keyed by payload column 0 of join 0
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S8, 0)});
		key_from(p.in.joins[1], 0, 0);
		CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
		CHECK(slots_are(p.plan.count, 2, {1, -1}), "W %u", p.plan.count.W);
		CHECK(slots_are(p.plan.mat, 3, {1, 2}), "W %u", p.plan.mat.W);
		const PipeSource &s = p.plan.joins[1].key[0];
		CHECK(s.join == 0 && s.col == 0 && s.width == 4 && s.sx == 1, "source (%d,%d) %u %u", s.join, s.col, s.width, s.sx);
		const PipeSource &s0 = p.plan.joins[0].key[0];
		CHECK(s0.join == -1 && s0.col == 0 && s0.width == 4 && s0.sx == 1, "source (%d,%d) %u %u", s0.join, s0.col, s0.width,
		      s0.sx);
	}
	{ // a condition, not a key, is the only reader of join 0: its 8-byte payload column 1 < join 1's own column 1
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S8, 1)});
		add_pred(p.in.joins[1], POLR_CMP_LT, 0, 1, 1);
		CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
		CHECK(slots_are(p.plan.count, 2, {1, -1}), "W %u", p.plan.count.W);
		const PipeSource &s = p.plan.joins[1].pred[0];
		CHECK(s.join == 0 && s.col == 1 && s.width == 8 && s.sx == 1, "source (%d,%d) %u %u", s.join, s.col, s.width, s.sx);
		CHECK(p.plan.joins[0].ext == 0 && p.plan.joins[1].ext == 1, "ext %u %u", p.plan.joins[0].ext, p.plan.joins[1].ext);
	}
	{ // join 1's condition and join 2's key both read join 0: one slot
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S8, 1), join_on_probe(KIND_S8, 2)});
		add_pred(p.in.joins[1], POLR_CMP_GE, 0, 0, 0);
		key_from(p.in.joins[2], 0, 0);
		CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
		CHECK(slots_are(p.plan.count, 2, {1, -1, -1}), "W %u", p.plan.count.W);
	}
	{ // join index order, a join's keys before its conditions: join 1's condition reads join 2 (slot 1), then join 3's key
	  // reads join 1 (slot 2) before its condition reads join 0 (slot 3)
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S8, 1), join_on_probe(KIND_S8, 2),
		                  join_on_probe(KIND_S8, 0)});
		add_pred(p.in.joins[1], POLR_CMP_NE, 2, 0, 0);
		add_pred(p.in.joins[3], POLR_CMP_EQ, 0, 0, 0);
		key_from(p.in.joins[3], 1, 0);
		p.paths = {0, 2, 1, 3};
		CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
		CHECK(slots_are(p.plan.count, 4, {3, 2, 1, -1}), "W %u", p.plan.count.W);
		CHECK(slots_are(p.plan.mat, 5, {1, 2, 3, 4}), "W %u", p.plan.mat.W);
	}
	{ // a packed composite key needs the extension record, conditions or not
		Pipe p = pipe_of({join_on_probe(KIND_S16, 0)});
		p.in.joins[0].packed = 1;
		CHECK(p.run() == POLR_OK && p.plan.joins[0].ext == 1, "ext %u", p.plan.joins[0].ext);
	}
	group_done("slots");
}

static void mult_and_unique() {
	{ // a repeating S16 join nobody reads
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S16, 1)});
		CHECK(p.run() == POLR_OK && p.plan.mult == 1, "mult %u", p.plan.mult);
		CHECK(p.plan.flat == 0, "flat %u", p.plan.flat);
	}
	{ // ... with a condition
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S16, 1)});
		add_pred(p.in.joins[1], POLR_CMP_LT, -1, 2, 0);
		CHECK(p.run() == POLR_OK && p.plan.mult == 0, "mult %u", p.plan.mult);
	}
	{ // ... read by a later key
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S16, 1), join_on_probe(KIND_S8, 0)});
		key_from(p.in.joins[2], 1, 0);
		CHECK(p.run() == POLR_OK && p.plan.mult == 0, "mult %u", p.plan.mult);
		CHECK(slots_are(p.plan.count, 2, {-1, 1, -1}), "W %u", p.plan.count.W);
	}
	{ // all unique; and what "unique" is: a perfect table, KIND_S8 (whatever max_run says), or a longest run of at most 1
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_S8, 1), join_on_probe(KIND_S16, 2),
		                  join_on_probe(KIND_S16, 0), join_on_probe(KIND_S16, 1)});
		p.in.joins[0].max_run = 7;
		p.in.joins[1].max_run = 7;
		p.in.joins[2].max_run = 1;
		p.in.joins[3].max_run = 0;
		p.in.joins[4].max_run = 1;
		CHECK(p.run() == POLR_OK && p.plan.mult == 0, "mult %u", p.plan.mult);
		for (uint32_t j = 0; j < 5; j++) {
			CHECK(p.plan.joins[j].unique == 1, "join %u: unique %u", j, p.plan.joins[j].unique);
		}
		p.in.joins[4].max_run = 2;
		CHECK(p.run() == POLR_OK && p.plan.mult == 1 && p.plan.joins[4].unique == 2, "mult %u unique %u", p.plan.mult,
		      p.plan.joins[4].unique);
		// the materialising variant never folds: there is one mult, the counting variant's
		CHECK(p.plan.joins[3].unique == 1, "unique %u", p.plan.joins[3].unique);
	}
	group_done("mult and unique");
}

static uint32_t flat_of(Pipe &p) {
	CHECK(p.run() == POLR_OK, "%s", p.plan.msg);
	return p.plan.flat * 2 + p.plan.flat_emit; // 0: generic, 2: flat, 3: flat and emitting runs too
}

static void flat() {
	{
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_PERFECT, 1)});
		CHECK(flat_of(p) == 3, "two perfect tables");
		CHECK(p.plan.flat_wpb == 16, "wpb %u", p.plan.flat_wpb);
	}
	{ // six joins at most
		std::vector<PipePlanJoin> six(6, join_on_probe(KIND_PERFECT, 0)), seven(7, join_on_probe(KIND_PERFECT, 0));
		Pipe p6 = pipe_of(six), p7 = pipe_of(seven);
		CHECK(flat_of(p6) == 3, "k = 6");
		CHECK(flat_of(p7) == 0, "k = 7");
		CHECK(p7.plan.flat_wpb == 0 && p7.plan.n_lds_tables == 0 && p7.plan.joins[0].lds_off1 == 0, "k = 7: nothing flat is set");
	}
	{ // an 8-byte key
		Pipe p = pipe_of({join_on_probe(KIND_S8, 3)});
		p.in.joins[0].key_width[0] = 8;
		CHECK(flat_of(p) == 0, "8-byte key");
	}
	{ // two key columns
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0)});
		PipePlanJoin &t = p.in.joins[0];
		t.n_keys = t.desc.n_keys = 2;
		t.key_width[1] = 4;
		t.desc.key_src_join[1] = -1;
		t.desc.key_src_col[1] = 1;
		CHECK(flat_of(p) == 0, "two key columns");
	}
	{ // a key read through a build column
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_PERFECT, 0)});
		key_from(p.in.joins[1], 0, 0);
		CHECK(flat_of(p) == 0, "key through a build column");
	}
	{ // a condition
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0)});
		add_pred(p.in.joins[0], POLR_CMP_LT, -1, 1, 0);
		CHECK(flat_of(p) == 0, "a condition");
	}
	{ // a signed perfect table: min down to -2^31
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0)});
		PipePlanJoin &t = p.in.joins[0];
		t.min_value = -2147483648ll;
		t.max_value = t.min_value + 99;
		CHECK(flat_of(p) == 3, "signed min -2^31");
		t.min_value = -2147483649ll;
		t.max_value = t.min_value + 99;
		CHECK(flat_of(p) == 0, "signed min -2^31 - 1");
		t.min_value = 2147483548ll;
		t.max_value = 2147483647ll;
		CHECK(flat_of(p) == 3, "signed max 2^31 - 1");
		t.max_value = 2147483648ll;
		t.range = 100;
		CHECK(flat_of(p) == 0, "signed max 2^31");
	}
	{ // an unsigned perfect table: max up to 2^32 - 1, min from 0
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0)});
		PipePlanJoin &t = p.in.joins[0];
		t.key_signed = 0;
		t.min_value = 4294967196ll;
		t.max_value = 4294967295ll;
		CHECK(flat_of(p) == 3, "unsigned max 2^32 - 1");
		t.max_value = 4294967296ll;
		t.range = 100;
		CHECK(flat_of(p) == 0, "unsigned max 2^32");
		t.min_value = -1;
		t.max_value = 98;
		t.range = 99;
		CHECK(flat_of(p) == 0, "unsigned min -1");
		// the whole domain: flat, but far too large for LDS
		t.min_value = 0;
		t.max_value = 4294967295ll;
		t.range = 0xFFFFFFFFull;
		CHECK(flat_of(p) == 3 && p.plan.n_lds_tables == 0 && p.plan.joins[0].lds_off1 == 0, "the whole unsigned domain");
		t.range = 0x100000000ull;
		CHECK(flat_of(p) == 0, "range 2^32");
	}
	{
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_S16, 1)});
		p.in.joins[1].max_run = 1;
		CHECK(flat_of(p) == 0, "KIND_S16, unique keys or not");
	}
	{ // KIND_S8: up to 2^31 slots
		Pipe p = pipe_of({join_on_probe(KIND_S8, 0)});
		p.in.joins[0].capacity = 1ull << 31;
		CHECK(flat_of(p) == 2, "capacity 2^31");
		p.in.joins[0].capacity = 1ull << 32;
		CHECK(flat_of(p) == 0, "capacity 2^32");
	}
	{ // perfect + S8: flat, but emitting runs take the generic pipeline
		Pipe p = pipe_of({join_on_probe(KIND_PERFECT, 0), join_on_probe(KIND_S8, 1)});
		CHECK(flat_of(p) == 2, "mixed");
		CHECK(p.plan.n_lds_tables == 1 && p.plan.lds_table_join[0] == 0 && p.plan.joins[0].lds_off1 == 1 &&
		          p.plan.joins[1].lds_off1 == 0,
		      "the hash table stays in HBM");
	}
	group_done("flat");
}

static void lds_tables() {
	// 4 KB per wave: 16 waves, budget min(64 KB, 156 KB - 64 KB) = 64 KB = 16384 dwords
	{ // smallest first.  Ranges 999, 99, 40: 32, 4 and 2 dwords
		Pipe p = pipe_of({perfect_range(0, 999), perfect_range(1, 99), perfect_range(2, 40)});
		const PipePlan &pl = p.plan;
		CHECK(flat_of(p) == 3 && pl.flat_wpb == 16 && pl.n_lds_tables == 3, "%u tables", pl.n_lds_tables);
		CHECK(pl.lds_table_join[0] == 2 && pl.lds_table_off[0] == 0 && pl.lds_table_len[0] == 2, "table 0");
		CHECK(pl.lds_table_join[1] == 1 && pl.lds_table_off[1] == 4 && pl.lds_table_len[1] == 4, "table 1");
		CHECK(pl.lds_table_join[2] == 0 && pl.lds_table_off[2] == 8 && pl.lds_table_len[2] == 32, "table 2");
		CHECK(pl.lds_table_dwords == 40, "%u dwords", pl.lds_table_dwords);
		CHECK(pl.joins[0].lds_off1 == 9 && pl.joins[1].lds_off1 == 5 && pl.joins[2].lds_off1 == 1, "lds_off1 %u %u %u",
		      pl.joins[0].lds_off1, pl.joins[1].lds_off1, pl.joins[2].lds_off1);
	}
	{ // the same build side joined twice: one copy
		Pipe p = pipe_of({perfect_range(0, 99), perfect_range(1, 99)});
		p.in.joins[1].table = p.in.joins[0].table;
		const PipePlan &pl = p.plan;
		CHECK(flat_of(p) == 3 && pl.n_lds_tables == 1 && pl.lds_table_dwords == 4, "%u tables, %u dwords", pl.n_lds_tables,
		      pl.lds_table_dwords);
		CHECK(pl.joins[0].lds_off1 == 1 && pl.joins[1].lds_off1 == 1, "lds_off1 %u %u", pl.joins[0].lds_off1, pl.joins[1].lds_off1);
	}
	{ // padded to 4 dwords: ranges 160 and 200 are 6 and 7 dwords, 8 each
		Pipe p = pipe_of({perfect_range(0, 200), perfect_range(1, 160)});
		const PipePlan &pl = p.plan;
		CHECK(flat_of(p) == 3 && pl.n_lds_tables == 2 && pl.lds_table_dwords == 16, "%u tables, %u dwords", pl.n_lds_tables,
		      pl.lds_table_dwords);
		CHECK(pl.lds_table_len[0] == 6 && pl.lds_table_off[0] == 0 && pl.lds_table_len[1] == 7 && pl.lds_table_off[1] == 8, "padding");
		CHECK(pl.joins[0].lds_off1 == 9 && pl.joins[1].lds_off1 == 1, "lds_off1 %u %u", pl.joins[0].lds_off1, pl.joins[1].lds_off1);
	}
	{ // exactly the budget fits, one dword more does not: 16380 + 4 dwords, then 16380 + 8
		Pipe p = pipe_of({perfect_range(0, 16380 * 32 - 1), perfect_range(1, 99)});
		CHECK(flat_of(p) == 3 && p.plan.n_lds_tables == 2 && p.plan.lds_table_dwords == 16384, "%u dwords", p.plan.lds_table_dwords);
		p.in.joins[1] = perfect_range(1, 129); // 5 dwords, padded 8
		CHECK(flat_of(p) == 3 && p.plan.n_lds_tables == 1 && p.plan.lds_table_dwords == 8 && p.plan.joins[0].lds_off1 == 0,
		      "%u tables, %u dwords", p.plan.n_lds_tables, p.plan.lds_table_dwords);
	}
	{ // the walk ENDS at the first table over budget (20000 dwords).  Join 2 names join 0's table but claims a larger range
	  // than join 1 (so that it sorts behind it): it would share join 0's copy, were the walk to go on
		Pipe p = pipe_of({perfect_range(0, 99), perfect_range(1, 20000 * 32 - 1), perfect_range(2, 700000)});
		p.in.joins[2].table = p.in.joins[0].table;
		const PipePlan &pl = p.plan;
		CHECK(flat_of(p) == 3 && pl.n_lds_tables == 1 && pl.lds_table_dwords == 4, "%u tables, %u dwords", pl.n_lds_tables,
		      pl.lds_table_dwords);
		CHECK(pl.joins[0].lds_off1 == 1 && pl.joins[1].lds_off1 == 0 && pl.joins[2].lds_off1 == 0, "lds_off1 %u %u %u",
		      pl.joins[0].lds_off1, pl.joins[1].lds_off1, pl.joins[2].lds_off1);
	}
	{ // waves per workgroup: 16 while 16 waves' queues fit 120 KB (7680 bytes each), else 8 (15360), else 4
		static const struct {
			size_t per_wave;
			uint32_t wpb;
		} W[] = {{2048, 16}, {7680, 16}, {7681, 8}, {15360, 8}, {15361, 4}, {40000, 4}};
		for (const auto &w : W) {
			Pipe p = pipe_of({join_on_probe(KIND_S8, 0)});
			p.in.flat_wave_bytes = w.per_wave;
			CHECK(flat_of(p) == 2 && p.plan.flat_wpb == w.wpb, "%zu bytes per wave: wpb %u", w.per_wave, p.plan.flat_wpb);
		}
	}
	{ // the budget: 16 waves of 7680 bytes leave 156 KB - 120 KB = 9216 dwords; 16 waves of 4096 bytes 16384 (the 64 KB
	  // cap); 8 or 4 waves 16 KB = 4096 dwords
		static const struct {
			size_t per_wave;
			uint64_t words;
			uint32_t fits;
		} B[] = {{7680, 9216, 1},  {7680, 9217, 0}, {4096, 10000, 1}, {4096, 16384, 1}, {4096, 16385, 0},
		         {7681, 4096, 1},  {7681, 4097, 0}, {7681, 5000, 0},  {7680, 5000, 1},  {15361, 4096, 1},
		         {15361, 4097, 0}, {1024, 16384, 1}, {1024, 16385, 0}};
		for (const auto &b : B) {
			Pipe p = pipe_of({perfect_range(0, b.words * 32 - 1)});
			p.in.flat_wave_bytes = b.per_wave;
			CHECK(flat_of(p) == 3 && p.plan.n_lds_tables == b.fits, "%zu bytes per wave, %llu dwords: %u tables", b.per_wave,
			      (unsigned long long)b.words, p.plan.n_lds_tables);
		}
	}
	group_done("lds tables");
}

// ---- refusals: one input per defect, the code and the whole message ------------------------------------------------------
static void refused(Pipe p, int code, const char *msg) {
	const int rc = p.run();
	CHECK(rc == code && p.plan.code == code && strcmp(p.plan.msg, msg) == 0, "want %d \"%s\", got %d \"%s\"", code, msg, rc,
	      p.plan.msg);
}
static void accepted(Pipe p) {
	CHECK(p.run() == POLR_OK && p.plan.code == POLR_OK && p.plan.msg[0] == 0, "%d \"%s\"", p.plan.code, p.plan.msg);
}

static Pipe two() {
	return pipe_of({join_on_probe(KIND_S8, 0), join_on_probe(KIND_S8, 1)});
}

static void refusals() {
	Pipe p;
	// 1. argument limits
	p = two(); p.in.k = 0; p.in.joins.clear();
	refused(p, POLR_E_UNSUPPORTED, "0 multiplexed joins not supported (1..8)");
	p = two(); p.in.k = 9; p.in.joins.clear();
	refused(p, POLR_E_UNSUPPORTED, "9 multiplexed joins not supported (1..8)");
	p = two(); p.in.n_paths = 0;
	refused(p, POLR_E_UNSUPPORTED, "0 join orders not supported (1..32)");
	p = two(); p.in.n_paths = 33;
	refused(p, POLR_E_UNSUPPORTED, "33 join orders not supported (1..32)");
	p = two(); p.in.n_probe_rows = 0xFFFFFFF0ull;
	refused(p, POLR_E_UNSUPPORTED, "probe side of 4294967280 rows exceeds the 32-bit row-id space per shard");
	p = two(); p.in.n_probe_rows = 0xFFFFFFEFull;
	accepted(p);
	{ // 8 joins and 32 join orders are fine
		Pipe w = pipe_of(std::vector<PipePlanJoin>(8, join_on_probe(KIND_S8, 0)));
		w.in.n_paths = 32;
		w.paths.clear();
		for (uint32_t q = 0; q < 32; q++) {
			for (uint32_t j = 0; j < 8; j++) {
				w.paths.push_back((int32_t)((j + q) % 8));
			}
		}
		accepted(w);
	}
	// 2. the descriptors, join by join
	p = two(); p.in.joins[1] = PipePlanJoin();
	refused(p, POLR_E_INVALID, "join 1: build side not finalized");
	p = two(); p.in.joins[0].desc.n_keys = 2;
	refused(p, POLR_E_INVALID, "join 0: 2 probe keys for a 1-key table");
	p = two(); p.in.joins[0].desc.n_keys = p.in.joins[0].n_keys = 0;
	refused(p, POLR_E_INVALID, "join 0: 0 probe keys for a 0-key table");
	p = two(); p.in.joins[1].desc.n_keys = p.in.joins[1].n_keys = 5;
	refused(p, POLR_E_INVALID, "join 1: 5 probe keys for a 5-key table");
	p = two(); p.in.joins[0].desc.n_preds = 5;
	refused(p, POLR_E_UNSUPPORTED, "join 0: 5 non-equality conditions (at most 4)");
	p = two(); key_from(p.in.joins[1], 2, 0);
	refused(p, POLR_E_INVALID, "join 1 key 0: reads a build column of join 2");
	p = two(); key_from(p.in.joins[1], 1, 0);
	refused(p, POLR_E_INVALID, "join 1 key 0: reads a build column of join 1");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_LT, 0, 0, 0);
	refused(p, POLR_E_INVALID, "join 0 condition 0: reads a build column of join 0");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_LT, -1, 0, 0); add_pred(p.in.joins[0], POLR_CMP_LT, 5, 0, 0);
	refused(p, POLR_E_INVALID, "join 0 condition 1: reads a build column of join 5");
	// 3. the paths
	p = two(); p.paths = {0, 0};
	refused(p, POLR_E_INVALID, "path 0 is not a permutation of the 2 joins");
	p = two(); p.paths = {1, -1};
	refused(p, POLR_E_INVALID, "path 0 is not a permutation of the 2 joins");
	p = two(); p.in.n_paths = 2; p.paths = {1, 0, 0, 2};
	refused(p, POLR_E_INVALID, "path 1 is not a permutation of the 2 joins");
	p = two(); key_from(p.in.joins[1], 0, 0); p.in.n_paths = 2; p.paths = {0, 1, 1, 0};
	refused(p, POLR_E_INVALID, "path 1 probes join 1 before join 0 that provides its key");
	p = two(); add_pred(p.in.joins[1], POLR_CMP_LT, 0, 0, 0); p.paths = {1, 0};
	refused(p, POLR_E_INVALID, "path 0 probes join 1 before join 0 that a condition of it reads");
	// 4. the columns, join by join
	p = two(); p.in.joins[1].device = 1;
	refused(p, POLR_E_INVALID, "join 1: build side lives on another device");
	p = two(); key_from(p.in.joins[0], -1, 6);
	refused(p, POLR_E_INVALID, "join 0 key 0: probe column 6 out of range");
	p = two(); key_from(p.in.joins[0], -1, -1);
	refused(p, POLR_E_INVALID, "join 0 key 0: probe column -1 out of range");
	p = two(); key_from(p.in.joins[1], 0, 3);
	refused(p, POLR_E_INVALID, "join 1 key 0: build column (0,3) out of range");
	p = two(); key_from(p.in.joins[1], 0, -2);
	refused(p, POLR_E_INVALID, "join 1 key 0: build column (0,-2) out of range");
	p = two(); p.in.joins[0].key_width[0] = 8;
	refused(p, POLR_E_INVALID, "join 0 key 0: probe key is 4 bytes, build key 8 bytes (a CAST'ed key: polr_ht_set_key_flags(..., "
	                           "POLR_KEY_BY_VALUE) before the table is finalized)");
	p = two(); p.in.joins[0].key_width[0] = 8; p.in.joins[0].key_flags[0] = POLR_KEY_BY_VALUE;
	accepted(p);
	p = two(); key_from(p.in.joins[1], 0, 1); // (the 8-byte payload column of join 0 against a 4-byte key)
	refused(p, POLR_E_INVALID, "join 1 key 0: probe key is 8 bytes, build key 4 bytes (a CAST'ed key: polr_ht_set_key_flags(..., "
	                           "POLR_KEY_BY_VALUE) before the table is finalized)");
	p = two(); key_from(p.in.joins[0], -1, 4); p.in.joins[0].key_flags[0] = POLR_KEY_BY_VALUE;
	refused(p, POLR_E_UNSUPPORTED, "join 0 key 0: probe key of 16 bytes");
	p = two(); key_from(p.in.joins[0], -1, 4); p.in.joins[0].key_width[0] = 16;
	refused(p, POLR_E_UNSUPPORTED, "join 0 key 0: probe key of 16 bytes");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_IS_NULL, -1, 1, 0);
	refused(p, POLR_E_UNSUPPORTED, "join 0 condition 0: comparison 6 (EQ, NE, LT, GT, LE, GE, STR_EQ)");
	p = two(); add_pred(p.in.joins[0], 9, -1, 1, 0);
	refused(p, POLR_E_UNSUPPORTED, "join 0 condition 0: comparison 9 (EQ, NE, LT, GT, LE, GE, STR_EQ)");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_LT, -1, 1, 3);
	refused(p, POLR_E_INVALID, "join 0 condition 0: build column 3 out of range");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_LT, -1, 6, 0);
	refused(p, POLR_E_INVALID, "join 0 condition 0: probe column 6 out of range");
	p = two(); add_pred(p.in.joins[1], POLR_CMP_LT, 0, 3, 0);
	refused(p, POLR_E_INVALID, "join 1 condition 0: build column (0,3) out of range");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_STR_EQ, -1, 0, 2);
	refused(p, POLR_E_INVALID,
	        "join 0 condition 0: STR_EQ compares two columns of 16-byte string cells (left 4 bytes, right 16 bytes)");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_STR_EQ, -1, 4, 1);
	refused(p, POLR_E_INVALID,
	        "join 0 condition 0: STR_EQ compares two columns of 16-byte string cells (left 16 bytes, right 8 bytes)");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_STR_EQ, -1, 4, 2);
	accepted(p);
	p = two(); add_pred(p.in.joins[0], POLR_CMP_LT, -1, 0, 1);
	refused(p, POLR_E_INVALID, "join 0 condition 0: left side is 4 bytes, right side 8 bytes");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_EQ, -1, 4, 2);
	refused(p, POLR_E_INVALID, "join 0 condition 0: left side is 16 bytes, right side 16 bytes");
	p = two(); add_pred(p.in.joins[0], POLR_CMP_GE, -1, 3, 1);
	accepted(p);
	// the order of the passes: descriptors of ALL joins, then the paths, then the columns
	p = two(); p.in.joins[0].device = 1; p.in.joins[1] = PipePlanJoin();
	refused(p, POLR_E_INVALID, "join 1: build side not finalized");
	p = two(); p.in.joins[0].device = 1; p.paths = {1, 1};
	refused(p, POLR_E_INVALID, "path 0 is not a permutation of the 2 joins");
	p = two(); key_from(p.in.joins[0], -1, 6); p.in.joins[1].desc.n_preds = 5;
	refused(p, POLR_E_UNSUPPORTED, "join 1: 5 non-equality conditions (at most 4)");
	group_done("refusals");
}

// ---- invariants over random valid pipelines ------------------------------------------------------------------------------
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { // 0..n-1
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}

static void invariants() {
	static const size_t PER_WAVE[] = {1024, 4096, 7680, 7681, 15360, 15361};
	unsigned plans = 0, n_flat = 0, n_emit = 0, n_mult = 0, n_tables = 0, n_shared = 0;
	for (uint32_t it = 0; it < 4000; it++) {
		const uint32_t k = 1 + rnd(8);
		// rank[j]: a join reads build columns only of joins of lower rank, so every order by rank is a legal path
		uint32_t rank[POLR_KMAX];
		for (uint32_t j = 0; j < k; j++) {
			rank[j] = j;
		}
		for (uint32_t j = k; j > 1; j--) {
			std::swap(rank[j - 1], rank[rnd(j)]);
		}
		const uint32_t read_pct = rnd(3) * 15; // many pipelines read nothing through a build column (flat candidates)
		auto pick_source = [&](uint32_t j, int32_t &sj, int32_t &sc) {
			sj = -1;
			sc = (int32_t)rnd(3);
			if (rnd(100) < read_pct) {
				const uint32_t o = rnd(k);
				if (rank[o] < rank[j]) {
					sj = (int32_t)o;
					sc = 0; // (the 4-byte payload column)
				}
			}
		};
		std::vector<PipePlanJoin> joins;
		bool reads[POLR_KMAX] = {};
		for (uint32_t j = 0; j < k; j++) {
			const uint32_t kinds[] = {KIND_PERFECT, KIND_PERFECT, KIND_S8, KIND_S16};
			PipePlanJoin t = join_on_probe(kinds[rnd(read_pct ? 4 : 3)], 0);
			if (t.kind == KIND_PERFECT) {
				t.range = 1 + rnd(rnd(2) ? 400000 : 4000);
				t.max_value = (int64_t)t.range;
				if (j && rnd(4) == 0 && joins[j - 1].kind == KIND_PERFECT) { // the same build side once more
					const polr_join_desc d = t.desc;
					t = joins[j - 1];
					t.desc = d;
				}
			}
			t.max_run = rnd(3);
			pick_source(j, t.desc.key_src_join[0], t.desc.key_src_col[0]);
			if (rnd(100) < read_pct) {
				int32_t sj, sc;
				pick_source(j, sj, sc);
				add_pred(t, rnd(6), sj, sc, 0);
			}
			if (t.desc.key_src_join[0] >= 0) {
				reads[t.desc.key_src_join[0]] = true;
			}
			if (t.desc.n_preds && t.desc.pred_src_join[0] >= 0) {
				reads[t.desc.pred_src_join[0]] = true;
			}
			joins.push_back(t);
		}
		Pipe p = pipe_of(joins);
		p.in.flat_wave_bytes = PER_WAVE[rnd(6)];
		p.in.n_paths = 1 + rnd(32);
		p.paths.clear();
		for (uint32_t q = 0; q < p.in.n_paths; q++) {
			// a random order that respects the dependencies: of the joins not yet placed, any whose sources are all placed
			uint32_t placed = 0;
			for (uint32_t pos = 0; pos < k; pos++) {
				uint32_t ready[POLR_KMAX], n_ready = 0;
				for (uint32_t j = 0; j < k; j++) {
					const polr_join_desc &d = joins[j].desc;
					const bool key_ok = d.key_src_join[0] < 0 || ((placed >> d.key_src_join[0]) & 1);
					const bool pred_ok = !d.n_preds || d.pred_src_join[0] < 0 || ((placed >> d.pred_src_join[0]) & 1);
					if (!((placed >> j) & 1) && key_ok && pred_ok) {
						ready[n_ready++] = j;
					}
				}
				const uint32_t j = ready[rnd(n_ready)];
				p.paths.push_back((int32_t)j);
				placed |= 1u << j;
			}
		}
		const int before = failures;
		const PipePlan &pl = p.plan;
		CHECK(p.run() == POLR_OK, "%s", pl.msg);
		plans++;
		// counting slots: distinct, inside 1..W-1, and exactly the joins some key or condition reads have one
		uint32_t used = 0, n_read = 0;
		bool slots_ok = true;
		for (uint32_t j = 0; j < POLR_KMAX; j++) {
			const int32_t s = pl.count.slot_of_join[j];
			const bool wants = j < k && reads[j];
			n_read += wants;
			slots_ok = slots_ok && (s >= 0) == wants;
			if (s >= 0) {
				slots_ok = slots_ok && s >= 1 && (uint32_t)s < pl.count.W && !((used >> s) & 1);
				used |= 1u << s;
			}
			slots_ok = slots_ok && pl.mat.slot_of_join[j] == (j < k ? (int32_t)(1 + j) : -1);
		}
		CHECK(slots_ok && pl.count.W == 1 + n_read && pl.mat.W == 1 + k, "slots: W %u, %u joins read", pl.count.W, n_read);
		CHECK((!pl.flat_emit || pl.flat) && (!pl.flat || pl.count.W == 1) && (!pl.mult || !pl.flat), "flat %u emit %u W %u mult %u",
		      pl.flat, pl.flat_emit, pl.count.W, pl.mult);
		// LDS tables: in ascending offsets without overlap, inside the budget; a join's lds_off1 - 1 is the offset of the
		// table that is its build side's
		const size_t per_wave = p.in.flat_wave_bytes;
		const uint32_t wpb = per_wave * 16 <= 120 * 1024 ? 16 : (per_wave * 8 <= 120 * 1024 ? 8 : 4);
		size_t budget = 16 * 1024;
		if (wpb == 16) {
			budget = 156 * 1024 - per_wave * 16 < 64 * 1024 ? 156 * 1024 - per_wave * 16 : 64 * 1024;
		}
		bool lds_ok = pl.flat || (pl.n_lds_tables == 0 && pl.lds_table_dwords == 0 && pl.flat_wpb == 0);
		lds_ok = lds_ok && (!pl.flat || pl.flat_wpb == wpb) && pl.n_lds_tables <= POLR_KMAX;
		uint32_t end = 0;
		for (uint32_t t = 0; t < pl.n_lds_tables && lds_ok; t++) {
			const PipePlanJoin &src = joins[pl.lds_table_join[t]];
			lds_ok = src.kind == KIND_PERFECT && pl.lds_table_off[t] >= end && pl.lds_table_off[t] % 4 == 0 &&
			         pl.lds_table_len[t] == (src.range + 32) / 32;
			end = pl.lds_table_off[t] + pl.lds_table_len[t];
		}
		lds_ok = lds_ok && end <= pl.lds_table_dwords && (size_t)pl.lds_table_dwords * 4 <= budget;
		for (uint32_t j = 0; j < k && lds_ok; j++) {
			const uint32_t off1 = pl.joins[j].lds_off1;
			if (off1) {
				bool found = false;
				for (uint32_t t = 0; t < pl.n_lds_tables; t++) {
					if (pl.lds_table_off[t] == off1 - 1) {
						found = joins[pl.lds_table_join[t]].table == joins[j].table;
						n_shared += found && pl.lds_table_join[t] != j;
					}
				}
				lds_ok = found;
			}
		}
		CHECK(lds_ok, "LDS tables: %u tables, %u dwords, budget %zu bytes", pl.n_lds_tables, pl.lds_table_dwords, budget);
		n_flat += pl.flat;
		n_emit += pl.flat_emit;
		n_mult += pl.mult;
		n_tables += pl.n_lds_tables;
		if (failures != before) {
			printf("  at pipeline %u (k %u, %u paths)\n", it, k, p.in.n_paths);
		}
	}
	checks = 0;
	printf("invariants: %u plans, %u flat, %u emitting, %u with multiplicities, %u LDS tables, %u shared\n", plans, n_flat,
	       n_emit, n_mult, n_tables, n_shared);
}

int main() {
	slots();
	mult_and_unique();
	flat();
	lds_tables();
	refusals();
	invariants();
	if (failures) {
		printf("%d check(s) failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
