// A stand-alone check of the window plan of a device merger with spilled runs (bwa-mem-gpu_amd/csrc/spill_plan.h): built by
// tests/test_bam_spill_cpu.py with -fsanitize=address,undefined and run as a child process.  The cut tables are made here, in plain C++,
// from a sorted order given as a list of (run, position): per window and run the first position, SPILL_NO_CUT where the window holds none,
// the owner of the window's first record in the last cell -- what k_spill_cuts (k_bamspill.hip) computes.  Prints "ok" and returns 0, or says
// what went wrong.
#include "spill_plan.h"
#include <stdio.h>
#include <algorithm>
#include <utility>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #x, what); return 1; } } while (0)

static unsigned seed = 1;
static int rnd(int n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (unsigned)n); }
static char what[200];

struct Case {
	std::vector<std::vector<int64_t>> off;                         // per run: n_rec + 1 offsets
	std::vector<std::pair<int, int>> order;                        // (run, position) in sorted order
	int64_t piece_bytes = 1000;
	size_t tie_from = 0;                                           // where the tie block begins in the order
	size_t n_runs() const { return off.size(); }
	int64_t len(const std::pair<int, int> &o) const { return off[(size_t)o.first][(size_t)o.second + 1] - off[(size_t)o.first][(size_t)o.second]; }
};

// runs of the given record lengths; the order: a random interleaving of the first half of every run, then run `whole` (if any) in one go,
// then a tie block: what is left of every run, run after run
static Case make_case(const std::vector<std::vector<int64_t>> &lens, int whole)
{
	Case c;
	for (auto &l : lens) { std::vector<int64_t> o(1, 0); for (int64_t x : l) o.push_back(o.back() + x); c.off.push_back(o); }
	std::vector<int> at(lens.size(), 0);
	for (;;) {
		std::vector<int> open;
		for (size_t r = 0; r < lens.size(); ++r) if ((int)r != whole && at[r] < (int)lens[r].size() / 2) open.push_back((int)r);
		if (open.empty()) break;
		const int r = open[(size_t)rnd((int)open.size())];
		c.order.push_back({ r, at[(size_t)r]++ });
	}
	c.tie_from = c.order.size();
	for (size_t r = 0; r < lens.size(); ++r) if ((int)r != whole) while (at[r] < (int)lens[r].size()) c.order.push_back({ (int)r, at[r]++ });
	if (whole >= 0) {                                              // in the middle of the order: positions within a run stay ascending
		std::vector<std::pair<int, int>> w;
		for (int p = 0; p < (int)lens[(size_t)whole].size(); ++p) w.push_back({ whole, p });
		c.order.insert(c.order.begin() + (long)(c.tie_from / 3), w.begin(), w.end());
		c.tie_from += w.size();
	}
	return c;
}

// k_piece_first and k_spill_cuts, restated
static void make_tables(const Case &c, const std::vector<bool> &spilled, int wp, std::vector<int> *piece_first, std::vector<int> *cut, int *n_windows)
{
	const int n = (int)c.order.size();
	std::vector<int64_t> out_off(1, 0);
	for (auto &o : c.order) out_off.push_back(out_off.back() + c.len(o));
	const int n_pieces = (int)((out_off.back() + c.piece_bytes - 1) / c.piece_bytes);
	piece_first->assign((size_t)n_pieces, 0);
	for (int p = 0; p < n_pieces; ++p) { int i = 0; while (i + 1 < n && out_off[(size_t)i + 1] <= p * c.piece_bytes) ++i; (*piece_first)[(size_t)p] = i; }
	const int nw = *n_windows = (n_pieces + wp - 1) / wp;
	const size_t NR = c.n_runs();
	cut->assign((size_t)nw * (NR + 1), SPILL_NO_CUT);
	auto first = [&](int w) { return (*piece_first)[(size_t)w * (size_t)wp]; };
	for (int i = 0; i < n; ++i) {
		int w = 0;
		while (w + 1 < nw && first(w + 1) <= i) ++w;                 // the last window whose first ordinal is <= i
		const int r = c.order[(size_t)i].first, pos = c.order[(size_t)i].second;
		int &cell = (*cut)[(size_t)w * (NR + 1) + (size_t)r];
		if (spilled[(size_t)r] && pos < cell) cell = pos;
		for (int v = w; v >= 0 && first(v) == i; --v) (*cut)[(size_t)v * (NR + 1) + NR] = r;
	}
}

static std::vector<SpillRun> runs_of(const Case &c, const std::vector<bool> &spilled)
{
	std::vector<SpillRun> runs;
	for (size_t r = 0; r < c.n_runs(); ++r) runs.push_back({ spilled[r], (int64_t)c.off[r].size() - 1, c.off[r].size() > 1 ? c.off[r].data() : nullptr });
	return runs;
}

// the plan of one case, subset and window size, against what the finish needs of it
static int check_plan(const Case &c, const std::vector<bool> &spilled, int wp)
{
	std::vector<int> piece_first, cut;
	int nw = 0;
	make_tables(c, spilled, wp, &piece_first, &cut, &nw);
	const int n = (int)c.order.size();
	const size_t NR = c.n_runs();
	SpillPlan p;
	CHECK(spill_plan_begin(&p, runs_of(c, spilled), (int)piece_first.size(), wp, piece_first.data(), n) == 0);
	CHECK(p.n_windows == nw && (int)p.first.size() == nw + 1 && p.first[(size_t)nw] == n && p.first[0] == 0);
	CHECK(spill_plan_cuts(&p, cut.data()) == 0);
	int64_t cap = 0;
	for (int w = 0; w < nw; ++w) {
		std::vector<std::pair<int64_t, int64_t>> placed;
		int64_t sum = 0;
		for (size_t r = 0; r < NR; ++r) {
			int64_t lo, counted, hi;
			p.slice(w, r, &lo, &counted, &hi);
			const int64_t n_rec = (int64_t)c.off[r].size() - 1;
			if (!spilled[r]) { CHECK(p.slice_bytes(w, r) == 0); continue; }
			CHECK(0 <= lo && lo <= counted && counted <= hi && hi <= n_rec && hi - counted <= 1);
			// the counted spans of a run tile its positions: every record is counted by exactly one window
			CHECK((w > 0 || lo == 0) && (w + 1 < nw || counted == n_rec));
			if (w + 1 < nw) { int64_t lo2, c2, h2; p.slice(w + 1, r, &lo2, &c2, &h2); CHECK(lo2 == counted); }
			const int64_t bytes = hi > lo ? c.off[r][(size_t)hi] - c.off[r][(size_t)lo] : 0;
			CHECK(p.slice_bytes(w, r) == bytes);
			if (bytes) placed.push_back({ p.slice_at[(size_t)w * NR + r], bytes });
			sum += bytes;
		}
		std::sort(placed.begin(), placed.end());
		for (size_t k = 0; k < placed.size(); ++k) CHECK(placed[k].first >= 0 && (k == 0 || placed[k - 1].first + placed[k - 1].second <= placed[k].first));   // no overlap
		CHECK(placed.empty() || placed.back().first + placed.back().second <= p.cap);
		if (sum > cap) cap = sum;
		// every record the window's pieces gather -- from its first record to the first record of the next window, inclusive -- is staged by it,
		// and counted by it unless a later window begins with the record
		const int last = w + 1 < nw ? p.first[(size_t)w + 1] : n - 1;
		for (int i = p.first[(size_t)w]; i <= last; ++i) {
			const size_t r = (size_t)c.order[(size_t)i].first;
			const int64_t pos = c.order[(size_t)i].second;
			if (!spilled[r]) continue;
			int64_t lo, counted, hi;
			p.slice(w, r, &lo, &counted, &hi);
			CHECK(lo <= pos && pos < hi);
			CHECK((pos < counted) == !(w + 1 < nw && i == p.first[(size_t)w + 1]));
		}
		// the straddling record: the first record of window w + 1 is staged by window w too
		if (w + 1 < nw) {
			const auto &o = c.order[(size_t)p.first[(size_t)w + 1]];
			CHECK(p.owner[(size_t)w + 1] == o.first);
			if (spilled[(size_t)o.first]) { int64_t lo, counted, hi; p.slice(w, (size_t)o.first, &lo, &counted, &hi); CHECK(counted == o.second && hi == counted + 1); }
		}
	}
	CHECK(p.cap == cap);                                           // the largest window's need, no more
	return 0;
}

// the windows a record of `bytes` bytes at ordinal i touches
static int windows_touched(const Case &c, int i, int wp)
{
	int64_t at = 0;
	for (int k = 0; k < i; ++k) at += c.len(c.order[(size_t)k]);
	const int64_t win = c.piece_bytes * wp;
	return (int)((at + c.len(c.order[(size_t)i]) - 1) / win - at / win + 1);
}

static int check_refusals()
{
	snprintf(what, sizeof what, "refusals");
	seed = 99;
	std::vector<std::vector<int64_t>> lens(3);
	for (auto &l : lens) for (int k = 0; k < 40; ++k) l.push_back(60 + rnd(80));
	const Case c = make_case(lens, -1);
	const std::vector<bool> spilled = { true, false, true };
	std::vector<int> piece_first, good;
	int nw = 0;
	make_tables(c, spilled, 1, &piece_first, &good, &nw);
	CHECK(nw >= 4);
	const auto plan_of = [&](const std::vector<int> &cut) {
		SpillPlan p;
		const int rc = spill_plan_begin(&p, runs_of(c, spilled), (int)piece_first.size(), 1, piece_first.data(), (int)c.order.size());
		return rc ? rc : spill_plan_cuts(&p, cut.data());
	};
	CHECK(plan_of(good) == 0);
	for (int owner : { -1, 3, 1000 }) { std::vector<int> bad = good; bad[(size_t)2 * 4 + 3] = owner; CHECK(plan_of(bad) == BWAHIP_EINTERNAL); }   // an owner that is no run
	for (int cell : { 40, 41, -1, SPILL_NO_CUT - 1 }) for (size_t r : { 0, 1, 2 }) { std::vector<int> bad = good; bad[(size_t)1 * 4 + r] = cell; CHECK(plan_of(bad) == BWAHIP_EINTERNAL); }   // a cell at or beyond n_rec, a resident run's too
	{ std::vector<int> bad = good; for (int w = 0; w < nw; ++w) if (bad[(size_t)w * 4 + 2] == 0) bad[(size_t)w * 4 + 2] = 1; CHECK(plan_of(bad) == BWAHIP_EINTERNAL); }   // a spilled run that does not begin in window 0
	// as many records as the preset of a cell: refused for a spilled run, before any table is looked at
	SpillPlan p;
	const int one = 0;
	CHECK(spill_plan_begin(&p, { { true, SPILL_NO_CUT, nullptr } }, 1, 1, &one, 5) == BWAHIP_ECAPACITY);
	CHECK(spill_plan_begin(&p, { { true, SPILL_NO_CUT - 1, nullptr }, { false, SPILL_NO_CUT, nullptr } }, 1, 1, &one, 5) == 0);
	return 0;
}

int main()
{
	int longest_tie = 0, longest_rec = 0, inside_one = 0, n_plans = 0;
	for (int n_runs : { 1, 3, 7 }) {
		seed = 7u * (unsigned)n_runs;
		// records of 40 to 160 bytes in pieces of 1 000; run 1 (of 3 and 7) has no record, run 2 three short ones that come together, and one
		// record of run 0's second half is longer than three windows of two pieces
		std::vector<std::vector<int64_t>> lens((size_t)n_runs);
		for (int r = 0; r < n_runs; ++r) for (int k = 0, nr = r == 1 ? 0 : r == 2 ? 3 : 60 + rnd(40); k < nr; ++k) lens[(size_t)r].push_back(r == 2 ? 40 : 40 + rnd(121));
		lens[0][lens[0].size() - 7] = 7300;
		const Case c = make_case(lens, n_runs > 2 ? 2 : -1);
		int64_t total = 0;
		for (auto &o : c.order) total += c.len(o);
		const int n_pieces = (int)((total + c.piece_bytes - 1) / c.piece_bytes);
		for (int wp : { 1, 2, n_pieces + 3 }) {
			for (int i = 0; i < (int)c.order.size(); ++i) if (c.len(c.order[(size_t)i]) == 7300) longest_rec = std::max(longest_rec, wp <= 2 ? windows_touched(c, i, wp) : 0);
			if (wp <= 2) {                                             // the whole windows the tie block covers
				int64_t tie = 0;
				for (size_t i = c.tie_from; i < c.order.size(); ++i) tie += c.len(c.order[i]);
				longest_tie = std::max(longest_tie, (int)(tie / (c.piece_bytes * wp)) - 1);
			}
			if (n_runs > 2 && wp == 2) {                               // run 2's 120 bytes: inside one window of 2 000, unless a cut falls into them (then the plan is checked all the same)
				int64_t at = 0;
				for (auto &o : c.order) { if (o.first == 2) break; at += c.len(o); }
				if (at / 2000 == (at + 119) / 2000) ++inside_one;
			}
			for (unsigned subset = 0; subset < 1u << n_runs; ++subset) {
				std::vector<bool> spilled;
				for (int r = 0; r < n_runs; ++r) spilled.push_back(subset >> r & 1);
				snprintf(what, sizeof what, "%d runs, subset %#x, window_pieces %d of %d pieces", n_runs, subset, wp, n_pieces);
				if (check_plan(c, spilled, wp)) return 1;
				++n_plans;
			}
		}
	}
	snprintf(what, sizeof what, "the cases themselves");
	CHECK(longest_tie >= 3 && longest_rec >= 4 && inside_one >= 1 && n_plans == 3 * (2 + 8 + 128));
	if (check_refusals()) return 1;
	printf("ok\n");
	return 0;
}
