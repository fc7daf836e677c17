// The window plan of a device merger's finish with spilled runs (k_bammerge.hip, k_bamspill.hip): which positions of which spilled run every
// window of window_pieces pieces stages, where in the staging buffer, and how large that buffer must be.  Host arithmetic on the cut table
// k_spill_cuts leaves and the runs' host offsets; no device, no HIP: tests/spill_plan_check.cpp includes this header alone.
//
// Window w stages the positions [lo, hi) of run r and counts [lo, counted): the record-reading stages handle a record in the one window
// that counts it.  hi = counted + 1 where r owns the first record of window w + 1: that record begins in window w (or at the cut), its
// bytes are gathered by both, so both stage it.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../include/bwahip.h"

constexpr int SPILL_NO_CUT = 0x7f7f7f7f;                           // what a cell of the cut table is preset to: the window holds no record of the run

struct SpillRun { bool spilled; int64_t n_rec; const int64_t *h_off; };   // h_off: the n_rec + 1 offsets of a spilled run that has records (otherwise not read)

struct SpillPlan {
	int n = 0, n_windows = 0;
	std::vector<SpillRun> runs;                                    // in run order; h_off points into the merger's runs: the plan lives no longer than one finish
	std::vector<int> first;                                        // per window: the ordinal of its first record; n_windows + 1 entries, the last = n
	std::vector<int> owner;                                        // per window: the run of its first record
	std::vector<int64_t> S;                                        // [window][run], n_windows + 1 rows: the first position the window needs, the last row = n_rec
	std::vector<int64_t> slice_at;                                 // [window][run]: the slice's place in the window's staging buffer
	int64_t cap = 0;                                               // the largest window's bytes
	size_t n_runs() const { return runs.size(); }
	void slice(int w, size_t r, int64_t *lo, int64_t *counted, int64_t *hi) const
	{
		*lo = S[(size_t)w * n_runs() + r]; *counted = S[((size_t)w + 1) * n_runs() + r];
		*hi = *counted + (w + 1 < n_windows && (size_t)owner[(size_t)w + 1] == r ? 1 : 0);
	}
	int64_t slice_bytes(int w, size_t r) const
	{
		int64_t lo, counted, hi;
		slice(w, r, &lo, &counted, &hi);
		return runs[r].spilled && hi > lo ? runs[r].h_off[hi] - runs[r].h_off[lo] : 0;
	}
};

// The windows of n_pieces pieces whose first records are piece_first (k_piece_first), n records in all.  BWAHIP_ECAPACITY: a spilled run has
// as many records as the preset of a cell.  Before the cut table is made: n_windows sizes it.
inline int spill_plan_begin(SpillPlan *p, const std::vector<SpillRun> &runs, int n_pieces, int window_pieces, const int *piece_first, int n)
{
	for (const SpillRun &r : runs) if (r.spilled && r.n_rec >= SPILL_NO_CUT) return BWAHIP_ECAPACITY;
	const int wp = window_pieces > 0 ? window_pieces : 1;
	p->runs = runs; p->n = n; p->n_windows = (n_pieces + wp - 1) / wp;
	p->first.assign((size_t)p->n_windows + 1, n);
	for (int w = 0; w < p->n_windows; ++w) p->first[(size_t)w] = piece_first[(size_t)w * wp];
	return 0;
}

// cut: n_windows rows of n_runs + 1 cells as k_spill_cuts leaves them -- per run the lowest position among the window's records (SPILL_NO_CUT:
// none; cells of resident runs are not looked at beyond their range), in the last cell the window's owner.  BWAHIP_EINTERNAL: an owner that is
// no run, a cell outside its run, a spilled run whose first window does not begin at position 0.
inline int spill_plan_cuts(SpillPlan *p, const int *cut)
{
	const size_t NR = p->n_runs();
	const int nw = p->n_windows;
	p->S.assign(((size_t)nw + 1) * NR, 0); p->owner.assign((size_t)nw, 0);
	for (size_t r = 0; r < NR; ++r) p->S[(size_t)nw * NR + r] = p->runs[r].n_rec;
	for (int w = nw - 1; w >= 0; --w) {
		const int *row = cut + (size_t)w * (NR + 1);
		if (row[NR] < 0 || (size_t)row[NR] >= NR) return BWAHIP_EINTERNAL;
		p->owner[(size_t)w] = row[NR];
		for (size_t r = 0; r < NR; ++r) {                             // a window without a record of the run takes the next window's start
			const int64_t next = p->S[((size_t)w + 1) * NR + r];
			if (row[r] < 0 || (row[r] != SPILL_NO_CUT && row[r] >= p->runs[r].n_rec)) return BWAHIP_EINTERNAL;
			p->S[(size_t)w * NR + r] = p->runs[r].spilled && row[r] < next ? row[r] : next;
		}
	}
	for (size_t r = 0; r < NR; ++r) if (p->runs[r].spilled && p->S[r] != 0) return BWAHIP_EINTERNAL;   // every ordinal lies in or behind window 0
	// every window's exact staging need, from the runs' offsets
	p->slice_at.assign((size_t)nw * NR, 0);
	p->cap = 0;
	for (int w = 0; w < nw; ++w) {
		int64_t at = 0;
		for (size_t r = 0; r < NR; ++r) {
			if (!p->runs[r].spilled) continue;
			p->slice_at[(size_t)w * NR + r] = at;
			at += p->slice_bytes(w, r);
		}
		if (at > p->cap) p->cap = at;
	}
	return 0;
}
