/* The early stop of ksw_extend2 ("ksw_extend2: rows that cannot matter") as plain C: the row loop of ksw.c:380-479 as
 * oracle/ora_ksw.c restates it, plus the rule, so that the rule itself is pinned where no GPU is needed
 * (tests/test_ext_early_stop_model.py compiles this file and compares it with liboracle.so's ora_ksw_extend2).
 *
 * ees_extend2: one call.  every = 0: the rule is off; k: it is tested after every k-th row.  *flags: bit 0 = the rule ended the loop,
 * bit 1 = it did so in a row the kernels' scalar pre-filter would have kept the test out of (must never happen: the pre-filter is a
 * necessary condition).  *rows = rows run, *evals = rows in which the pre-filter let the test through.
 * ees_compare: n seeded cases of one family against a caller-supplied ksw_extend2, counts into stats[]. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int32_t h, e; } cell_t;

int ees_extend2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                int o_del, int e_del, int o_ins, int e_ins, int w, int end_bonus, int zdrop, int h0, int every,
                int *qle_, int *tle_, int *gtle_, int *gscore_, int *max_off_, int *flags_, int *rows_, int *evals_)
{
	cell_t *row;
	int8_t *prof;
	int i, j, k, oe_del = o_del + e_del, oe_ins = o_ins + e_ins, mx, flags = 0, evals = 0;
	int beg, end, best, best_i, best_j, max_ins, max_del, best_ie, gscore, max_off;
	prof = (int8_t*)malloc((size_t)qlen * m + 1);
	row = (cell_t*)calloc(qlen + 2, sizeof(cell_t));
	for (k = i = 0; k < m; ++k) {
		const int8_t *p = &mat[k * m];
		for (j = 0; j < qlen; ++j) prof[i++] = p[query[j]];
	}
	row[0].h = h0; row[1].h = h0 > oe_ins ? h0 - oe_ins : 0;
	for (j = 2; j <= qlen && row[j-1].h > e_ins; ++j) row[j].h = row[j-1].h - e_ins;
	for (i = 0, mx = 0; i < m * m; ++i) mx = mx > mat[i] ? mx : mat[i];
	max_ins = (int)((double)(qlen * mx + end_bonus - o_ins) / e_ins + 1.);
	max_ins = max_ins > 1 ? max_ins : 1;
	w = w < max_ins ? w : max_ins;
	max_del = (int)((double)(qlen * mx + end_bonus - o_del) / e_del + 1.);
	max_del = max_del > 1 ? max_del : 1;
	w = w < max_del ? w : max_del;
	best = h0; best_i = best_j = -1; best_ie = -1; gscore = -1; max_off = 0;
	beg = 0; end = qlen;
	for (i = 0; i < tlen; ++i) {
		int t, f = 0, h1, rowmax = 0, rowmax_j = -1;
		const int8_t *s = &prof[target[i] * qlen];
		if (beg < i - w) beg = i - w;
		if (end > i + w + 1) end = i + w + 1;
		if (end > qlen) end = qlen;
		if (beg == 0) { h1 = h0 - (o_del + e_del * (i + 1)); if (h1 < 0) h1 = 0; }
		else h1 = 0;
		for (j = beg; j < end; ++j) {
			cell_t *p = &row[j];
			int h, M = p->h, e = p->e;
			p->h = h1;
			M = M ? M + s[j] : 0;
			h = M > e ? M : e;
			h = h > f ? h : f;
			h1 = h;
			rowmax_j = rowmax > h ? rowmax_j : j;
			rowmax = rowmax > h ? rowmax : h;
			t = M - oe_del; t = t > 0 ? t : 0;
			e -= e_del; e = e > t ? e : t;
			p->e = e;
			t = M - oe_ins; t = t > 0 ? t : 0;
			f -= e_ins; f = f > t ? f : t;
		}
		row[end].h = h1; row[end].e = 0;
		if (j == qlen) {
			best_ie = gscore > h1 ? best_ie : i;
			gscore = gscore > h1 ? gscore : h1;
		}
		if (rowmax == 0) { ++i; break; }
		if (rowmax > best) {
			best = rowmax; best_i = i; best_j = rowmax_j;
			max_off = max_off > abs(rowmax_j - i) ? max_off : abs(rowmax_j - i);
		} else if (zdrop > 0) {
			if (i - best_i > rowmax_j - best_j) {
				if (best - rowmax - ((i - best_i) - (rowmax_j - best_j)) * e_del > zdrop) { ++i; break; }
			} else {
				if (best - rowmax - ((rowmax_j - best_j) - (i - best_i)) * e_ins > zdrop) { ++i; break; }
			}
		}
		for (j = beg; j < end && row[j].h == 0 && row[j].e == 0; ++j);
		beg = j;
		for (j = end; j >= beg && row[j].h == 0 && row[j].e == 0; --j);
		end = j + 2 < qlen ? j + 2 : qlen;
		/* ---- the rule: no H of a later row exceeds phi */
		if (every > 0 && (i + 1) % every == 0 && end == qlen && gscore >= 0) {
			int phi = 0;
			if (rowmax_j + 1 >= qlen || rowmax + mx * (qlen - 1 - rowmax_j) < gscore) ++evals;   /* rows in which the kernels go on to the vector part */
			for (j = beg; j < qlen; ++j) {
				const int ph = row[j].h ? row[j].h + mx * (qlen - j) : 0, pe = row[j].e ? row[j].e + mx * (qlen - 1 - j) : 0;
				phi = phi > ph ? phi : ph;
				phi = phi > pe ? phi : pe;
			}
			if (phi < gscore && phi <= best) {
				flags |= 1;
				if (!(rowmax_j + 1 >= qlen || rowmax + mx * (qlen - 1 - rowmax_j) < gscore)) flags |= 2;
				++i; break;
			}
		}
	}
	free(row); free(prof);
	*qle_ = best_j + 1; *tle_ = best_i + 1; *gtle_ = best_ie + 1; *gscore_ = gscore; *max_off_ = max_off;
	if (flags_) *flags_ = flags;
	if (rows_) *rows_ = i;
	if (evals_) *evals_ = evals;
	return best;
}

/* ---------------------------------------------------------------- seeded cases, drawn as tests/dp_kat.py's rand_case draws them */
typedef int (*extend2_fn)(int, const uint8_t*, int, const uint8_t*, int, const int8_t*, int, int, int, int, int, int, int, int,
                          int*, int*, int*, int*, int*);

static _Thread_local uint64_t rs;                           /* (callers may run several ees_compare at once, one per thread) */
static uint64_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs * 0x2545F4914F6CDD1DULL >> 11; }   /* xorshift64* */
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }                                  /* lo .. hi */
static double runi(void) { return (double)rnd() / 9007199254740992.0; }

static const int MATS[5][2] = { {1, 4}, {2, 3}, {1, 1}, {3, 9}, {50, 60} };
static const int GAPS[5][4] = { {6, 1, 6, 1}, {4, 2, 7, 1}, {1, 1, 1, 1}, {16, 1, 16, 1}, {0, 1, 0, 1} };
static const int BANDS[12] = { 0, 1, 2, 5, 20, 31, 32, 63, 64, 100, 127, 400 };
static const int ZDROPS[5] = { 0, 1, 10, 100, 1000 };
static const int BONUSES[3] = { 0, 5, 50 };
static const int EDGE_LEN[12] = { 1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 700 };

static void scmat(int a, int b, int8_t *m)
{
	for (int i = 0; i < 25; ++i) m[i] = -1;
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[i * 5 + j] = (int8_t)(i == j ? a : -b);
}
/* the query with substitutions, short indels and now and then a long gap, cut or filled to tlen (dp_kat.mutate) */
static int mutate(const uint8_t *q, int qlen, int tlen, double err, uint8_t *t, int cap)
{
	int n = qlen;
	for (int i = 0; i < qlen; ++i) t[i] = q[i] > 3 ? 0 : q[i];
	for (int i = 0; i < qlen; ++i) {
		if (runi() >= err || n == 0) continue;
		const int p = rint_(0, n - 1);
		const double k = runi();
		if (k < 0.6) t[p] = (uint8_t)((t[p] + 1 + rint_(0, 2)) & 3);
		else {
			int g = runi() < 0.25 ? rint_(1, 40) : rint_(1, 3);
			if (k < 0.8) { if (g > n - p) g = n - p; memmove(t + p, t + p + g, (size_t)(n - p - g)); n -= g; }
			else if (n + g <= cap) { memmove(t + p + g, t + p, (size_t)(n - p)); for (int x = 0; x < g; ++x) t[p + x] = (uint8_t)rint_(0, 3); n += g; }
		}
	}
	for (; n < tlen; ++n) t[n] = (uint8_t)rint_(0, 3);
	return tlen;
}

enum { FAM_RANDOM = 0, FAM_TANDEM = 1, FAM_BENCH = 2 };
enum { ST_CASES, ST_DIFF, ST_STOPPED, ST_PREFILTER_MISS, ST_ROWS_FULL, ST_ROWS_RULE, ST_FIRST_DIFF, ST_GSCORE_NEG_STOPPED, ST_EVALS, ST_N };

/* stats: ST_* counts (ST_FIRST_DIFF: index of the first differing case, or -1; ST_ROWS_FULL, the rows of the loop without the rule, only
 * with want_rows, which costs a third DP per case).  Returns the number of differing cases. */
long ees_compare(extend2_fn ora, uint64_t seed, long n, int family, int every, int want_rows, long *stats)
{
	static _Thread_local uint8_t q[1024], t[4096];
	int8_t mat[25];
	rs = seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL;
	for (int i = 0; i < 16; ++i) rnd();
	memset(stats, 0, sizeof(long) * ST_N);
	stats[ST_FIRST_DIFF] = -1;
	for (long c = 0; c < n; ++c) {
		int qlen, tlen, w, h0, zdrop, bonus, mi = rint_(0, 4), gi = rint_(0, 4);
		double err = runi() < 0.75 ? runi() * 0.08 : runi() * 0.30;
		const double n_frac = runi() < 0.2 ? runi() * 0.05 : 0.0;
		{ const int k = rint_(0, 2); qlen = k == 0 ? EDGE_LEN[rint_(0, 11)] : k == 1 ? rint_(1, 700) : rint_(1, 250); }
		tlen = qlen + rint_(-40, 80); if (tlen < 1) tlen = 1;
		w = BANDS[rint_(0, 11)];
		h0 = runi() < 0.5 ? rint_(1, 5000) : rint_(1, 120);
		zdrop = ZDROPS[rint_(0, 4)]; bonus = BONUSES[rint_(0, 2)];
		if (family == FAM_BENCH) {      /* the benchmark's flanks: 1/-4, 6/1, w 100, z-drop 100, bonus 5, tlen = qlen + max_gap, 1 % substitutions, first base a mismatch */
			qlen = rint_(3, 102); mi = 0; gi = 0; w = 100; zdrop = 100; bonus = 5; h0 = rint_(19, 147);
			int mg = qlen * 1 - 6 + 1; mg = mg > 1 ? mg : 1; mg = mg < 200 ? mg : 200;
			tlen = qlen + mg;
		}
		if (family == FAM_TANDEM) {     /* a repeat of period 1..6 against a longer repeat of the same unit */
			const int per = rint_(1, 6);
			uint8_t unit[6];
			for (int i = 0; i < per; ++i) unit[i] = (uint8_t)rint_(0, 3);
			if (qlen > 650) qlen = 650;
			tlen = qlen + rint_(0, 120);
			for (int i = 0; i < qlen; ++i) q[i] = unit[i % per];
			for (int i = 0; i < tlen; ++i) t[i] = unit[i % per];
			err = runi() < 0.5 ? 0.0 : runi() * 0.03;
			for (int i = 0; i < tlen; ++i) if (runi() < err) t[i] = (uint8_t)rint_(0, 3);
			for (int i = 0; i < qlen; ++i) if (runi() < err) q[i] = (uint8_t)rint_(0, 3);
		} else {
			for (int i = 0; i < qlen; ++i) q[i] = (uint8_t)(runi() < n_frac ? 4 : rint_(0, 3));
			if (family == FAM_BENCH) {
				for (int i = 0; i < tlen; ++i) t[i] = (uint8_t)(i < qlen ? (runi() < 0.01 ? (q[i] + 1 + rint_(0, 2)) & 3 : q[i] & 3) : rint_(0, 3));
				t[0] = (uint8_t)((q[0] + 1) & 3);
			} else {
				mutate(q, qlen, tlen, err, t, (int)sizeof(t) - 64);
				for (int i = 0; i < tlen; ++i) if (runi() < n_frac) t[i] = 4;
			}
		}
		scmat(MATS[mi][0], MATS[mi][1], mat);
		int a[6], b[6], flags, rows, rows_full, evals;
		a[0] = ora(qlen, q, tlen, t, 5, mat, GAPS[gi][0], GAPS[gi][1], GAPS[gi][2], GAPS[gi][3], w, bonus, zdrop, h0, &a[1], &a[2], &a[3], &a[4], &a[5]);
		b[0] = ees_extend2(qlen, q, tlen, t, 5, mat, GAPS[gi][0], GAPS[gi][1], GAPS[gi][2], GAPS[gi][3], w, bonus, zdrop, h0, every, &b[1], &b[2], &b[3], &b[4], &b[5], &flags, &rows, &evals);
		int c0[6];
		if (!want_rows) { memcpy(c0, a, sizeof a); rows_full = 0; }
		else c0[0] = ees_extend2(qlen, q, tlen, t, 5, mat, GAPS[gi][0], GAPS[gi][1], GAPS[gi][2], GAPS[gi][3], w, bonus, zdrop, h0, 0, &c0[1], &c0[2], &c0[3], &c0[4], &c0[5], 0, &rows_full, 0);
		++stats[ST_CASES];
		if (memcmp(a, b, sizeof a) || memcmp(a, c0, sizeof a)) { if (stats[ST_FIRST_DIFF] < 0) stats[ST_FIRST_DIFF] = c; ++stats[ST_DIFF]; }
		if (flags & 1) ++stats[ST_STOPPED];
		if (flags & 2) ++stats[ST_PREFILTER_MISS];
		if ((flags & 1) && a[4] < 0) ++stats[ST_GSCORE_NEG_STOPPED];
		stats[ST_ROWS_FULL] += rows_full; stats[ST_ROWS_RULE] += rows; stats[ST_EVALS] += evals;
	}
	return stats[ST_DIFF];
}
