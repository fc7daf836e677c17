/* The diagonal rule of ksw_extend2 ("ksw_extend2: flanks the diagonal answers") as plain C: a predicate and the six results it
 * writes down, so that the rule is pinned where no GPU is needed (tests/test_ext_diag_model.py compiles this file and compares it with
 * liboracle.so's ora_ksw_extend2; tests/test_gpu_ext_diag.py holds the device's DIAG bit against the predicate).
 *
 * edg_rule: one call.  Returns 1 and fills out6 (score, qle, tle, gtle, gscore, max_off) when the rule applies, else 0.
 * edg_compare: n seeded cases of one family; the oracle is called where the predicate holds, counts go into stats[]. */
#include <stdint.h>
#include <string.h>

/* K: the largest integer with K * (a + b) < g, g = min(o_del + e_del, o_ins + e_ins); 0 when the matrix is not bwa_fill_scmat(a, b) with
 * a >= 1 and b >= 0 in its ACGT block (the N row and column are never read: a flank with an N is refused) */
int edg_k(int m, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins)
{
	if (m != 5) return 0;
	const int a = mat[0], b = -mat[1];
	for (int i = 0; i < 4; ++i)
		for (int j = 0; j < 4; ++j)
			if (mat[i * 5 + j] != (i == j ? a : -b)) return 0;
	if (a < 1 || b < 0) return 0;
	const int g = o_del + e_del < o_ins + e_ins ? o_del + e_del : o_ins + e_ins;
	return g < 1 ? 0 : (g - 1) / (a + b);
}

int edg_rule(int qlen, const uint8_t *q, int tlen, const uint8_t *t, int m, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
             int w, int end_bonus, int zdrop, int h0, int *out6)
{
	const int K = edg_k(m, mat, o_del, e_del, o_ins, e_ins);
	(void)w; (void)end_bonus;                                   /* the diagonal is inside every band, and the bonus is the caller's business */
	if (K < 1 || qlen < 1 || tlen < qlen || h0 < 1) return 0;
	const int a = mat[0], b = -mat[1];
	if (zdrop > 0 && K * b > zdrop) return 0;
	int mism = 0, d = h0, best = h0, best_j = -1;
	for (int j = 0; j < qlen; ++j) if (q[j] > 3 || t[j] > 3) return 0;
	for (int j = 0; j < qlen; ++j) {
		if (q[j] == t[j]) d += a;
		else {
			if (++mism > K) return 0;
			d -= b;
			if (d < 1) return 0;
		}
		if (d > best) { best = d; best_j = j; }                 /* strictly: the first base at which the largest value is reached */
	}
	out6[0] = best; out6[1] = best_j + 1; out6[2] = best_j + 1; out6[3] = qlen; out6[4] = d; out6[5] = 0;
	return 1;
}

/* ---------------------------------------------------------------- seeded cases */
typedef int (*extend2_fn)(int, const uint8_t*, int, const uint8_t*, int, const int8_t*, int, int, int, int, int, int, int, int,
                          int*, int*, int*, int*, int*);

static _Thread_local uint64_t rs;                           /* (callers may run several edg_compare at once, one per thread) */
static uint64_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs * 0x2545F4914F6CDD1DULL >> 11; }   /* xorshift64* */
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }                                  /* lo .. hi */
static double runi(void) { return (double)rnd() / 9007199254740992.0; }

/* the grids of tests/dp_kat.py */
static const int MATS[5][2] = { {1, 4}, {2, 3}, {1, 1}, {3, 9}, {50, 60} };
static const int GAPS[5][4] = { {6, 1, 6, 1}, {4, 2, 7, 1}, {1, 1, 1, 1}, {16, 1, 16, 1}, {0, 1, 0, 1} };
static const int BANDS[12] = { 0, 1, 2, 5, 20, 31, 32, 63, 64, 100, 127, 400 };
static const int ZDROPS[5] = { 0, 1, 10, 100, 1000 };
static const int BONUSES[3] = { 0, 5, 50 };

static void scmat(int a, int b, int8_t *m)
{
	for (int i = 0; i < 25; ++i) m[i] = -1;
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[i * 5 + j] = (int8_t)(i == j ? a : -b);
}
static void substitute(uint8_t *s, int p) { s[p] = (uint8_t)((s[p] + 1 + rint_(0, 2)) & 3); }

enum { FAM_GRID = 0, FAM_TANDEM = 1, FAM_SHIFT = 2, FAM_BENCH = 3,
       /* edge families; those from FAM_REFUSE_FIRST on must be refused */
       FAM_SHORT = 4, FAM_ENDS = 5, FAM_EXACT = 6, FAM_TLEN_EQ = 7,
       FAM_REFUSE_FIRST = 8, FAM_TLEN_SHORT = 8, FAM_H0_LOW = 9, FAM_ZDROP_LOW = 10, FAM_GAPS_CHEAP = 11, FAM_N = 12, FAM_COUNT = 13 };
enum { ST_CASES, ST_HOLDS, ST_DIFF, ST_FIRST_DIFF, ST_N };

/* stats: ST_CASES, ST_HOLDS (the predicate held), ST_DIFF (it held and a result differs from the oracle's), ST_FIRST_DIFF (index of the
 * first such case, or -1).  Returns ST_DIFF. */
long edg_compare(extend2_fn ora, uint64_t seed, long n, int family, long *stats)
{
	static _Thread_local uint8_t q[1024], t[2048];
	int8_t mat[25];
	rs = seed * 0x9E3779B97F4A7C15ULL + 0x7654321ULL + (uint64_t)family * 0x100000001B3ULL;
	for (int i = 0; i < 16; ++i) rnd();
	memset(stats, 0, sizeof(long) * ST_N);
	stats[ST_FIRST_DIFF] = -1;
	for (long c = 0; c < n; ++c) {
		int mi = rint_(0, 4), gi = rint_(0, 4);
		int qlen = rint_(0, 3) == 0 ? rint_(1, 700) : rint_(1, 200);
		int w = BANDS[rint_(0, 11)], zdrop = ZDROPS[rint_(0, 4)], bonus = BONUSES[rint_(0, 2)];
		int h0 = runi() < 0.5 ? rint_(1, 5000) : rint_(1, 120);
		int a = MATS[mi][0], b = MATS[mi][1];
		int g4[4]; memcpy(g4, GAPS[gi], sizeof g4);
		if (family >= FAM_SHORT && family != FAM_GAPS_CHEAP) {  /* the edge families want the rule alive apart from their own edge */
			do { mi = rint_(0, 4); gi = rint_(0, 4); a = MATS[mi][0]; b = MATS[mi][1]; memcpy(g4, GAPS[gi], sizeof g4); scmat(a, b, mat); }
			while (edg_k(5, mat, g4[0], g4[1], g4[2], g4[3]) < 1);
			if (zdrop > 0 && zdrop < 1000) zdrop = 1000;
			h0 = rint_(2 * b + 1, 2 * b + 200);
		}
		scmat(a, b, mat);
		const int K = edg_k(5, mat, g4[0], g4[1], g4[2], g4[3]);
		int tlen = qlen + rint_(0, 80);
		int nsub = rint_(0, K + 1);
		if (family == FAM_BENCH) {      /* the benchmark's flanks: 3 to 102 bases, 1/-4, 6/1, w 100, z-drop 100, bonus 5, tlen = qlen + max_gap, the first base a mismatch (the seed ended there), 1 % substitutions after it */
			qlen = rint_(3, 102); a = 1; b = 4; scmat(a, b, mat); memcpy(g4, GAPS[0], sizeof g4); w = 100; zdrop = 100; bonus = 5; h0 = rint_(19, 147);
			int mg = qlen - 6 + 1; mg = mg > 1 ? mg : 1; mg = mg < 200 ? mg : 200;
			tlen = qlen + mg;
		}
		if (family == FAM_SHORT) { qlen = rint_(1, 8); tlen = qlen + rint_(0, 20); }
		if (family == FAM_TLEN_EQ) tlen = qlen;
		if (family == FAM_TLEN_SHORT) tlen = qlen - 1;
		/* ---- the sequences */
		if (family == FAM_TANDEM) {     /* a repeat of period 1..6 against a longer repeat of the same unit, 0 to K + 1 substitutions */
			const int per = rint_(1, 6);
			uint8_t unit[6];
			for (int i = 0; i < per; ++i) unit[i] = (uint8_t)rint_(0, 3);
			tlen = qlen + rint_(0, 120);
			for (int i = 0; i < qlen; ++i) q[i] = unit[i % per];
			for (int i = 0; i < tlen; ++i) t[i] = unit[i % per];
		} else {
			for (int i = 0; i < qlen; ++i) q[i] = (uint8_t)rint_(0, 3);
			for (int i = 0; i < tlen; ++i) t[i] = i < qlen ? q[i] : (uint8_t)rint_(0, 3);
		}
		if (family == FAM_SHIFT) {      /* the query inside the target again, shifted by 1 to 8 bases; low complexity in half of the cases */
			const int sh = rint_(1, 8);
			if (rint_(0, 1)) for (int i = 0; i < qlen; ++i) q[i] = (uint8_t)(rint_(0, 9) ? q[i > 0 ? i - 1 : 0] : rint_(0, 3));
			tlen = qlen + sh + rint_(0, 40);
			if (rint_(0, 3)) for (int i = 0; i < tlen; ++i) t[i] = i < qlen ? q[i] : q[(i + 8 * qlen - sh) % qlen];   /* the straight copy, going on as the shifted one */
			else for (int i = 0; i < tlen; ++i) t[i] = i >= sh && i - sh < qlen ? q[i - sh] : (uint8_t)rint_(0, 3);   /* the shifted copy alone */
		}
		if (family == FAM_BENCH) {
			for (int i = 1; i < qlen; ++i) if (runi() < 0.01) substitute(t, i);
			t[0] = (uint8_t)((q[0] + 1 + rint_(0, 2)) & 3);
		} else if (family == FAM_ENDS) {                        /* a mismatch at the first base, at the last one, or at both */
			const int k = rint_(0, 2);
			if (k != 1) substitute(t, 0);
			if (k != 0 && qlen > 1) substitute(t, qlen - 1);
		} else if (family == FAM_EXACT || family == FAM_TLEN_SHORT) {
			;                                                     /* no mismatch at all */
		} else if (family == FAM_H0_LOW) {                      /* the first base a mismatch that h0 cannot pay: the diagonal dies */
			h0 = rint_(1, b); substitute(t, 0);
		} else if (family == FAM_ZDROP_LOW) {
			if (b < 2) { b = 4; a = 1; scmat(a, b, mat); memcpy(g4, GAPS[0], sizeof g4); }
			zdrop = rint_(1, b - 1);
			if (rint_(0, 1)) substitute(t, rint_(0, qlen - 1));
		} else if (family == FAM_GAPS_CHEAP) {                  /* g <= a + b: not one mismatch is affordable */
			a = MATS[mi][0]; b = MATS[mi][1]; scmat(a, b, mat);
			const int e = rint_(1, 2), o = rint_(0, a + b - e > 0 ? a + b - e : 0);
			g4[0] = rint_(0, 1) ? o : o + rint_(0, 20); g4[1] = e; g4[2] = g4[0] == o ? o + rint_(0, 20) : o; g4[3] = e;
			if (rint_(0, 1)) substitute(t, rint_(0, qlen - 1));
		} else if (family == FAM_N) {                           /* an N in the query, or in the target bases the flank lies on */
			if (rint_(0, 3) == 0) substitute(t, rint_(0, qlen - 1));
			if (rint_(0, 1)) q[rint_(0, qlen - 1)] = 4; else t[rint_(0, qlen - 1)] = 4;
		} else {
			for (int k = 0; k < nsub; ++k) { const int p = rint_(0, qlen - 1); if (p < tlen) substitute(t, p); }
			if (family == FAM_GRID && rint_(0, 19) == 0) { const int p = rint_(0, tlen - 1); t[p] = 4; }      /* now and then an N anywhere in the target */
		}
		if (tlen < 0) tlen = 0;
		int r[6], o6[6];
		const int holds = edg_rule(qlen, q, tlen, t, 5, mat, g4[0], g4[1], g4[2], g4[3], w, bonus, zdrop, h0, r);
		++stats[ST_CASES];
		if (!holds) continue;
		++stats[ST_HOLDS];
		o6[0] = ora(qlen, q, tlen, t, 5, mat, g4[0], g4[1], g4[2], g4[3], w, bonus, zdrop, h0, &o6[1], &o6[2], &o6[3], &o6[4], &o6[5]);
		if (memcmp(r, o6, sizeof r)) { if (stats[ST_FIRST_DIFF] < 0) stats[ST_FIRST_DIFF] = c; ++stats[ST_DIFF]; }
	}
	return stats[ST_DIFF];
}
