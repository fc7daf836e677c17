/* The table jump of bwt_smem1a ("k_smem: the short-string triangle skipped by table jumps") as plain C on top of liboracle.so's
 * ora_set_intv and ora_extend, so that the rule is pinned where no GPU is needed (tests/test_smem_skip_model.py compiles this file and
 * holds it against ora_smem1a, call by call and bit for bit; tests/test_gpu_smem_skip.py holds the kernel against the oracle).
 *
 * The "table" is ssk_table: the bi-interval of a string by successive forward extensions, the function bwahip_kat_kmer_table pins the
 * device's interval table to.
 *
 * ssk_smem1a: one call of bwt_smem1a(x, min_intv) with max_intv = 0 and jump depth J (J < 2: plain).  A call that can jump starts its
 * forward phase at the table entry of read[x..x+J); the ends x+1 .. x+J-1 are dormant entries, not stored and presumed alive, and the
 * backward step at i materialises the one with end i + J -- its string read[i..i+J) is one look-up -- after the active entries.  A
 * jumped or materialised string that occurs fewer than min_intv times abandons the call, which is then run again in the plain way.
 * Turns are counted the way the kernel pays them: one per ora_extend, one per look-up, and those of an abandoned attempt stay paid. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "ora.h"

enum { SSK_CALLS, SSK_CAN_JUMP, SSK_JUMPED, SSK_FALLBACKS, SSK_LOOKUPS, SSK_PLAIN_TURNS, SSK_SKIP_TURNS, SSK_ABANDONED_TURNS, SSK_DIFF,
       SSK_FIRST_DIFF_READ, SSK_FIRST_DIFF_X, SSK_N };

static void push(ora_intv_v *v, const ora_intv_t *p)
{
	if (v->n == v->m) { v->m = v->m ? v->m << 1 : 16; v->a = (ora_intv_t*)realloc(v->a, v->m * sizeof(ora_intv_t)); }
	v->a[v->n++] = *p;
}
static void reverse(ora_intv_v *v)
{
	for (int i = 0; i < v->n >> 1; ++i) { ora_intv_t t = v->a[i]; v->a[i] = v->a[v->n - 1 - i]; v->a[v->n - 1 - i] = t; }
}

/* the bi-interval of s[0..n), all ACGT: what the interval table holds for that string (only the size of a string that does not occur is
 * ever looked at) */
void ssk_table(const ora_fmi_t *f, const uint8_t *s, int n, ora_intv_t *out)
{
	ora_intv_t ik, ok[4];
	ora_set_intv(f, s[0], &ik);
	for (int k = 1; k < n; ++k) { ora_extend(f, &ik, ok, 0); ik = ok[3 - s[k]]; }
	ik.info = 0;
	*out = ik;
}

/* one attempt: J >= 2 speculative, else plain.  Returns 0 when the attempt was abandoned (never when plain); *turns: extends + look-ups */
static int attempt(const ora_fmi_t *f, int len, const uint8_t *q, int x, int min_intv, int J, ora_intv_v *mem, ora_intv_v *tmp[2],
                   int *ret, long *turns, long *lookups)
{
	int i, j, c, dormant = 0;
	ora_intv_t ik, ok[4];
	ora_intv_v *prev = tmp[0], *curr = tmp[1], *sw;
	mem->n = 0; *turns = 0; *lookups = 0;
	if (J >= 2) {                                           /* forward jump */
		ssk_table(f, q + x, J, &ik); ++*turns; ++*lookups;
		if (ik.x[2] < (uint64_t)min_intv) return 0;
		ik.info = x + J; dormant = J - 1;
	} else { ora_set_intv(f, q[x], &ik); ik.info = x + 1; }
	for (i = (int)ik.info, curr->n = 0; i < len; ++i) {     /* bwt.c:304-320 */
		if (q[i] < 4) {
			c = 3 - q[i];
			ora_extend(f, &ik, ok, 0); ++*turns;
			if (ok[c].x[2] != ik.x[2]) {
				push(curr, &ik);
				if (ok[c].x[2] < (uint64_t)min_intv) break;
			}
			ik = ok[c]; ik.info = i + 1;
		} else { push(curr, &ik); break; }
	}
	if (i == len) push(curr, &ik);
	reverse(curr);
	*ret = (int)curr->a[0].info;
	sw = curr; curr = prev; prev = sw;
	for (i = x - 1; i >= -1; --i) {                         /* bwt.c:326-345 */
		c = i < 0 ? -1 : q[i] < 4 ? q[i] : -1;
		for (j = 0, curr->n = 0; j < prev->n; ++j) {
			ora_intv_t *p = &prev->a[j];
			if (c >= 0) { ora_extend(f, p, ok, 1); ++*turns; }
			if (c < 0 || ok[c].x[2] < (uint64_t)min_intv) {
				if (curr->n == 0 && (mem->n == 0 || (uint64_t)(i + 1) < mem->a[mem->n - 1].info >> 32)) {
					ik = *p; ik.info |= (uint64_t)(i + 1) << 32;
					push(mem, &ik);
				}
			} else if (curr->n == 0 || ok[c].x[2] != curr->a[curr->n - 1].x[2]) {
				ok[c].info = p->info;
				push(curr, &ok[c]);
			}
		}
		if (c >= 0 && dormant > 0) {                        /* the dormant entry with end i + J: shorter than every active one */
			ssk_table(f, q + i, J, &ik); ++*turns; ++*lookups;
			if (ik.x[2] < (uint64_t)min_intv) return 0;       /* it died at a step nobody saw, or here: the call is run again plainly */
			if (curr->n == 0 || ik.x[2] != curr->a[curr->n - 1].x[2]) { ik.info = i + J; push(curr, &ik); }
			--dormant;
		}
		if (curr->n == 0) break;                            /* (never while a dormant entry is left: the one just materialised is alive) */
		sw = curr; curr = prev; prev = sw;
	}
	reverse(mem);
	return 1;
}

/* 1 when the call at x can jump J bases: they lie inside the read and are all ACGT */
static int can_jump(int len, const uint8_t *q, int x, int J)
{
	if (J < 2 || x + J > len) return 0;
	for (int k = 0; k < J; ++k) if (q[x + k] > 3) return 0;
	return 1;
}

int ssk_smem1a(const ora_fmi_t *f, int len, const uint8_t *q, int x, int min_intv, int J, ora_intv_v *mem, ora_intv_v *tmp[2], long *stats)
{
	int ret = 0;
	long turns, lookups;
	mem->n = 0;
	if (q[x] > 3) return x + 1;
	if (min_intv < 1) min_intv = 1;
	if (can_jump(len, q, x, J)) {
		++stats[SSK_CAN_JUMP];
		const int ok = attempt(f, len, q, x, min_intv, J, mem, tmp, &ret, &turns, &lookups);
		stats[SSK_SKIP_TURNS] += turns; stats[SSK_LOOKUPS] += lookups;
		if (ok) { ++stats[SSK_JUMPED]; return ret; }
		++stats[SSK_FALLBACKS]; stats[SSK_ABANDONED_TURNS] += turns;
	}
	attempt(f, len, q, x, min_intv, 0, mem, tmp, &ret, &turns, &lookups);
	stats[SSK_SKIP_TURNS] += turns;
	return ret;
}

typedef struct { ora_intv_v mem, ref, tmpv[2]; } work_t;
static void work_free(work_t *w) { free(w->mem.a); free(w->ref.a); free(w->tmpv[0].a); free(w->tmpv[1].a); }

/* one call through both, compared; plain turns are counted by a plain attempt of the model (the same ora_extend calls ora_smem1a makes) */
static int both(const ora_fmi_t *f, int len, const uint8_t *q, int x, int min_intv, int J, work_t *w, long *stats, long rd)
{
	ora_intv_v *tmp[2] = { &w->tmpv[0], &w->tmpv[1] };
	int r0, ret;
	long turns, lookups;
	const int want = ora_smem1a(f, len, q, x, min_intv, 0, &w->ref, tmp);
	++stats[SSK_CALLS];
	if (q[x] < 4) {
		attempt(f, len, q, x, min_intv < 1 ? 1 : min_intv, 0, &w->mem, tmp, &r0, &turns, &lookups);
		stats[SSK_PLAIN_TURNS] += turns;
	}
	ret = ssk_smem1a(f, len, q, x, min_intv, J, &w->mem, tmp, stats);
	if (ret != want || w->mem.n != w->ref.n || (w->mem.n && memcmp(w->mem.a, w->ref.a, (size_t)w->mem.n * sizeof(ora_intv_t)))) {
		if (stats[SSK_DIFF]++ == 0) { stats[SSK_FIRST_DIFF_READ] = rd; stats[SSK_FIRST_DIFF_X] = x; }
	}
	return ret;
}

/* every ACGT x of every read as a call of its own.  Returns the number of calls that differ from ora_smem1a. */
long ssk_compare_every_x(const ora_fmi_t *f, long n_reads, const uint8_t *codes, const int64_t *off, int min_intv, int J, long *stats)
{
	work_t w; memset(&w, 0, sizeof w);
	memset(stats, 0, sizeof(long) * SSK_N);
	stats[SSK_FIRST_DIFF_READ] = stats[SSK_FIRST_DIFF_X] = -1;
	for (long r = 0; r < n_reads; ++r) {
		const uint8_t *q = codes + off[r];
		const int len = (int)(off[r + 1] - off[r]);
		for (int x = 0; x < len; ++x) if (q[x] < 4) both(f, len, q, x, min_intv, J, &w, stats, r);
	}
	work_free(&w);
	return stats[SSK_DIFF];
}

/* the calls passes 1 and 2 of mem_collect_intv make (bwamem.c:144-165); the depth is clamped to min_seed_len as the kernel clamps it.
 * stats1 / stats2: the two passes apart (may be the same array); fb_by_intv[2 * m], fb_by_intv[2 * m + 1]: calls that could jump and
 * fallbacks at min_intv = m (m < n_by_intv; larger ones in the last pair). */
long ssk_collect(const ora_fmi_t *f, long n_reads, const uint8_t *codes, const int64_t *off, int min_seed_len, double split_factor,
                 int split_width, int J, long *stats1, long *stats2, long *fb_by_intv, int n_by_intv)
{
	work_t w; memset(&w, 0, sizeof w);
	ora_intv_v all = { 0, 0, 0 };
	const int split_len = (int)(min_seed_len * split_factor + .499);
	memset(stats1, 0, sizeof(long) * SSK_N); memset(stats2, 0, sizeof(long) * SSK_N);
	stats1[SSK_FIRST_DIFF_READ] = stats1[SSK_FIRST_DIFF_X] = stats2[SSK_FIRST_DIFF_READ] = stats2[SSK_FIRST_DIFF_X] = -1;
	if (fb_by_intv) memset(fb_by_intv, 0, sizeof(long) * 2 * n_by_intv);
	if (J > min_seed_len) J = min_seed_len;
	for (long r = 0; r < n_reads; ++r) {
		const uint8_t *q = codes + off[r];
		const int len = (int)(off[r + 1] - off[r]);
		int x = 0;
		all.n = 0;
		if (len < min_seed_len) continue;                   /* bwamem.c:267 */
		while (x < len) {
			if (q[x] < 4) {
				const long cj = stats1[SSK_CAN_JUMP], fb = stats1[SSK_FALLBACKS];
				x = both(f, len, q, x, 1, J, &w, stats1, r);
				if (fb_by_intv && n_by_intv > 1) { fb_by_intv[2] += stats1[SSK_CAN_JUMP] - cj; fb_by_intv[3] += stats1[SSK_FALLBACKS] - fb; }
				for (int k = 0; k < w.mem.n; ++k)
					if ((int)((uint32_t)w.mem.a[k].info - (w.mem.a[k].info >> 32)) >= min_seed_len) push(&all, &w.mem.a[k]);
			} else ++x;
		}
		const int old_n = all.n;
		for (int k = 0; k < old_n; ++k) {
			const ora_intv_t p = all.a[k];
			const int start = (int)(p.info >> 32), end = (int)(uint32_t)p.info;
			if (end - start < split_len || p.x[2] > (uint64_t)split_width) continue;
			const long cj = stats2[SSK_CAN_JUMP], fb = stats2[SSK_FALLBACKS];
			both(f, len, q, (start + end) >> 1, (int)p.x[2] + 1, J, &w, stats2, r);
			if (fb_by_intv) {
				int m = (int)p.x[2] + 1; if (m >= n_by_intv) m = n_by_intv - 1;
				fb_by_intv[2 * m] += stats2[SSK_CAN_JUMP] - cj; fb_by_intv[2 * m + 1] += stats2[SSK_FALLBACKS] - fb;
			}
		}
	}
	work_free(&w); free(all.a);
	return stats1[SSK_DIFF] + stats2[SSK_DIFF];
}
