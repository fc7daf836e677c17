/* ORACLE (test infrastructure only) -- paired-end logic.
 * Restates bwamem_pair.c: insert-size statistics (:72-135), mate rescue
 * (:137-206), pairing (:208-271), paired SAM output and mapQ (:276-419).
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <assert.h>
#include "ora.h"

static inline int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)   /* bwamem_pair.c:48 */
{
	int64_t p2;
	int r1 = (b1 >= l_pac), r2 = (b2 >= l_pac);
	p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

static int best_sub(const ora_opt_t *opt, const ora_reg_v *r)   /* bwamem_pair.c:57 cal_sub */
{
	int j;
	for (j = 1; j < r->n; ++j) {
		int b_max = r->a[j].qb > r->a[0].qb ? r->a[j].qb : r->a[0].qb;
		int e_min = r->a[j].qe < r->a[0].qe ? r->a[j].qe : r->a[0].qe;
		if (e_min > b_max) {
			int min_l = r->a[j].qe - r->a[j].qb < r->a[0].qe - r->a[0].qb ? r->a[j].qe - r->a[j].qb : r->a[0].qe - r->a[0].qb;
			if (e_min - b_max >= min_l * opt->mask_level) break;
		}
	}
	return j < r->n ? r->a[j].score : opt->min_seed_len * opt->a;
}

void ora_pestat(const ora_opt_t *opt, int64_t l_pac, int n, const ora_reg_v *regs, ora_pestat_t pes[4])   /* bwamem_pair.c:72 */
{
	int i, d, max;
	struct { size_t n, m; uint64_t *a; } isize[4];
	memset(pes, 0, 4 * sizeof(ora_pestat_t));
	memset(isize, 0, sizeof isize);
	for (i = 0; i < n >> 1; ++i) {
		int dir;
		int64_t is;
		const ora_reg_v *r0 = &regs[i << 1 | 0], *r1 = &regs[i << 1 | 1];
		if (r0->n == 0 || r1->n == 0) continue;
		if (best_sub(opt, r0) > 0.8 * r0->a[0].score) continue;      /* MIN_RATIO */
		if (best_sub(opt, r1) > 0.8 * r1->a[0].score) continue;
		if (r0->a[0].rid != r1->a[0].rid) continue;
		dir = infer_dir(l_pac, r0->a[0].rb, r1->a[0].rb, &is);
		if (is && is <= opt->max_ins) {
			if (isize[dir].n == isize[dir].m) {
				isize[dir].m = isize[dir].m ? isize[dir].m << 1 : 2;
				isize[dir].a = (uint64_t*)realloc(isize[dir].a, 8 * isize[dir].m);
			}
			isize[dir].a[isize[dir].n++] = is;
		}
	}
	for (d = 0; d < 4; ++d) {
		ora_pestat_t *r = &pes[d];
		uint64_t *q = isize[d].a;
		size_t qn = isize[d].n;
		int p25, p50, p75, x;
		if (qn < 10) { r->failed = 1; free(q); isize[d].a = 0; continue; }   /* MIN_DIR_CNT */
		ora_sort_u64(qn, q);
		p25 = (int)q[(int)(.25 * qn + .499)];
		p50 = (int)q[(int)(.50 * qn + .499)];
		p75 = (int)q[(int)(.75 * qn + .499)];
		(void)p50;
		r->low = (int)(p25 - 2.0 * (p75 - p25) + .499);              /* OUTLIER_BOUND */
		if (r->low < 1) r->low = 1;
		r->high = (int)(p75 + 2.0 * (p75 - p25) + .499);
		for (i = x = 0, r->avg = 0; i < (int)qn; ++i)
			if (q[i] >= (uint64_t)r->low && q[i] <= (uint64_t)r->high) r->avg += q[i], ++x;
		r->avg /= x;
		for (i = 0, r->std = 0; i < (int)qn; ++i)
			if (q[i] >= (uint64_t)r->low && q[i] <= (uint64_t)r->high) r->std += (q[i] - r->avg) * (q[i] - r->avg);
		r->std = sqrt(r->std / x);
		r->low = (int)(p25 - 3.0 * (p75 - p25) + .499);              /* MAPPING_BOUND */
		r->high = (int)(p75 + 3.0 * (p75 - p25) + .499);
		if (r->low > r->avg - 4.0 * r->std) r->low = (int)(r->avg - 4.0 * r->std + .499);    /* MAX_STDDEV */
		if (r->high < r->avg + 4.0 * r->std) r->high = (int)(r->avg + 4.0 * r->std + .499);
		if (r->low < 1) r->low = 1;
		free(q); isize[d].a = 0;
	}
	for (d = 0, max = 0; d < 4; ++d) max = max > (int)isize[d].n ? max : (int)isize[d].n;
	for (d = 0; d < 4; ++d)
		if (pes[d].failed == 0 && isize[d].n < max * 0.05) pes[d].failed = 1;   /* MIN_DIR_RATIO */
}

int ora_matesw(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], const ora_reg_t *a, int l_ms, const uint8_t *ms, ora_reg_v *ma)   /* bwamem_pair.c:137 */
{
	int64_t l_pac = ref->l_pac;
	int i, r, skip[4], n = 0, rid = -1;
	for (r = 0; r < 4; ++r) skip[r] = pes[r].failed ? 1 : 0;
	for (i = 0; i < ma->n; ++i) {
		int64_t dist;
		r = infer_dir(l_pac, a->rb, ma->a[i].rb, &dist);
		if (dist >= pes[r].low && dist <= pes[r].high) skip[r] = 1;
	}
	if (skip[0] + skip[1] + skip[2] + skip[3] == 4) return 0;
	for (r = 0; r < 4; ++r) {
		int is_rev, is_larger;
		uint8_t *seq, *rev = 0, *ref_seq = 0;
		int64_t rb, re;
		if (skip[r]) continue;
		is_rev = (r >> 1 != (r & 1));
		is_larger = !(r >> 1);
		if (is_rev) {
			rev = (uint8_t*)malloc(l_ms);
			for (i = 0; i < l_ms; ++i) rev[l_ms - 1 - i] = ms[i] < 4 ? 3 - ms[i] : 4;
			seq = rev;
		} else seq = (uint8_t*)ms;
		if (!is_rev) {
			rb = is_larger ? a->rb + pes[r].low : a->rb - pes[r].high;
			re = (is_larger ? a->rb + pes[r].high : a->rb - pes[r].low) + l_ms;
		} else {
			rb = (is_larger ? a->rb + pes[r].low : a->rb - pes[r].high) - l_ms;
			re = is_larger ? a->rb + pes[r].high : a->rb - pes[r].low;
		}
		if (rb < 0) rb = 0;
		if (re > l_pac << 1) re = l_pac << 1;
		if (rb < re) ref_seq = ora_fetch_seq(ref, &rb, (rb + re) >> 1, &re, &rid);
		if (a->rid == rid && re - rb >= opt->min_seed_len) {
			ora_kswr_t aln;
			ora_reg_t b;
			int tmp, xtra = ORA_KSW_XSUBO | ORA_KSW_XSTART | (l_ms * opt->a < 250 ? ORA_KSW_XBYTE : 0) | (opt->min_seed_len * opt->a);
			aln = ora_ksw_align2(l_ms, seq, (int)(re - rb), ref_seq, 5, opt->mat, opt->o_del, opt->e_del, opt->o_ins, opt->e_ins, xtra);
			memset(&b, 0, sizeof(b));
			if (aln.score >= opt->min_seed_len && aln.qb >= 0) {
				b.rid = a->rid;
				b.is_alt = a->is_alt;
				b.qb = is_rev ? l_ms - (aln.qe + 1) : aln.qb;
				b.qe = is_rev ? l_ms - aln.qb : aln.qe + 1;
				b.rb = is_rev ? (l_pac << 1) - (rb + aln.te + 1) : rb + aln.tb;
				b.re = is_rev ? (l_pac << 1) - (rb + aln.tb) : rb + aln.te + 1;
				b.score = aln.score;
				b.csub = aln.score2;
				b.secondary = -1;
				b.seedcov = (int)((b.re - b.rb < b.qe - b.qb ? b.re - b.rb : b.qe - b.qb) >> 1);
				if (ma->n == ma->m) { ma->m = ma->m ? ma->m << 1 : 2; ma->a = (ora_reg_t*)realloc(ma->a, ma->m * sizeof(ora_reg_t)); }
				ma->a[ma->n++] = b;
				for (i = 0; i < ma->n - 1; ++i)
					if (ma->a[i].score < b.score) break;
				tmp = i;
				for (i = ma->n - 1; i > tmp; --i) ma->a[i] = ma->a[i-1];
				ma->a[i] = b;
			}
			++n;
		}
		if (n) ma->n = ora_sort_dedup_patch(opt, 0, 0, ma->n, ma->a);
		free(rev);
		free(ref_seq);
	}
	return n;
}

static void kat_get(ora_reg_t *p, const int64_t *x)   /* a region from its 19 words (dump_regs' order, main_oracle.c) */
{
	uint32_t u = (uint32_t)x[18];
	memset(p, 0, sizeof(ora_reg_t));
	p->rb = x[0]; p->re = x[1]; p->qb = (int)x[2]; p->qe = (int)x[3]; p->rid = (int)x[4]; p->score = (int)x[5]; p->truesc = (int)x[6];
	p->sub = (int)x[7]; p->alt_sc = (int)x[8]; p->csub = (int)x[9]; p->sub_n = (int)x[10]; p->w = (int)x[11]; p->seedcov = (int)x[12];
	p->secondary = (int)x[13]; p->secondary_all = (int)x[14]; p->seedlen0 = (int)x[15]; p->n_comp = (int)x[16]; p->is_alt = (int)x[17];
	memcpy(&p->frac_rep, &u, 4);
}

/* Test helper (tests/mate_insert_cases.py): the list update of ora_matesw above, lines "ma->a[ma->n++] = b" to the call of
 * ora_sort_dedup_patch, replayed on a caller's list.  start19 / step19 / out19: 19 words per region in dump_regs' order (main_oracle.c);
 * hit[t] != 0: step t is an orientation whose alignment gave region t of step19, 0: an orientation that was tried without a hit -- the
 * call at its end is made either way.  out19 has room for n + n_steps regions; returns the final length. */
int ora_kat_mate_insert(int max_chain_gap, float mask_level_redun, int n, const int64_t *start19, int n_steps, const int *hit, const int64_t *step19, int64_t *out19)
{
	ora_opt_t opt;
	ora_reg_t *a = (ora_reg_t*)calloc((size_t)(n + n_steps + 1), sizeof(ora_reg_t));
	int i, t, tmp;
	memset(&opt, 0, sizeof opt);
	opt.max_chain_gap = max_chain_gap; opt.mask_level_redun = mask_level_redun;
	for (i = 0; i < n; ++i) kat_get(&a[i], start19 + 19 * i);
	for (t = 0; t < n_steps; ++t) {
		if (hit[t]) {
			ora_reg_t b;
			kat_get(&b, step19 + 19 * t);
			a[n++] = b;
			for (i = 0; i < n - 1; ++i)
				if (a[i].score < b.score) break;
			tmp = i;
			for (i = n - 1; i > tmp; --i) a[i] = a[i-1];
			a[i] = b;
		}
		n = ora_sort_dedup_patch(&opt, 0, 0, n, a);
	}
	for (i = 0; i < n; ++i) {
		const ora_reg_t *p = &a[i];
		int64_t *w = out19 + 19 * i;
		uint32_t u;
		memcpy(&u, &p->frac_rep, 4);
		w[0] = p->rb; w[1] = p->re; w[2] = p->qb; w[3] = p->qe; w[4] = p->rid; w[5] = p->score; w[6] = p->truesc; w[7] = p->sub; w[8] = p->alt_sc; w[9] = p->csub;
		w[10] = p->sub_n; w[11] = p->w; w[12] = p->seedcov; w[13] = p->secondary; w[14] = p->secondary_all; w[15] = p->seedlen0; w[16] = p->n_comp; w[17] = p->is_alt; w[18] = u;
	}
	free(a);
	return n;
}

/* st (may be NULL): what a test wants to know beyond mem_pair's results -- the sizes of v and u, the (k, i) of u's two largest elements */
int ora_pair_ex(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], ora_read_t s[2], ora_reg_v a[2], int id,
                int *sub, int *n_sub, int z[2], int n_pri[2], ora_pair_stat_t *st)   /* bwamem_pair.c:208 */
{
	struct { size_t n, m; ora_pair64_t *a; } v = { 0, 0, 0 }, u = { 0, 0, 0 };
	int r, i, k, y[4], ret;
	int64_t l_pac = ref->l_pac;
	(void)s;
	for (r = 0; r < 2; ++r) {
		for (i = 0; i < n_pri[r]; ++i) {
			ora_pair64_t key;
			ora_reg_t *e = &a[r].a[i];
			key.x = e->rb < l_pac ? e->rb : (l_pac << 1) - 1 - e->rb;
			key.x = (uint64_t)e->rid << 32 | (key.x - ref->anns[e->rid].offset);
			key.y = (uint64_t)e->score << 32 | i << 2 | (e->rb >= l_pac) << 1 | r;
			if (v.n == v.m) { v.m = v.m ? v.m << 1 : 2; v.a = (ora_pair64_t*)realloc(v.a, v.m * sizeof(ora_pair64_t)); }
			v.a[v.n++] = key;
		}
	}
	ora_sort_pair64(v.n, v.a);
	y[0] = y[1] = y[2] = y[3] = -1;
	for (i = 0; i < (int)v.n; ++i) {
		for (r = 0; r < 2; ++r) {
			int dir = r << 1 | (v.a[i].y >> 1 & 1), which;
			if (pes[dir].failed) continue;
			which = r << 1 | ((v.a[i].y & 1) ^ 1);
			if (y[which] < 0) continue;
			for (k = y[which]; k >= 0; --k) {
				int64_t dist;
				int q;
				double ns;
				ora_pair64_t *p;
				if ((int)(v.a[k].y & 3) != which) continue;
				dist = (int64_t)v.a[i].x - v.a[k].x;
				if (dist > pes[dir].high) break;
				if (dist < pes[dir].low) continue;
				ns = (dist - pes[dir].avg) / pes[dir].std;
				q = (int)((v.a[i].y >> 32) + (v.a[k].y >> 32) + .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * opt->a + .499);
				if (q < 0) q = 0;
				if (u.n == u.m) { u.m = u.m ? u.m << 1 : 2; u.a = (ora_pair64_t*)realloc(u.a, u.m * sizeof(ora_pair64_t)); }
				p = &u.a[u.n++];
				p->y = (uint64_t)k << 32 | i;
				p->x = (uint64_t)q << 32 | (ora_hash64(p->y ^ id << 8) & 0xffffffffU);   /* `id<<8` binds before `^` */
			}
		}
		y[v.a[i].y & 3] = i;
	}
	if (u.n) {
		int tmp = opt->a + opt->b;
		tmp = tmp > opt->o_del + opt->e_del ? tmp : opt->o_del + opt->e_del;
		tmp = tmp > opt->o_ins + opt->e_ins ? tmp : opt->o_ins + opt->e_ins;
		ora_sort_pair64(u.n, u.a);
		if (st) {
			st->best[0] = (int)(u.a[u.n-1].y >> 32); st->best[1] = (int)(u.a[u.n-1].y & 0xffffffffU);
			if (u.n > 1) { st->second[0] = (int)(u.a[u.n-2].y >> 32); st->second[1] = (int)(u.a[u.n-2].y & 0xffffffffU); }
		}
		i = u.a[u.n-1].y >> 32; k = u.a[u.n-1].y << 32 >> 32;
		z[v.a[i].y & 1] = v.a[i].y << 32 >> 34;
		z[v.a[k].y & 1] = v.a[k].y << 32 >> 34;
		ret = u.a[u.n-1].x >> 32;
		*sub = u.n > 1 ? u.a[u.n-2].x >> 32 : 0;
		for (i = (long)u.n - 2, *n_sub = 0; i >= 0; --i)
			if (*sub - (int)(u.a[i].x >> 32) <= tmp) ++*n_sub;
	} else ret = 0, *sub = 0, *n_sub = 0;
	if (st) { st->nv = (int)v.n; st->n_u = (int)u.n; }
	free(u.a); free(v.a);
	return ret;
}

int ora_pair(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], ora_read_t s[2], ora_reg_v a[2], int id,
             int *sub, int *n_sub, int z[2], int n_pri[2])   /* bwamem_pair.c:208 */
{
	return ora_pair_ex(opt, ref, pes, s, a, id, sub, n_sub, z, n_pri, 0);
}

#define RAW_MAPQ(diff, a) ((int)(6.02 * (diff) / (a) + .499))   /* bwamem_pair.c:274 */

/* stage records (ora.h): inert while ora_pe_dump is NULL */
ora_pe_dump_t *ora_pe_dump = 0;
static void dump_lists(ora_reg_v *to, uint64_t id, const ora_reg_v a[2])
{
	int i;
	for (i = 0; i < 2; ++i) {
		ora_reg_v *d = &to[(id - ora_pe_dump->id0) << 1 | i];
		d->n = d->m = a[i].n;
		d->a = (ora_reg_t*)malloc((a[i].n ? a[i].n : 1) * sizeof(ora_reg_t));
		if (a[i].n) memcpy(d->a, a[i].a, a[i].n * sizeof(ora_reg_t));
	}
}
static void dump_pair(uint64_t id, int paired, const int z[2], const int alt[2], const int q_se[2], int extra_flag, int o, int subo, int n_sub)
{
	int i;
	for (i = 0; i < 2; ++i) {
		int64_t *p = ora_pe_dump->pair[(id - ora_pe_dump->id0) << 1 | i];
		p[0] = paired; p[1] = z[i]; p[2] = alt[i]; p[3] = q_se[i]; p[4] = extra_flag; p[5] = o; p[6] = subo; p[7] = n_sub;
	}
}

/* The decisions of mem_sam_pe between the marked lists and the records (bwamem_pair.c:311-365, 397-411), in one place for ora_sam_pe and
 * ora_kat_pair: mem_pair, is_multi, score_un, q_pe, q_se, the sub adopted from a secondary z[i], the re-parenting of secondary_all, the
 * ALT hit printed beside z[i], and the no-pairing branch's choice of h[i].  a[]: marked (and, under -5, reordered) lists; updated as
 * mem_sam_pe updates them. */
void ora_pe_decide(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], uint64_t id, ora_reg_v a[2], int n_pri[2], ora_pe_dec_t *d)
{
	int i, j, z[2];
	memset(d, 0, sizeof *d);
	d->extra_flag = 1;
	d->alt[0] = d->alt[1] = -1;
	d->st.zraw[0] = d->st.zraw[1] = -1;
	d->st.best[0] = d->st.best[1] = d->st.second[0] = d->st.second[1] = -1;
	if (!(opt->flag & ORA_F_NOPAIRING) && n_pri[0] && n_pri[1]) {
		int subo, is_multi[2];
		z[0] = z[1] = -1;
		d->ran = 1;
		d->o = ora_pair_ex(opt, ref, pes, 0, a, (int)id, &d->subo, &d->n_sub, z, n_pri, &d->st);
		d->st.zraw[0] = z[0]; d->st.zraw[1] = z[1];
		subo = d->subo;
		for (i = 0; i < 2; ++i) {
			for (j = 1; j < n_pri[i]; ++j)
				if (a[i].a[j].secondary < 0 && a[i].a[j].score >= opt->T) break;
			is_multi[i] = j < n_pri[i] ? 1 : 0;
		}
		d->is_multi = is_multi[0] | is_multi[1] << 1;
		if (d->o > 0 && !is_multi[0] && !is_multi[1]) {
			int q_pe, score_un, q_se[2], o = d->o, n_sub = d->n_sub;
			d->paired = 1;
			score_un = a[0].a[0].score + a[1].a[0].score - opt->pen_unpaired;
			d->has_un = 1; d->o_un = o - score_un;
			subo = subo > score_un ? subo : score_un;
			q_pe = RAW_MAPQ(o - subo, opt->a);
			if (n_sub > 0) q_pe -= (int)(4.343 * log(n_sub + 1) + .499);
			if (q_pe < 0) q_pe = 0;
			if (q_pe > 60) q_pe = 60;
			q_pe = (int)(q_pe * (1. - .5 * (a[0].a[0].frac_rep + a[1].a[0].frac_rep)) + .499);
			if (o > score_un) {
				ora_reg_t *c[2];
				c[0] = &a[0].a[z[0]]; c[1] = &a[1].a[z[1]];
				for (i = 0; i < 2; ++i) {
					if (c[i]->secondary >= 0) c[i]->sub = a[i].a[c[i]->secondary].score, c[i]->secondary = -2;
					q_se[i] = ora_approx_mapq_se(opt, c[i]);
				}
				q_se[0] = q_se[0] > q_pe ? q_se[0] : q_pe < q_se[0] + 40 ? q_pe : q_se[0] + 40;
				q_se[1] = q_se[1] > q_pe ? q_se[1] : q_pe < q_se[1] + 40 ? q_pe : q_se[1] + 40;
				d->extra_flag |= 2;
				q_se[0] = q_se[0] < RAW_MAPQ(c[0]->score - c[0]->csub, opt->a) ? q_se[0] : RAW_MAPQ(c[0]->score - c[0]->csub, opt->a);
				q_se[1] = q_se[1] < RAW_MAPQ(c[1]->score - c[1]->csub, opt->a) ? q_se[1] : RAW_MAPQ(c[1]->score - c[1]->csub, opt->a);
			} else {
				z[0] = z[1] = 0;
				q_se[0] = ora_approx_mapq_se(opt, &a[0].a[0]);
				q_se[1] = ora_approx_mapq_se(opt, &a[1].a[0]);
			}
			for (i = 0; i < 2; ++i) {
				int k = a[i].a[z[i]].secondary_all;
				if (k >= 0 && k < n_pri[i]) {
					assert(a[i].a[k].secondary_all < 0);
					for (j = 0; j < a[i].n; ++j)
						if (a[i].a[j].secondary_all == k || j == k) a[i].a[j].secondary_all = z[i];
					a[i].a[z[i]].secondary_all = -1;
					++d->n_reparent;
				}
			}
			for (i = 0; i < 2; ++i) {
				const ora_reg_t *p = &a[i].a[n_pri[i]];
				d->alt[i] = n_pri[i] < a[i].n && !(p->score < opt->T || p->secondary >= 0 || !p->is_alt) ? n_pri[i] : -1;
				d->z[i] = z[i]; d->q_se[i] = q_se[i];
			}
			return;
		}
	}
	for (i = 0; i < 2; ++i) {                                   /* no pairing (bwamem_pair.c:397-411): the region h[i] is made of */
		int which = -1;
		if (a[i].n) {
			if (a[i].a[0].score >= opt->T) which = 0;
			else if (n_pri[i] < a[i].n && a[i].a[n_pri[i]].score >= opt->T) which = n_pri[i];
		}
		d->z[i] = which;
	}
}

int ora_sam_pe(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], uint64_t id, ora_read_t s[2], ora_reg_v a[2])   /* bwamem_pair.c:276 */
{
	int n = 0, i, j, n_pri[2], n_aa[2];
	ora_str_t str = { 0, 0, 0 };
	ora_aln_t h[2], g[2], aa[2][2];
	ora_pe_dec_t d;
	memset(h, 0, sizeof h); memset(g, 0, sizeof g);
	n_aa[0] = n_aa[1] = 0;
	if (ora_pe_dump) dump_lists(ora_pe_dump->se, id, a);
	if (!(opt->flag & ORA_F_NO_RESCUE)) {
		ora_reg_v b[2] = { { 0, 0, 0 }, { 0, 0, 0 } };
		for (i = 0; i < 2; ++i)
			for (j = 0; j < a[i].n; ++j)
				if (a[i].a[j].score >= a[i].a[0].score - opt->pen_unpaired) {
					if (b[i].n == b[i].m) { b[i].m = b[i].m ? b[i].m << 1 : 2; b[i].a = (ora_reg_t*)realloc(b[i].a, b[i].m * sizeof(ora_reg_t)); }
					b[i].a[b[i].n++] = a[i].a[j];
				}
		for (i = 0; i < 2; ++i)
			for (j = 0; j < b[i].n && j < opt->max_matesw; ++j)
				n += ora_matesw(opt, ref, pes, &b[i].a[j], s[!i].l_seq, (uint8_t*)s[!i].seq, &a[!i]);
		free(b[0].a); free(b[1].a);
	}
	if (ora_pe_dump) dump_lists(ora_pe_dump->pe, id, a);
	n_pri[0] = ora_mark_primary_se(opt, a[0].n, a[0].a, id << 1 | 0);
	n_pri[1] = ora_mark_primary_se(opt, a[1].n, a[1].a, id << 1 | 1);
	if (opt->flag & ORA_F_PRIMARY5) { ora_reorder_primary5(opt->T, &a[0]); ora_reorder_primary5(opt->T, &a[1]); }
	ora_pe_decide(opt, ref, pes, id, a, n_pri, &d);
	if (d.paired) {
		char **XA[2];
		if (ora_pe_dump) dump_pair(id, 1, d.z, d.alt, d.q_se, d.extra_flag, d.o, d.subo, d.n_sub);
		if (!(opt->flag & ORA_F_ALL)) {
			for (i = 0; i < 2; ++i) XA[i] = ora_gen_alt(opt, ref, &a[i], s[i].l_seq, s[i].seq);
		} else XA[0] = XA[1] = 0;
		for (i = 0; i < 2; ++i) {
			h[i] = ora_reg2aln(opt, ref, s[i].l_seq, s[i].seq, &a[i].a[d.z[i]]);
			h[i].mapq = (uint32_t)d.q_se[i] & 0xff;
			h[i].flag |= 0x40 << i | d.extra_flag;
			h[i].XA = XA[i] ? XA[i][d.z[i]] : 0;
			aa[i][n_aa[i]++] = h[i];
			if (d.alt[i] >= 0) {
				g[i] = ora_reg2aln(opt, ref, s[i].l_seq, s[i].seq, &a[i].a[d.alt[i]]);
				g[i].flag |= 0x800 | 0x40 << i | d.extra_flag;
				g[i].XA = XA[i] ? XA[i][d.alt[i]] : 0;
				aa[i][n_aa[i]++] = g[i];
			}
		}
		for (i = 0; i < n_aa[0]; ++i) ora_aln2sam(opt, ref, &str, &s[0], n_aa[0], aa[0], i, &h[1]);
		s[0].sam = strdup(str.s); str.l = 0;
		for (i = 0; i < n_aa[1]; ++i) ora_aln2sam(opt, ref, &str, &s[1], n_aa[1], aa[1], i, &h[0]);
		s[1].sam = str.s;
		if (strcmp(s[0].name, s[1].name) != 0) { fprintf(stderr, "[ora] paired reads have different names: \"%s\", \"%s\"\n", s[0].name, s[1].name); exit(1); }
		for (i = 0; i < 2; ++i) {
			free(h[i].cigar); free(g[i].cigar);
			if (XA[i] == 0) continue;
			for (j = 0; j < a[i].n; ++j) free(XA[i][j]);
			free(XA[i]);
		}
	} else {
		int extra_flag = d.extra_flag;
		for (i = 0; i < 2; ++i) {
			if (d.z[i] >= 0) h[i] = ora_reg2aln(opt, ref, s[i].l_seq, s[i].seq, &a[i].a[d.z[i]]);
			else h[i] = ora_reg2aln(opt, ref, s[i].l_seq, s[i].seq, 0);
		}
		if (ora_pe_dump) { const int none[2] = { -1, -1 }, zero[2] = { 0, 0 }; dump_pair(id, 0, d.z, none, zero, extra_flag, d.o, d.subo, d.n_sub); }
		if (!(opt->flag & ORA_F_NOPAIRING) && h[0].rid == h[1].rid && h[0].rid >= 0) {
			int64_t dist;
			int dir = infer_dir(ref->l_pac, a[0].a[0].rb, a[1].a[0].rb, &dist);
			if (!pes[dir].failed && dist >= pes[dir].low && dist <= pes[dir].high) extra_flag |= 2;
		}
		ora_reg2sam(opt, ref, &s[0], &a[0], 0x41 | extra_flag, &h[1]);
		ora_reg2sam(opt, ref, &s[1], &a[1], 0x81 | extra_flag, &h[0]);
		if (strcmp(s[0].name, s[1].name) != 0) { fprintf(stderr, "[ora] paired reads have different names: \"%s\", \"%s\"\n", s[0].name, s[1].name); exit(1); }
		free(h[0].cigar); free(h[1].cigar);
	}
	return n;
}

static void kat_put(int64_t *w, const ora_reg_t *p)   /* a region as its 19 words */
{
	uint32_t u;
	memcpy(&u, &p->frac_rep, 4);
	w[0] = p->rb; w[1] = p->re; w[2] = p->qb; w[3] = p->qe; w[4] = p->rid; w[5] = p->score; w[6] = p->truesc; w[7] = p->sub; w[8] = p->alt_sc; w[9] = p->csub;
	w[10] = p->sub_n; w[11] = p->w; w[12] = p->seedcov; w[13] = p->secondary; w[14] = p->secondary_all; w[15] = p->seedlen0; w[16] = p->n_comp; w[17] = p->is_alt; w[18] = u;
}

/* Test helper (`bwa_oracle katpair`): what mem_sam_pe decides about one pair of caller-supplied region lists without aligning anything --
 * ora_mark_primary_se of both ends (ids pair_id << 1 | end), ora_reorder_primary5 under -5, ora_pe_decide, and the selection as
 * mem_sam_pe uses it: paired, ora_select's XA membership (what ora_gen_alt lists) kept for the records of z[i] and the ALT hit; not
 * paired, ora_select as ora_reg2sam uses it and need 4 for the region of h[i] where it prints nothing itself.
 * regs19[e]: n[e] regions in the 19-word layout of the stage records.
 * marked[e]: 2 + 19 n[e] words -- n, n_pri, the lists as marked, before any decision (what `bwaref katpair` can give);
 * out[e]: 12 + 22 n[e] words -- the 8 words of the paired-end stage record, n, n_pri, regions with a task, regions with a record, then per
 *   region in the final order the 19 words as mem_sam_pe left them, the index the region had in regs19 (through the hash), need, XA owner;
 * pair5: mem_pair's ret, sub, n_sub and raw z[2] (-1: not set; 0 0 0 -1 -1 when it did not run);
 * extra: nv, the size of u, (k, i) of the best and of the second element of u (-1: none), 1 and o - score_un where that was compared
 *   (else 0 0), the is_multi bits, the number of ends re-parented. */
void ora_kat_pair(const ora_opt_t *opt, const ora_ref_t *ref, const ora_pestat_t pes[4], int64_t pair_id, const int n[2], const int64_t *const regs19[2],
                  int64_t *marked[2], int64_t *out[2], int64_t pair5[5], int64_t extra[ORA_KAT_PAIR_EXTRA])
{
	ora_reg_v a[2];
	ora_pe_dec_t d;
	int e, i, j, n_pri[2];
	for (e = 0; e < 2; ++e) {
		a[e].n = a[e].m = n[e]; a[e].a = (ora_reg_t*)calloc(n[e] ? n[e] : 1, sizeof(ora_reg_t));
		for (i = 0; i < n[e]; ++i) kat_get(&a[e].a[i], regs19[e] + 19 * i);
		n_pri[e] = ora_mark_primary_se(opt, n[e], a[e].a, pair_id << 1 | e);
	}
	if (opt->flag & ORA_F_PRIMARY5) { ora_reorder_primary5(opt->T, &a[0]); ora_reorder_primary5(opt->T, &a[1]); }
	for (e = 0; e < 2; ++e) {
		marked[e][0] = n[e]; marked[e][1] = n_pri[e];
		for (i = 0; i < n[e]; ++i) kat_put(marked[e] + 2 + 19 * i, &a[e].a[i]);
	}
	ora_pe_decide(opt, ref, pes, (uint64_t)pair_id, a, n_pri, &d);
	pair5[0] = d.o; pair5[1] = d.subo; pair5[2] = d.n_sub; pair5[3] = d.st.zraw[0]; pair5[4] = d.st.zraw[1];
	extra[0] = d.st.nv; extra[1] = d.st.n_u; extra[2] = d.st.best[0]; extra[3] = d.st.best[1]; extra[4] = d.st.second[0]; extra[5] = d.st.second[1];
	extra[6] = d.has_un; extra[7] = d.o_un; extra[8] = d.is_multi; extra[9] = d.n_reparent;
	for (e = 0; e < 2; ++e) {
		const int m = n[e];
		uint8_t *need = (uint8_t*)calloc(m ? m : 1, 1);
		int *owner = (int*)calloc(m ? m : 1, sizeof(int));
		int n_task = 0, n_rec = 0;
		int64_t *o = out[e];
		if (d.paired) {
			ora_select(opt, m, a[e].a, !(opt->flag & ORA_F_ALL), need, owner);
			for (i = 0; i < m; ++i) {
				int nd = 0;
				if (i == d.z[e] || i == d.alt[e]) nd |= ORA_NEED_REC;
				if ((need[i] & ORA_NEED_XA) && (owner[i] == d.z[e] || owner[i] == d.alt[e])) nd |= ORA_NEED_XA; else owner[i] = -1;
				need[i] = (uint8_t)nd;
			}
			n_rec = 1 + (d.alt[e] >= 0);
		} else if (m > 0) {
			ora_select(opt, m, a[e].a, !(opt->flag & ORA_F_ALL), need, owner);
			for (i = 0; i < m; ++i) n_rec += (need[i] & ORA_NEED_REC) != 0;
			if (d.z[e] >= 0 && need[d.z[e]] == 0) need[d.z[e]] = 4;
		}
		for (i = 0; i < m; ++i) n_task += need[i] != 0;
		o[0] = d.paired; o[1] = d.z[e]; o[2] = d.alt[e]; o[3] = d.paired ? d.q_se[e] : 0; o[4] = d.paired ? d.extra_flag : 1; o[5] = d.o; o[6] = d.subo; o[7] = d.n_sub;
		o[8] = m; o[9] = n_pri[e]; o[10] = n_task; o[11] = n_rec;
		for (i = 0; i < m; ++i) {
			int64_t *w = o + 12 + 22 * i;
			const uint64_t id = (uint64_t)pair_id << 1 | e;
			kat_put(w, &a[e].a[i]);
			for (j = 0; j < m && ora_hash64(id + j) != a[e].a[i].hash; ++j);
			w[19] = j < m ? j : -1; w[20] = need[i]; w[21] = owner[i];
		}
		free(need); free(owner); free(a[e].a);
	}
}
