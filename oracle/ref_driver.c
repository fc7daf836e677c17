/* TEST INFRASTRUCTURE ONLY -- never linked into, or called from, the product.
 *
 * Driver around the *reference's own* CPU implementation (the stock bwa 0.7.17
 * path that still lives in /root/reference: bwamem.c, bwt.c, ksw.c, bntseq.c,
 * bwa.c, bwamem_pair.c, bwamem_extra.c ...).  The reference sources are
 * compiled where they lie by oracle/Makefile; only this file is ours.  It is
 * used to (a) pin the C restatement in oracle/ and (b) generate the golden
 * vectors committed under tests/golden/.
 *
 * We #include the reference's bwamem.c into this translation unit (instead of
 * linking bwamem.o) for one reason: mem_collect_intv (bwamem.c:137) is static
 * and the per-stage dump needs it.
 *
 * Sub-commands
 *   index  <in.fa> <prefix>                      bwa_idx_build (bwtindex.c:255)
 *   mem    [-p] [-t N] [-K bases] <prefix> <r1.fq> [r2.fq]   SAM body on stdout
 *   stages <prefix> <reads.fq> <out.bin>         per-read stage dump (SE)
 *   katfm  <prefix> <out.bin> <n> <seed>         known answers: occ4/extend/sa
 *   katksw <out.bin> <n> <seed>                  known answers: ksw_extend2 /
 *                                                ksw_global2 / ksw_align2
 *   katalign <out.bin> <n> <seed>                known answers: ksw_align2 under
 *                                                other matrices / gap costs / xtra
 *   katdp  <out.bin> <n> <seed>                  known answers: ksw_extend2 / ksw_global2 over
 *                                                the whole range of lengths, bands, matrices
 *   katchain [options] <prefix> <cases.bin> <out.bin>   known answers: chains and filtered chains of given seed lists
 *   katdedup [options] <prefix> <cases.bin> <out.bin>   known answers: mem_sort_dedup_patch of given region lists
 *   katmark [options] <prefix> <cases.bin> <out.bin>    known answers: primary marking and mapQ of given region lists
 *   katpair [options] <prefix> <cases.bin> <out.bin>    known answers: mem_pair on given pairs of region lists
 *
 * Dump format ("i64 records"): a stream of  [tag:i64][n:i64][n x i64].
 */
#include "bwamem.c" /* reference source, found through -I/root/reference */
#include <zlib.h>
#include <sys/time.h>
static double now_s(void) { struct timeval tv; gettimeofday(&tv, 0); return tv.tv_sec + tv.tv_usec * 1e-6; }
#include <unistd.h>
#include "kseq.h"
KSEQ_DECLARE(gzFile)

extern int bwa_idx_build(const char *fa, const char *prefix, int algo_type, int block_size);
#define OPT_T mem_opt_t
#define PES_T mem_pestat_t
#define OPT_FILL_SCMAT(a, b, mat) bwa_fill_scmat((a), (b), (mat))
#define OPT_LOG(x) log(x)
#include "opt_parse.h"
#include "kat_mark_io.h"
#include "kat_dedup_io.h"
#include "kat_pair_io.h"

/* ---------------------------------------------------------------- records */
static void rec_write(FILE *fp, int64_t tag, int64_t n, const int64_t *v)
{
	fwrite(&tag, 8, 1, fp); fwrite(&n, 8, 1, fp);
	if (n) fwrite(v, 8, n, fp);
}
typedef struct { int64_t n, m; int64_t *a; } i64v;
static inline void push(i64v *v, int64_t x)
{
	if (v->n == v->m) { v->m = v->m ? v->m << 1 : 256; v->a = realloc(v->a, v->m * 8); }
	v->a[v->n++] = x;
}
static inline int64_t f2i(float f) { uint32_t u; memcpy(&u, &f, 4); return (int64_t)u; }

enum { TAG_READ = 100, TAG_INTV = 1, TAG_CHAIN = 2, TAG_CHAIN_FLT = 3, TAG_REGS_PRE = 5, TAG_REGS = 4,
       TAG_OCC4 = 10, TAG_EXTEND = 11, TAG_SA = 12, TAG_KSW_EXT = 20, TAG_KSW_GLB = 21, TAG_KSW_ALN = 22, TAG_KSW_ALN2 = 23 };

static void dump_chains(FILE *fp, int64_t tag, int n, const mem_chain_t *a)
{
	i64v v = {0, 0, 0};
	int i, j;
	push(&v, n);
	for (i = 0; i < n; ++i) {
		const mem_chain_t *c = &a[i];
		push(&v, c->pos); push(&v, c->rid); push(&v, c->is_alt); push(&v, c->w); push(&v, c->kept);
		push(&v, c->first); push(&v, f2i(c->frac_rep)); push(&v, c->n);
		for (j = 0; j < c->n; ++j) {
			push(&v, c->seeds[j].rbeg); push(&v, c->seeds[j].qbeg);
			push(&v, c->seeds[j].len); push(&v, c->seeds[j].score);
		}
	}
	rec_write(fp, tag, v.n, v.a);
	free(v.a);
}

static void dump_regs(FILE *fp, int64_t tag, int n, const mem_alnreg_t *a)
{
	i64v v = {0, 0, 0};
	int i;
	push(&v, n);
	for (i = 0; i < n; ++i) {
		const mem_alnreg_t *p = &a[i];
		push(&v, p->rb); push(&v, p->re); push(&v, p->qb); push(&v, p->qe); push(&v, p->rid);
		push(&v, p->score); push(&v, p->truesc); push(&v, p->sub); push(&v, p->alt_sc); push(&v, p->csub);
		push(&v, p->sub_n); push(&v, p->w); push(&v, p->seedcov); push(&v, p->secondary);
		push(&v, p->secondary_all); push(&v, p->seedlen0); push(&v, p->n_comp); push(&v, p->is_alt);
		push(&v, f2i(p->frac_rep));
	}
	rec_write(fp, tag, v.n, v.a);
	free(v.a);
}

/* ------------------------------------------------------------------- index */
static int main_index(int argc, char **argv)
{
	if (argc < 3) return 1;
	bwa_verbose = 1;
	return bwa_idx_build(argv[1], argv[2], 0, 10000000);
}

/* --------------------------------------------------------------------- mem */
static int main_mem(int argc, char **argv)
{
	mem_opt_t *opt = mem_opt_init();
	int c, n;
	int64_t n_processed = 0;
	double t_align = 0;
	bwaidx_t *idx;
	gzFile f1, f2 = 0;
	kseq_t *ks, *ks2 = 0;
	bseq1_t *seqs;
	optparse_t op;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 2 > argc) return 1;
	idx = bwa_idx_load(argv[optind], BWA_IDX_ALL);
	if (idx == 0) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->bns->n_seqs; ++c) idx->bns->anns[c].is_alt = 0;
	f1 = gzopen(argv[optind + 1], "r"); ks = kseq_init(f1);
	if (optind + 2 < argc && !op.smart_pe) { f2 = gzopen(argv[optind + 2], "r"); ks2 = kseq_init(f2); opt->flag |= MEM_F_PE; }
	strcpy(bwa_rg_id, op.rg_id);
	{
		int chunk = op.fixed_chunk > 0 ? op.fixed_chunk : opt->chunk_size * opt->n_threads; /* fastmap.c:304 */
		while ((seqs = bseq_read(chunk, &n, ks, ks2)) != 0) {
			int i;
			if (n == 0) { free(seqs); break; }
			if (!op.copy_comment) for (i = 0; i < n; ++i) { free(seqs[i].comment); seqs[i].comment = 0; } /* stock: no -C */
			if (op.align_only) { /* -Z: the first half of mem_process_seqs only (bwamem.c:1225-1232): kt_for(worker1) == mem_align1_core per read */
				extern void kt_for(int n_threads, void (*func)(void*,int,int), void *data, int n);
				worker_t w;
				double t0;
				w.regs = malloc(n * sizeof(mem_alnreg_v));
				w.opt = opt; w.bwt = idx->bwt; w.bns = idx->bns; w.pac = idx->pac; w.seqs = seqs; w.n_processed = n_processed; w.pes = 0;
				w.aux = malloc(opt->n_threads * sizeof(smem_aux_t*));
				for (i = 0; i < opt->n_threads; ++i) w.aux[i] = smem_aux_init();
				t0 = now_s();
				kt_for(opt->n_threads, worker1, &w, (opt->flag & MEM_F_PE) ? n >> 1 : n);
				t_align += now_s() - t0;
				for (i = 0; i < opt->n_threads; ++i) smem_aux_destroy(w.aux[i]);
				free(w.aux);
				for (i = 0; i < n; ++i) { free(w.regs[i].a); seqs[i].sam = 0; }
				free(w.regs);
			} else
			{ double t0 = now_s(); mem_process_seqs(opt, idx->bwt, idx->bns, idx->pac, n_processed, n, seqs, op.has_pes0 ? op.pes : 0); t_align += now_s() - t0; }
			n_processed += n;
			for (i = 0; i < n; ++i) {
				if (seqs[i].sam) fputs(seqs[i].sam, stdout);
				free(seqs[i].name); free(seqs[i].seq); free(seqs[i].qual); free(seqs[i].sam);
			}
			free(seqs);
		}
	}
	fprintf(stderr, "[bwaref] aligned %lld reads in %.3f s with %d threads (mem_process_seqs only)\n", (long long)n_processed, t_align, opt->n_threads);
	kseq_destroy(ks); gzclose(f1);
	if (ks2) { kseq_destroy(ks2); gzclose(f2); }
	bwa_idx_destroy(idx);
	free(opt);
	return 0;
}

/* ------------------------------------------------------------------ stages */
static int main_stages(int argc, char **argv)
{
	mem_opt_t *opt = mem_opt_init();
	bwaidx_t *idx;
	gzFile f1;
	kseq_t *ks;
	FILE *out;
	int64_t id = 0;
	optparse_t op;
	int c;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	argv += optind - 1;
	idx = bwa_idx_load(argv[1], BWA_IDX_ALL);
	if (idx == 0) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->bns->n_seqs; ++c) idx->bns->anns[c].is_alt = 0;
	f1 = gzopen(argv[2], "r"); ks = kseq_init(f1);
	out = fopen(argv[3], "wb");
	while (kseq_read(ks) >= 0) {
		int i, l_seq = ks->seq.l;
		char *seq = malloc(l_seq + 1);
		smem_aux_t *aux = smem_aux_init();
		mem_chain_v chn;
		mem_alnreg_v regs;
		int64_t hdr[2];
		i64v v = {0, 0, 0};
		memcpy(seq, ks->seq.s, l_seq + 1);
		for (i = 0; i < l_seq; ++i) seq[i] = seq[i] < 4 ? seq[i] : nst_nt4_table[(int)seq[i]]; /* bwamem.c:1067 */
		hdr[0] = id++; hdr[1] = l_seq;
		rec_write(out, TAG_READ, 2, hdr);
		/* stage 1: intervals (bwamem.c:137) */
		if (l_seq >= opt->min_seed_len) { /* mem_chain's guard, bwamem.c:267 */
			mem_collect_intv(opt, idx->bwt, l_seq, (uint8_t*)seq, aux);
			for (i = 0; i < aux->mem.n; ++i) {
				push(&v, aux->mem.a[i].x[0]); push(&v, aux->mem.a[i].x[1]);
				push(&v, aux->mem.a[i].x[2]); push(&v, aux->mem.a[i].info);
			}
		}
		rec_write(out, TAG_INTV, v.n, v.a);
		free(v.a);
		/* stage 2: chains (bwamem.c:258) */
		chn = mem_chain(opt, idx->bwt, idx->bns, l_seq, (uint8_t*)seq, aux);
		/* w, kept and first are not set before mem_chain_flt (mem_chain's `tmp` is a stack variable, bwamem.c:287): what they hold depends
		 * on how this file was compiled.  Dumped as 0, as the restatement has them; mem_chain_flt sets all three before it reads them. */
		for (i = 0; i < chn.n; ++i) { chn.a[i].w = 0; chn.a[i].kept = 0; chn.a[i].first = 0; }
		dump_chains(out, TAG_CHAIN, chn.n, chn.a);
		/* stage 3: filtered chains (bwamem.c:334, 605) */
		chn.n = mem_chain_flt(opt, chn.n, chn.a);
		mem_flt_chained_seeds(opt, idx->bns, idx->pac, l_seq, (uint8_t*)seq, chn.n, chn.a);
		dump_chains(out, TAG_CHAIN_FLT, chn.n, chn.a);
		/* stage 4: extension (bwamem.c:639) */
		kv_init(regs);
		for (i = 0; i < chn.n; ++i) {
			mem_chain2aln(opt, idx->bns, idx->pac, l_seq, (uint8_t*)seq, &chn.a[i], &regs);
			free(chn.a[i].seeds);
		}
		free(chn.a);
		dump_regs(out, TAG_REGS_PRE, regs.n, regs.a);
		/* stage 5: dedup/patch (bwamem.c:444) + is_alt (bwamem.c:1091) */
		regs.n = mem_sort_dedup_patch(opt, idx->bns, idx->pac, (uint8_t*)seq, regs.n, regs.a);
		for (i = 0; i < regs.n; ++i)
			if (regs.a[i].rid >= 0 && idx->bns->anns[regs.a[i].rid].is_alt) regs.a[i].is_alt = 1;
		dump_regs(out, TAG_REGS, regs.n, regs.a);
		free(regs.a);
		smem_aux_destroy(aux);
		free(seq);
	}
	fclose(out);
	kseq_destroy(ks); gzclose(f1);
	bwa_idx_destroy(idx);
	free(opt);
	return 0;
}

/* ------------------------------------------------------- known answers: FM */
static uint64_t rng_state;
static inline uint64_t rng(void)
{ /* splitmix64 */
	uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
	return z ^ (z >> 31);
}

static int main_katfm(int argc, char **argv)
{
	bwaidx_t *idx;
	FILE *out;
	int i, n;
	if (argc < 5) return 1;
	bwa_verbose = 1;
	idx = bwa_idx_load(argv[1], BWA_IDX_BWT);
	out = fopen(argv[2], "wb");
	n = atoi(argv[3]); rng_state = strtoull(argv[4], 0, 10);
	for (i = 0; i < n; ++i) {
		const bwt_t *bwt = idx->bwt;
		bwtint_t k = i == 0 ? (bwtint_t)-1 : i == 1 ? bwt->seq_len : i == 2 ? bwt->primary : i == 3 ? bwt->primary - 1 :
			i == 4 ? 0 : rng() % (bwt->seq_len + 1);
		bwtint_t cnt[4];
		int64_t r[8];
		bwt_occ4(bwt, k, cnt);
		r[0] = k; r[1] = cnt[0]; r[2] = cnt[1]; r[3] = cnt[2]; r[4] = cnt[3];
		rec_write(out, TAG_OCC4, 5, r);
		if (k != (bwtint_t)-1) {
			r[1] = bwt_sa(bwt, k);
			rec_write(out, TAG_SA, 2, r);
		}
	}
	for (i = 0; i < n; ++i) { /* random walks of bwt_extend in both directions */
		const bwt_t *bwt = idx->bwt;
		bwtintv_t ik, ok[4];
		int step, c0 = rng() & 3;
		bwt_set_intv(bwt, c0, ik);
		for (step = 0; step < 40 && ik.x[2] > 0; ++step) {
			int is_back = rng() & 1, c = rng() & 3, j;
			int64_t r[3 + 1 + 12];
			bwt_extend(bwt, &ik, ok, is_back);
			r[0] = ik.x[0]; r[1] = ik.x[1]; r[2] = ik.x[2]; r[3] = is_back;
			for (j = 0; j < 4; ++j) { r[4 + j*3] = ok[j].x[0]; r[5 + j*3] = ok[j].x[1]; r[6 + j*3] = ok[j].x[2]; }
			rec_write(out, TAG_EXTEND, 16, r);
			ik = ok[c];
		}
	}
	fclose(out);
	bwa_idx_destroy(idx);
	return 0;
}

/* ------------------------------------------------------ known answers: ksw */
static void rand_pair(int qlen, int tlen, int err_pct, uint8_t *q, uint8_t *t)
{ /* target = mutated copy of query, so alignments are non-trivial */
	int i, j = 0;
	for (i = 0; i < qlen; ++i) q[i] = rng() & 3;
	for (i = 0; i < tlen; ++i) {
		int r = rng() % 100;
		if (j >= qlen) { t[i] = rng() & 3; continue; }
		if (r < err_pct) { /* substitution / insertion / deletion, 1/3 each */
			int kind = rng() % 3;
			if (kind == 0) t[i] = (q[j] + 1 + rng() % 3) & 3, ++j;
			else if (kind == 1) t[i] = rng() & 3;
			else { j += 1 + rng() % 3; t[i] = j < qlen ? q[j] : (rng() & 3); ++j; }
		} else t[i] = q[j++];
		if ((rng() & 255) == 0) t[i] = 4; /* ambiguous base */
	}
}

static int main_katksw(int argc, char **argv)
{
	FILE *out;
	int i, n;
	int8_t mat[25];
	if (argc < 4) return 1;
	out = fopen(argv[1], "wb");
	n = atoi(argv[2]); rng_state = strtoull(argv[3], 0, 10);
	bwa_fill_scmat(1, 4, mat);
	for (i = 0; i < n; ++i) {
		int qlen = 1 + rng() % 250, tlen = qlen + (int)(rng() % 60) - 20, err = rng() % 12;
		int w = (rng() & 3) == 0 ? 5 + rng() % 20 : 100 << (rng() & 1);
		int h0 = 19 + rng() % 100, zdrop = (rng() & 7) == 0 ? 0 : 100, end_bonus = (rng() & 1) ? 5 : 0;
		int o_del = 6, e_del = 1, o_ins = 6, e_ins = 1;
		uint8_t *q, *t;
		i64v v = {0, 0, 0};
		int j, qle, tle, gtle, gscore, max_off, sc;
		if (tlen < 1) tlen = 1;
		if ((rng() & 15) == 0) { o_del = 4; e_del = 2; o_ins = 7; e_ins = 1; }
		q = malloc(qlen); t = malloc(tlen);
		rand_pair(qlen, tlen, err, q, t);
		/* inputs */
		push(&v, qlen); push(&v, tlen); push(&v, w); push(&v, h0); push(&v, zdrop); push(&v, end_bonus);
		push(&v, o_del); push(&v, e_del); push(&v, o_ins); push(&v, e_ins);
		for (j = 0; j < qlen; ++j) push(&v, q[j]);
		for (j = 0; j < tlen; ++j) push(&v, t[j]);
		/* ksw_extend2 (ksw.c:380) */
		sc = ksw_extend2(qlen, q, tlen, t, 5, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, &qle, &tle, &gtle, &gscore, &max_off);
		push(&v, sc); push(&v, qle); push(&v, tle); push(&v, gtle); push(&v, gscore); push(&v, max_off);
		rec_write(out, TAG_KSW_EXT, v.n, v.a);
		/* ksw_global2 (ksw.c:504) with CIGAR; band must admit the length difference */
		{
			int n_cigar = 0, wg = w > abs(tlen - qlen) + 3 ? w : abs(tlen - qlen) + 3;
			uint32_t *cigar = 0;
			v.n = 10 + qlen + tlen; v.a[2] = wg;
			sc = ksw_global2(qlen, q, tlen, t, 5, mat, o_del, e_del, o_ins, e_ins, wg, &n_cigar, &cigar);
			push(&v, sc); push(&v, n_cigar);
			for (j = 0; j < n_cigar; ++j) push(&v, cigar[j]);
			rec_write(out, TAG_KSW_GLB, v.n, v.a);
			free(cigar);
		}
		/* ksw_align2 (ksw.c:343) as mem_matesw calls it (bwamem_pair.c:166) */
		{
			kswr_t r;
			int xtra = KSW_XSUBO | KSW_XSTART | ((qlen * 1 < 250) ? KSW_XBYTE : 0) | (19 * 1);
			v.n = 10 + qlen + tlen;
			r = ksw_align2(qlen, q, tlen, t, 5, mat, o_del, e_del, o_ins, e_ins, xtra, 0);
			push(&v, r.score); push(&v, r.te); push(&v, r.qe); push(&v, r.score2); push(&v, r.te2);
			push(&v, r.tb); push(&v, r.qb);
			rec_write(out, TAG_KSW_ALN, v.n, v.a);
		}
		free(v.a); free(q); free(t);
	}
	fclose(out);
	return 0;
}

/* ksw_align2 (ksw.c:343) beyond the one call shape of katksw: word kernel as mem_seed_sw calls it (KSW_XSTART only,
 * bwamem.c:601), byte / word kernels with a sub-optimal threshold as mem_matesw does (bwamem_pair.c:165), under several
 * scoring matrices and gap costs.  Record: qlen tlen xtra o_del e_del o_ins e_ins mat[25] q[qlen] t[tlen] | 7 results. */
static int main_katalign(int argc, char **argv)
{
	static const int ab[4][2] = { {1, 4}, {2, 3}, {1, 1}, {3, 9} };
	static const int gaps[4][4] = { {6, 1, 6, 1}, {4, 2, 7, 1}, {1, 1, 1, 1}, {16, 1, 16, 1} };
	FILE *out;
	int i, n;
	if (argc < 4) return 1;
	out = fopen(argv[1], "wb");
	n = atoi(argv[2]); rng_state = strtoull(argv[3], 0, 10);
	for (i = 0; i < n; ++i) {
		const int *sc = ab[rng() % 4], *g = gaps[rng() % 4];
		int kind = rng() % 3, a = sc[0];
		int qlen = kind == 0 ? 1 + rng() % 199 : 1 + rng() % 400, tlen, err = rng() % 15, xtra, j;
		int8_t mat[25];
		uint8_t *q, *t;
		i64v v = {0, 0, 0};
		kswr_t r;
		if (kind == 0) { tlen = 1 + rng() % 199; xtra = KSW_XSTART; }                       /* mem_seed_sw */
		else {
			tlen = qlen + (int)(rng() % 500);
			xtra = KSW_XSUBO | KSW_XSTART | ((qlen * a < 250) ? KSW_XBYTE : 0) | (19 * a); /* mem_matesw */
			if (kind == 2 && (rng() & 1)) xtra &= ~KSW_XBYTE;                             /* word kernel on short queries too */
		}
		bwa_fill_scmat(a, sc[1], mat);
		q = malloc(qlen); t = malloc(tlen);
		if (kind == 0) rand_pair(qlen, tlen, err, q, t);
		else { /* the query sits somewhere inside a longer random target, mutated */
			int off = rng() % (tlen - qlen + 1);
			for (j = 0; j < tlen; ++j) t[j] = rng() & 3;
			rand_pair(qlen, qlen, err, q, t + off);
			if ((rng() & 3) == 0) for (j = 0; j < qlen && off + qlen + 40 + j < tlen; ++j) t[off + qlen + 40 + j] = q[j]; /* a second copy */
		}
		push(&v, qlen); push(&v, tlen); push(&v, xtra); push(&v, g[0]); push(&v, g[1]); push(&v, g[2]); push(&v, g[3]);
		for (j = 0; j < 25; ++j) push(&v, mat[j]);
		for (j = 0; j < qlen; ++j) push(&v, q[j]);
		for (j = 0; j < tlen; ++j) push(&v, t[j]);
		r = ksw_align2(qlen, q, tlen, t, 5, mat, g[0], g[1], g[2], g[3], xtra, 0);
		push(&v, r.score); push(&v, r.te); push(&v, r.qe); push(&v, r.score2); push(&v, r.te2); push(&v, r.tb); push(&v, r.qb);
		rec_write(out, TAG_KSW_ALN2, v.n, v.a);
		free(v.a); free(q); free(t);
	}
	fclose(out);
	return 0;
}

/* ksw_extend2 (ksw.c:380) and ksw_global2 (ksw.c:504) over the whole range the device forms are written for: flanks of 1 to 700
 * bases (half of the cases above 250, a quarter on the lengths where the device code changes form), bands from 0 to 400, h0 up
 * to 5000 (with the 50/60 matrix: scores beyond 16 bits), z-drop from 0 to 1000, five matrices, five sets of gap costs (one with a
 * free gap opening), 0 to 30 % errors, gaps of up to 40 bases, ambiguous bases.
 * Records: qlen tlen w h0 zdrop end_bonus o_del e_del o_ins e_ins mat[25] q[qlen] t[tlen] | 6 results (TAG_KSW_EXT_W)
 *          the same with w widened to admit the length difference, h0 = zdrop = end_bonus = 0 | score n_cigar cigar[] (TAG_KSW_GLB_W) */
enum { TAG_KSW_EXT_W = 24, TAG_KSW_GLB_W = 25 };

static void rand_pair_wide(int qlen, int tlen, int err_pct, int n_pct, uint8_t *q, uint8_t *t)
{ /* target = copy of the query with substitutions, short indels and now and then a gap of up to 40 bases */
	int i, j = 0;
	for (i = 0; i < qlen; ++i) q[i] = (int)(rng() % 100) < n_pct ? 4 : (rng() & 3);
	for (i = 0; i < tlen; ++i) {
		int r = rng() % 100;
		if (j >= qlen) { t[i] = rng() & 3; continue; }
		if (r < err_pct) {
			int kind = rng() % 8;
			if (kind < 4) t[i] = (q[j] + 1 + rng() % 3) & 3, ++j;             /* substitution */
			else if (kind < 6) t[i] = rng() & 3;                               /* base missing from the query */
			else if (kind < 7) { j += 1 + rng() % 3; t[i] = j < qlen ? q[j] : (rng() & 3); ++j; }
			else if ((rng() & 1) && tlen - i > 45) { int g = 1 + rng() % 40; while (g-- > 0 && i < tlen - 1) t[i++] = rng() & 3; t[i] = rng() & 3; } /* long gap in the query */
			else { j += 1 + rng() % 40; t[i] = j < qlen ? q[j] : (rng() & 3); ++j; }                                                    /* long gap in the target */
		} else t[i] = q[j++];
		if ((int)(rng() % 100) < n_pct) t[i] = 4;
	}
}

static int main_katdp(int argc, char **argv)
{
	static const int ab[5][2] = { {1, 4}, {2, 3}, {1, 1}, {3, 9}, {50, 60} };
	static const int gaps[5][4] = { {6, 1, 6, 1}, {4, 2, 7, 1}, {1, 1, 1, 1}, {16, 1, 16, 1}, {0, 1, 0, 1} };
	static const int ws[12] = { 0, 1, 2, 5, 20, 31, 32, 63, 64, 100, 127, 400 };
	static const int zds[5] = { 0, 1, 10, 100, 1000 }, ebs[3] = { 0, 5, 50 };
	static const int edge[12] = { 1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 700 };
	FILE *out;
	int i, n;
	if (argc < 4) return 1;
	out = fopen(argv[1], "wb");
	n = atoi(argv[2]); rng_state = strtoull(argv[3], 0, 10);
	for (i = 0; i < n; ++i) {
		const int *sc = ab[rng() % 5], *g = gaps[rng() % 5];
		int kind = rng() & 3;
		int qlen = kind < 2 ? 251 + rng() % 450 : kind == 2 ? 1 + rng() % 250 : edge[rng() % 12];
		int tlen = qlen - 40 + (int)(rng() % 121), err = (rng() & 3) ? rng() % 8 : rng() % 31, n_pct = (rng() & 7) == 0 ? 3 : 0;
		int w = ws[rng() % 12], h0 = (rng() & 1) ? 1 + rng() % 5000 : 1 + rng() % 120, zdrop = zds[rng() % 5], end_bonus = ebs[rng() % 3];
		int j, qle, tle, gtle, gscore, max_off, s, n_cigar = 0, wg;
		uint32_t *cigar = 0;
		int8_t mat[25];
		uint8_t *q, *t;
		i64v v = {0, 0, 0};
		if (tlen < 1) tlen = 1;
		if ((rng() & 31) == 0) n_pct = 100;                           /* nothing but ambiguous bases */
		bwa_fill_scmat(sc[0], sc[1], mat);
		q = malloc(qlen); t = malloc(tlen);
		rand_pair_wide(qlen, tlen, err, n_pct, q, t);
		push(&v, qlen); push(&v, tlen); push(&v, w); push(&v, h0); push(&v, zdrop); push(&v, end_bonus);
		push(&v, g[0]); push(&v, g[1]); push(&v, g[2]); push(&v, g[3]);
		for (j = 0; j < 25; ++j) push(&v, mat[j]);
		for (j = 0; j < qlen; ++j) push(&v, q[j]);
		for (j = 0; j < tlen; ++j) push(&v, t[j]);
		s = ksw_extend2(qlen, q, tlen, t, 5, mat, g[0], g[1], g[2], g[3], w, end_bonus, zdrop, h0, &qle, &tle, &gtle, &gscore, &max_off);
		push(&v, s); push(&v, qle); push(&v, tle); push(&v, gtle); push(&v, gscore); push(&v, max_off);
		rec_write(out, TAG_KSW_EXT_W, v.n, v.a);
		wg = w > abs(tlen - qlen) + 3 ? w : abs(tlen - qlen) + 3;    /* bwa.c:293-300: the band admits the length difference */
		v.n = 35 + qlen + tlen; v.a[2] = wg; v.a[3] = v.a[4] = v.a[5] = 0;
		s = ksw_global2(qlen, q, tlen, t, 5, mat, g[0], g[1], g[2], g[3], wg, &n_cigar, &cigar);
		push(&v, s); push(&v, n_cigar);
		for (j = 0; j < n_cigar; ++j) push(&v, cigar[j]);
		rec_write(out, TAG_KSW_GLB_W, v.n, v.a);
		free(cigar); free(v.a); free(q); free(t);
	}
	fclose(out);
	return 0;
}

/* katchain [options] <prefix> <cases.bin> <out.bin>: the reference's chaining on caller-supplied seeds -- its kbtree instantiation
 * (bwamem.c:194), test_and_merge, and mem_chain_flt (with mem_chain_weight inside), driven the way mem_chain drives them from bwamem.c:286
 * on.  cases.bin per read: TAG_READ [id, len], record 6 [(rbeg, qbeg, len, rid) per seed in look-up order; the rid given is ignored, the
 * reference's bns_intv2rid decides], TAG_INTV [(x[2], qbeg, qend) per interval, for frac_rep].  out.bin per read: TAG_READ, TAG_CHAIN
 * (w, kept, first as the tree holds them: not meaningful), TAG_CHAIN_FLT. */
static int main_katchain(int argc, char **argv)
{
	mem_opt_t *opt = mem_opt_init();
	bwaidx_t *idx;
	optparse_t op;
	FILE *in, *out;
	int64_t hdr[2], *rd[3] = { 0, 0, 0 }, rn[3] = { 0, 0, 0 };
	int c, k, rc = 0;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = bwa_idx_load(argv[optind], BWA_IDX_BNS);
	if (idx == 0) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->bns->n_seqs; ++c) idx->bns->anns[c].is_alt = 0;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out) return 1;
	while (fread(hdr, 8, 2, in) == 2) {
		static const int64_t want[3] = { TAG_READ, 6, TAG_INTV };
		kbtree_t(chn) *tree;
		mem_chain_v chain;
		int64_t t;
		int i, len, l_rep = 0, rb = 0, re = 0;
		for (k = 0; k < 3; ++k) {
			if (k && fread(hdr, 8, 2, in) != 2) { rc = 1; break; }
			if (hdr[0] != want[k] || hdr[1] < 0) { rc = 1; break; }
			rn[k] = hdr[1]; rd[k] = realloc(rd[k], (hdr[1] + 1) * 8);
			if (hdr[1] && fread(rd[k], 8, hdr[1], in) != (size_t)hdr[1]) { rc = 1; break; }
		}
		if (rc || rn[0] != 2 || rn[1] % 4 || rn[2] % 3) { rc = 1; break; }
		len = (int)rd[0][1];
		for (t = 0; t < rn[2]; t += 3) {                       /* query bases under over-abundant intervals (bwamem.c:272-279) */
			int qb = (int)rd[2][t + 1], qe = (int)rd[2][t + 2];
			if ((uint64_t)rd[2][t] <= (uint64_t)opt->max_occ) continue;
			if (qb > re) { l_rep += re - rb; rb = qb; re = qe; }
			else if (qe > re) re = qe;
		}
		l_rep += re - rb;
		tree = kb_init(chn, KB_DEFAULT_SIZE);
		for (t = 0; t < rn[1]; t += 4) {
			mem_chain_t key, *lower = 0, *upper = 0;
			mem_seed_t s;
			int rid, merged = 0;
			s.rbeg = key.pos = rd[1][t]; s.qbeg = (int)rd[1][t + 1]; s.score = s.len = (int)rd[1][t + 2];
			rid = bns_intv2rid(idx->bns, s.rbeg, s.rbeg + s.len);
			if (rid < 0) continue;
			if (kb_size(tree)) {
				kb_intervalp(chn, tree, &key, &lower, &upper);
				merged = lower && test_and_merge(opt, idx->bns->l_pac, lower, &s, rid);
			}
			if (!merged) {
				memset(&key, 0, sizeof key);                   /* the reference leaves w / kept / first as they are; the tests mask them */
				key.pos = s.rbeg; key.n = 1; key.m = 4;
				key.seeds = calloc(key.m, sizeof(mem_seed_t));
				key.seeds[0] = s;
				key.rid = rid; key.is_alt = !!idx->bns->anns[rid].is_alt;
				kb_putp(chn, tree, &key);
			}
		}
		kv_init(chain);
		kv_resize(mem_chain_t, chain, kb_size(tree) + 1);
#define katchain_take(p_) (chain.a[chain.n++] = *(p_))
		__kb_traverse(mem_chain_t, tree, katchain_take);
#undef katchain_take
		for (i = 0; i < chain.n; ++i) chain.a[i].frac_rep = (float)l_rep / len;
		kb_destroy(chn, tree);
		rec_write(out, TAG_READ, 2, rd[0]);
		dump_chains(out, TAG_CHAIN, chain.n, chain.a);
		chain.n = mem_chain_flt(opt, chain.n, chain.a);
		dump_chains(out, TAG_CHAIN_FLT, chain.n, chain.a);
		for (i = 0; i < chain.n; ++i) free(chain.a[i].seeds);
		free(chain.a);
	}
	for (k = 0; k < 3; ++k) free(rd[k]);
	fclose(in); fclose(out);
	bwa_idx_destroy(idx);
	free(opt);
	if (rc) fprintf(stderr, "[bwaref] katchain: malformed case file\n");
	return rc;
}

/* katmark [options] <prefix> <cases.bin> <out.bin>: the reference's own mem_mark_primary_se, mem_reorder_primary5 (under -5) and
 * mem_approx_mapq_se -- of every region: the function is defined for any region -- on caller-supplied region lists; kat_mark_io.h has both
 * file formats.  need, XA owner and the two counts are written as 0: the reference cannot give the selection without real alignments,
 * because mem_gen_alt and mem_reg2sam call mem_reg2aln as they go (a region here has no bases behind it).  The selection of the known
 * answers is ora_select, which the SAM goldens pin to the reference through ora_reg2sam / ora_gen_alt.  <prefix> is not read. */
static int main_katmark(int argc, char **argv)
{
	mem_opt_t *opt = mem_opt_init();
	optparse_t op;
	km_file_t k;
	FILE *in, *out;
	const int64_t *regs;
	int64_t i, *rec = 0;
	int c, n, rc, j, t;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || km_read_opt(in, opt, &k)) { fprintf(stderr, "[bwaref] katmark: cannot open the files, or no option record\n"); return 1; }
	while ((rc = km_next_read(in, &k, &i, &n, &regs)) > 0) {
		mem_alnreg_v v;
		int64_t hdr[2], id = km_read_id(&k, i);
		int n_pri;
		v.n = v.m = n; v.a = calloc(n ? n : 1, sizeof(mem_alnreg_t));
		for (j = 0; j < n; ++j) {
			const int64_t *w = regs + KM_REG_WORDS * j;
			mem_alnreg_t *p = &v.a[j];
			p->rb = w[0]; p->re = w[1]; p->qb = (int)w[2]; p->qe = (int)w[3]; p->rid = (int)w[4]; p->score = (int)w[5]; p->truesc = (int)w[6];
			p->sub = (int)w[7]; p->alt_sc = (int)w[8]; p->csub = (int)w[9]; p->sub_n = (int)w[10]; p->w = (int)w[11]; p->seedcov = (int)w[12];
			p->secondary = (int)w[13]; p->secondary_all = (int)w[14]; p->seedlen0 = (int)w[15]; p->n_comp = (int)w[16]; p->is_alt = (int)w[17];
			p->frac_rep = km_i2f(w[18]);
		}
		n_pri = mem_mark_primary_se(opt, n, v.a, id);
		if (opt->flag & MEM_F_PRIMARY5) mem_reorder_primary5(opt->T, &v);
		rec = realloc(rec, (4 + (size_t)KM_OUT_WORDS * n) * 8);
		rec[0] = n; rec[1] = n_pri; rec[2] = rec[3] = 0;
		for (j = 0; j < n; ++j) {
			const mem_alnreg_t *p = &v.a[j];
			int64_t *w = rec + 4 + KM_OUT_WORDS * j;
			w[0] = p->rb; w[1] = p->re; w[2] = p->qb; w[3] = p->qe; w[4] = p->rid; w[5] = p->score; w[6] = p->truesc; w[7] = p->sub; w[8] = p->alt_sc;
			w[9] = p->csub; w[10] = p->sub_n; w[11] = p->w; w[12] = p->seedcov; w[13] = p->secondary; w[14] = p->secondary_all; w[15] = p->seedlen0;
			w[16] = p->n_comp; w[17] = p->is_alt; w[18] = f2i(p->frac_rep); w[19] = (int64_t)p->hash;
			for (t = 0; t < n && hash_64((uint64_t)id + t) != p->hash; ++t);
			w[20] = t < n ? t : -1;
			w[21] = w[22] = 0; w[23] = mem_approx_mapq_se(opt, p); w[24] = 0;
		}
		hdr[0] = i; hdr[1] = n;
		rec_write(out, TAG_READ, 2, hdr);
		rec_write(out, KM_TAG_MARK, 4 + (int64_t)KM_OUT_WORDS * n, rec);
		free(v.a);
	}
	free(rec); free(k.buf);
	fclose(in); fclose(out);
	free(opt);
	if (rc) fprintf(stderr, "[bwaref] katmark: malformed case file\n");
	return rc ? 1 : 0;
}

/* katdedup [options] <prefix> <cases.bin> <out.bin>: the reference's own mem_sort_dedup_patch(opt, bns, pac, query, n, a) and the is_alt
 * loop of mem_align1_core (bwamem.c:1091-1095) on caller-supplied region lists over the index's reference; kat_dedup_io.h has both file
 * formats.  The words of what the function did are written as 0: the reference does not count. */
static int main_katdedup(int argc, char **argv)
{
	mem_opt_t *opt = mem_opt_init();
	optparse_t op;
	bwaidx_t *idx;
	kd_file_t k;
	FILE *in, *out;
	const int64_t *regs;
	uint8_t *seq;
	int64_t i, *rec = 0;
	int c, n, l, rc, j;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = bwa_idx_load(argv[optind], BWA_IDX_BNS | BWA_IDX_PAC);
	if (!idx) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->bns->n_seqs; ++c) idx->bns->anns[c].is_alt = 0;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || kd_read_opt(in, opt, &k)) { fprintf(stderr, "[bwaref] katdedup: cannot open the files, or no option record\n"); return 1; }
	while ((rc = kd_next_read(in, &k, &i, &l, &seq, &n, &regs)) > 0) {
		mem_alnreg_t *a = calloc(n, sizeof(mem_alnreg_t));
		int64_t hdr[2];
		(void)l;
		for (j = 0; j < n; ++j) {
			const int64_t *w = regs + KD_REG_WORDS * j;
			mem_alnreg_t *p = &a[j];
			p->rb = w[0]; p->re = w[1]; p->qb = (int)w[2]; p->qe = (int)w[3]; p->rid = (int)w[4]; p->score = (int)w[5]; p->truesc = (int)w[6];
			p->sub = (int)w[7]; p->alt_sc = (int)w[8]; p->csub = (int)w[9]; p->sub_n = (int)w[10]; p->w = (int)w[11]; p->seedcov = (int)w[12];
			p->secondary = (int)w[13]; p->secondary_all = (int)w[14]; p->seedlen0 = (int)w[15]; p->n_comp = (int)w[16]; p->is_alt = (int)w[17];
			p->frac_rep = km_i2f(w[18]);
		}
		n = mem_sort_dedup_patch(opt, idx->bns, idx->pac, seq, n, a);
		rec = realloc(rec, (1 + KD_STAT_WORDS + (size_t)KD_REG_WORDS * n) * 8);
		memset(rec, 0, (1 + KD_STAT_WORDS) * 8);
		rec[0] = n;
		for (j = 0; j < n; ++j) {
			mem_alnreg_t *p = &a[j];
			int64_t *w = rec + 1 + KD_STAT_WORDS + KD_REG_WORDS * j;
			if (p->rid >= 0 && idx->bns->anns[p->rid].is_alt) p->is_alt = 1;
			w[0] = p->rb; w[1] = p->re; w[2] = p->qb; w[3] = p->qe; w[4] = p->rid; w[5] = p->score; w[6] = p->truesc; w[7] = p->sub; w[8] = p->alt_sc;
			w[9] = p->csub; w[10] = p->sub_n; w[11] = p->w; w[12] = p->seedcov; w[13] = p->secondary; w[14] = p->secondary_all; w[15] = p->seedlen0;
			w[16] = p->n_comp; w[17] = p->is_alt; w[18] = f2i(p->frac_rep);
		}
		hdr[0] = i; hdr[1] = n;
		rec_write(out, TAG_READ, 2, hdr);
		rec_write(out, KD_TAG_OUT, 1 + KD_STAT_WORDS + (int64_t)KD_REG_WORDS * n, rec);
		free(a);
	}
	free(rec); free(k.buf); free(k.seq);
	fclose(in); fclose(out);
	bwa_idx_destroy(idx);
	free(opt);
	if (rc) fprintf(stderr, "[bwaref] katdedup: malformed case file\n");
	return rc ? 1 : 0;
}

/* katpair [options] <prefix> <cases.bin> <out.bin>: per pair of caller-supplied region lists the reference's own mem_mark_primary_se of
 * both ends (and mem_reorder_primary5 under -5), then -- where mem_sam_pe would call it: pairing not switched off, a primary-assembly hit
 * on both ends -- its exported mem_pair over the contig table of the index, z[] set to -1 beforehand; kat_pair_io.h has both file formats.
 * mem_sam_pe's own decisions cannot be called without aligning and printing: for those the oracle is the judge. */
static int main_katpair(int argc, char **argv)
{
	extern int mem_pair(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], bseq1_t s[2], mem_alnreg_v a[2], int id, int *sub, int *n_sub, int z[2], int n_pri[2]);
	mem_opt_t *opt = mem_opt_init();
	optparse_t op;
	bwaidx_t *idx;
	kp_file_t k;
	FILE *in, *out;
	const int64_t *regs[2];
	int64_t i[2], *rec = 0;
	int c, n[2], rc, e, j;
	bwa_verbose = 1;
	optparse_init(&op, opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = bwa_idx_load(argv[optind], BWA_IDX_BNS);
	if (!idx) return 1;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || kp_read_opt(in, opt, &k)) { fprintf(stderr, "[bwaref] katpair: cannot open the files, or no option record\n"); return 1; }
	while ((rc = kp_next_pair(in, &k, i, n, regs)) > 0) {
		mem_alnreg_v a[2];
		bseq1_t s[2];
		const int64_t id = (k.n_processed >> 1) + (i[0] >> 1);
		int n_pri[2], z[2] = { -1, -1 }, ret = 0, sub = 0, n_sub = 0;
		int64_t pair5[5];
		memset(s, 0, sizeof s);
		for (e = 0; e < 2; ++e) {
			a[e].n = a[e].m = n[e]; a[e].a = calloc(n[e] ? n[e] : 1, sizeof(mem_alnreg_t));
			for (j = 0; j < n[e]; ++j) {
				const int64_t *w = regs[e] + KM_REG_WORDS * j;
				mem_alnreg_t *p = &a[e].a[j];
				if (w[4] < 0 || w[4] >= idx->bns->n_seqs) rc = -1;
				p->rb = w[0]; p->re = w[1]; p->qb = (int)w[2]; p->qe = (int)w[3]; p->rid = (int)w[4]; p->score = (int)w[5]; p->truesc = (int)w[6];
				p->sub = (int)w[7]; p->alt_sc = (int)w[8]; p->csub = (int)w[9]; p->sub_n = (int)w[10]; p->w = (int)w[11]; p->seedcov = (int)w[12];
				p->secondary = (int)w[13]; p->secondary_all = (int)w[14]; p->seedlen0 = (int)w[15]; p->n_comp = (int)w[16]; p->is_alt = (int)w[17];
				p->frac_rep = km_i2f(w[18]);
			}
		}
		if (rc < 0) break;
		for (e = 0; e < 2; ++e) n_pri[e] = mem_mark_primary_se(opt, n[e], a[e].a, id << 1 | e);
		if (opt->flag & MEM_F_PRIMARY5) { mem_reorder_primary5(opt->T, &a[0]); mem_reorder_primary5(opt->T, &a[1]); }
		for (e = 0; e < 2; ++e) {
			int64_t hdr[2];
			rec = realloc(rec, (2 + (size_t)KM_REG_WORDS * n[e]) * 8);
			rec[0] = n[e]; rec[1] = n_pri[e];
			for (j = 0; j < n[e]; ++j) {
				const mem_alnreg_t *p = &a[e].a[j];
				int64_t *w = rec + 2 + KM_REG_WORDS * j;
				w[0] = p->rb; w[1] = p->re; w[2] = p->qb; w[3] = p->qe; w[4] = p->rid; w[5] = p->score; w[6] = p->truesc; w[7] = p->sub; w[8] = p->alt_sc;
				w[9] = p->csub; w[10] = p->sub_n; w[11] = p->w; w[12] = p->seedcov; w[13] = p->secondary; w[14] = p->secondary_all; w[15] = p->seedlen0;
				w[16] = p->n_comp; w[17] = p->is_alt; w[18] = f2i(p->frac_rep);
			}
			hdr[0] = i[e]; hdr[1] = n[e];
			rec_write(out, TAG_READ, 2, hdr);
			rec_write(out, KP_TAG_MARKED, 2 + (int64_t)KM_REG_WORDS * n[e], rec);
			if (e == 0) {
				if (!(opt->flag & MEM_F_NOPAIRING) && n_pri[0] && n_pri[1])
					ret = mem_pair(opt, idx->bns, 0, k.pes, s, a, (int)id, &sub, &n_sub, z, n_pri);
				pair5[0] = ret; pair5[1] = sub; pair5[2] = n_sub; pair5[3] = z[0]; pair5[4] = z[1];
				rec_write(out, KP_TAG_MEMPAIR, 5, pair5);
			}
		}
		free(a[0].a); free(a[1].a);
	}
	free(rec); kp_free(&k);
	fclose(in); fclose(out);
	bwa_idx_destroy(idx);
	free(opt);
	if (rc) fprintf(stderr, "[bwaref] katpair: malformed case file\n");
	return rc ? 1 : 0;
}

/* readfq <chunk_bases> <in1> [in2]: the batches the reference's bseq_read (bwa.c:191) cuts, one record per line as
 * name TAB comment-or-* TAB seq TAB qual-or-*, a line "#batch <n>" in front of every batch -- golden vectors for the product's
 * FASTA/FASTQ reader (csrc/fastq_reader.cpp) */
static int main_readfq(int argc, char **argv)
{
	gzFile f1, f2 = 0;
	kseq_t *ks, *ks2 = 0;
	bseq1_t *seqs;
	int n, i, chunk;
	if (argc < 3) return 1;
	chunk = atoi(argv[1]);
	f1 = gzopen(argv[2], "r"); ks = kseq_init(f1);
	if (argc > 3) { f2 = gzopen(argv[3], "r"); ks2 = kseq_init(f2); }
	while ((seqs = bseq_read(chunk, &n, ks, ks2)) != 0) {
		printf("#batch %d\n", n);
		for (i = 0; i < n; ++i) {
			printf("%s\t%s\t%s\t%s\n", seqs[i].name, seqs[i].comment ? seqs[i].comment : "*", seqs[i].seq, seqs[i].qual ? seqs[i].qual : "*");
			free(seqs[i].name); free(seqs[i].comment); free(seqs[i].seq); free(seqs[i].qual);
		}
		free(seqs);
		if (n == 0) break;
	}
	kseq_destroy(ks); gzclose(f1);
	if (ks2) { kseq_destroy(ks2); gzclose(f2); }
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: bwaref <index|mem|stages|katfm|katksw> ...\n");
		return 1;
	}
	if (strcmp(argv[1], "index") == 0) return main_index(argc - 1, argv + 1);
	if (strcmp(argv[1], "mem") == 0) return main_mem(argc - 1, argv + 1);
	if (strcmp(argv[1], "stages") == 0) return main_stages(argc - 1, argv + 1);
	if (strcmp(argv[1], "katfm") == 0) return main_katfm(argc - 1, argv + 1);
	if (strcmp(argv[1], "katksw") == 0) return main_katksw(argc - 1, argv + 1);
	if (strcmp(argv[1], "katalign") == 0) return main_katalign(argc - 1, argv + 1);
	if (strcmp(argv[1], "katdp") == 0) return main_katdp(argc - 1, argv + 1);
	if (strcmp(argv[1], "katchain") == 0) return main_katchain(argc - 1, argv + 1);
	if (strcmp(argv[1], "katmark") == 0) return main_katmark(argc - 1, argv + 1);
	if (strcmp(argv[1], "katdedup") == 0) return main_katdedup(argc - 1, argv + 1);
	if (strcmp(argv[1], "katpair") == 0) return main_katpair(argc - 1, argv + 1);
	if (strcmp(argv[1], "readfq") == 0) return main_readfq(argc - 1, argv + 1);
	fprintf(stderr, "unknown sub-command '%s'\n", argv[1]);
	return 1;
}
