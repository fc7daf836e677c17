/* ORACLE (test infrastructure only) -- command-line front end of the C
 * restatement.  Mirrors oracle/ref_driver.c so tests can diff the two:
 *   bwa_oracle mem    [-p] [-t N] [-K bases] [-a] <prefix> <r1.fq> [r2.fq]   SAM body on stdout
 *   bwa_oracle stages <prefix> <reads.fq> <out.bin>                          per-read stage dump
 *   bwa_oracle stages [options, -I] <prefix> <r1.fq> <r2.fq> <out.bin>       paired-end stage dump (one batch)
 *   bwa_oracle katchain [options] <prefix> <cases.bin> <out.bin>             chains of caller-supplied seed lists
 *   bwa_oracle katdedup [options] <prefix> <cases.bin> <out.bin>             mem_sort_dedup_patch and the is_alt marking of caller-supplied region lists
 *   bwa_oracle katmark [options] <prefix> <cases.bin> <out.bin>              primary marking, selection and mapQ of caller-supplied region lists
 *   bwa_oracle katpair [options] <prefix> <cases.bin> <out.bin>              mem_pair and mem_sam_pe's decisions on caller-supplied pairs of region lists
 * Batching follows bseq_read (bwa.c:191): reads are taken until the batch holds
 * >= chunk bases and an even number of reads.
 */
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <ctype.h>
#include <zlib.h>
#include <sys/time.h>
static double now_s(void) { struct timeval tv; gettimeofday(&tv, 0); return tv.tv_sec + tv.tv_usec * 1e-6; }
#include <math.h>
#include "ora.h"
#define OPT_T ora_opt_t
#define PES_T ora_pestat_t
#define OPT_FILL_SCMAT(a, b, mat) ora_fill_scmat((a), (b), (mat))
#define OPT_LOG(x) log(x)
#include "opt_parse.h"
#include "kat_mark_io.h"
#include "kat_dedup_io.h"
#include "kat_pair_io.h"

/* ---- minimal FASTA/FASTQ reader with kseq.h's field semantics ---- */
typedef struct { gzFile fp; char *line; size_t m; int peeked; } fq_t;
static int fq_getline(fq_t *f)
{
	size_t l = 0;
	if (f->peeked) { f->peeked = 0; return 1; }
	for (;;) {
		if (l + 4096 > f->m) { f->m = f->m ? f->m << 1 : 8192; f->line = (char*)realloc(f->line, f->m); }
		if (!gzgets(f->fp, f->line + l, (int)(f->m - l))) { if (l == 0) return 0; break; }
		l += strlen(f->line + l);
		if (l && f->line[l-1] == '\n') break;
	}
	while (l && (f->line[l-1] == '\n' || f->line[l-1] == '\r')) f->line[--l] = 0;
	return 1;
}
static int fq_read(fq_t *f, ora_read_t *r)
{
	char *p, *q;
	size_t l_seq = 0, m_seq = 0;
	memset(r, 0, sizeof *r);
	do { if (!fq_getline(f)) return 0; } while (f->line[0] != '>' && f->line[0] != '@');
	p = f->line + 1;
	for (q = p; *q && !isspace((unsigned char)*q); ++q);
	r->name = strndup(p, q - p);
	while (*q && isspace((unsigned char)*q)) ++q;
	if (*q) r->comment = strdup(q);
	while (fq_getline(f)) {
		size_t l;
		if (f->line[0] == '+' || f->line[0] == '>' || f->line[0] == '@') { if (f->line[0] != '+') f->peeked = 1; break; }
		l = strlen(f->line);
		if (l_seq + l + 1 > m_seq) { m_seq = (l_seq + l + 1) * 2; r->seq = (char*)realloc(r->seq, m_seq); }
		memcpy(r->seq + l_seq, f->line, l); l_seq += l;
	}
	if (!r->seq) r->seq = (char*)calloc(1, 1);
	r->seq[l_seq] = 0; r->l_seq = (int)l_seq;
	if (!f->peeked && f->line && f->line[0] == '+') {       /* quality: as many characters as bases */
		size_t l_q = 0;
		r->qual = (char*)malloc(l_seq + 1);
		while (l_q < l_seq && fq_getline(f)) {
			size_t l = strlen(f->line);
			if (l_q + l > l_seq) l = l_seq - l_q;
			memcpy(r->qual + l_q, f->line, l); l_q += l;
		}
		r->qual[l_q] = 0;
	}
	{ size_t l = strlen(r->name);                           /* bwa.c:73 trim_readno */
	  if (l > 2 && r->name[l-2] == '/' && isdigit((unsigned char)r->name[l-1])) r->name[l-2] = 0; }
	return 1;
}

static ora_read_t *read_batch(int chunk, int *n_, fq_t *f1, fq_t *f2)   /* bwa.c:191 bseq_read */
{
	int size = 0, m = 0, n = 0;
	ora_read_t *seqs = 0, r;
	while (fq_read(f1, &r)) {
		ora_read_t r2;
		if (f2 && !fq_read(f2, &r2)) break;
		if (n + 2 > m) { m = m ? m << 1 : 256; seqs = (ora_read_t*)realloc(seqs, m * sizeof(ora_read_t)); }
		r.id = n; seqs[n++] = r; size += r.l_seq;
		if (f2) { r2.id = n; seqs[n++] = r2; size += r2.l_seq; }
		if (size >= chunk && (n & 1) == 0) break;
	}
	*n_ = n;
	return seqs;
}

/* ---- record dump, same layout as ref_driver.c ---- */
static void rec_write(FILE *fp, int64_t tag, int64_t n, const int64_t *v) { fwrite(&tag, 8, 1, fp); fwrite(&n, 8, 1, fp); if (n) fwrite(v, 8, n, fp); }
typedef struct { int64_t n, m; int64_t *a; } i64v;
static inline void push(i64v *v, int64_t x) { if (v->n == v->m) { v->m = v->m ? v->m << 1 : 256; v->a = (int64_t*)realloc(v->a, v->m * 8); } v->a[v->n++] = x; }
static inline int64_t f2i(float f) { uint32_t u; memcpy(&u, &f, 4); return (int64_t)u; }
enum { TAG_READ = 100, TAG_INTV = 1, TAG_CHAIN = 2, TAG_CHAIN_FLT = 3, TAG_REGS_PRE = 5, TAG_REGS = 4, TAG_PESTAT = 7, TAG_REGS_PE = 8, TAG_PAIR = 9 };

static void dump_chains(FILE *fp, int64_t tag, int n, const ora_chain_t *a)
{
	i64v v = { 0, 0, 0 };
	int i, j;
	push(&v, n);
	for (i = 0; i < n; ++i) {
		const ora_chain_t *c = &a[i];
		push(&v, c->pos); push(&v, c->rid); push(&v, c->is_alt); push(&v, c->w); push(&v, c->kept);
		push(&v, c->first); push(&v, f2i(c->frac_rep)); push(&v, c->n);
		for (j = 0; j < c->n; ++j) { push(&v, c->seeds[j].rbeg); push(&v, c->seeds[j].qbeg); push(&v, c->seeds[j].len); push(&v, c->seeds[j].score); }
	}
	rec_write(fp, tag, v.n, v.a); free(v.a);
}
static void dump_regs(FILE *fp, int64_t tag, int n, const ora_reg_t *a)
{
	i64v v = { 0, 0, 0 };
	int i;
	push(&v, n);
	for (i = 0; i < n; ++i) {
		const ora_reg_t *p = &a[i];
		push(&v, p->rb); push(&v, p->re); push(&v, p->qb); push(&v, p->qe); push(&v, p->rid);
		push(&v, p->score); push(&v, p->truesc); push(&v, p->sub); push(&v, p->alt_sc); push(&v, p->csub);
		push(&v, p->sub_n); push(&v, p->w); push(&v, p->seedcov); push(&v, p->secondary);
		push(&v, p->secondary_all); push(&v, p->seedlen0); push(&v, p->n_comp); push(&v, p->is_alt);
		push(&v, f2i(p->frac_rep));
	}
	rec_write(fp, tag, v.n, v.a); free(v.a);
}

/* Paired-end stages: the whole input as ONE batch through ora_process_seqs with the recording hook of ora.h switched on.
 * PESTAT once, in front of the reads (per direction low, high, failed and the bit patterns of avg and std); per read REGS (the
 * list mem_sam_pe is given), REGS_PE (after all mem_matesw calls, bwamem_pair.c:299) and PAIR (see ora_pe_dump_t). */
static int stages_pe(ora_opt_t *opt, const optparse_t *op, ora_index_t *idx, const char *fq1, const char *fq2, const char *out_fn)
{
	fq_t f1 = { 0, 0, 0, 0 }, f2 = { 0, 0, 0, 0 };
	ora_pe_dump_t rec;
	ora_read_t *seqs;
	FILE *out;
	int64_t ps[20];
	int n, i, d;
	f1.fp = gzopen(fq1, "r"); f2.fp = gzopen(fq2, "r");
	if (!f1.fp || !f2.fp || !(out = fopen(out_fn, "wb"))) return 1;
	opt->flag |= ORA_F_PE;
	seqs = read_batch(0x7fffffff, &n, &f1, &f2);
	memset(&rec, 0, sizeof rec);
	rec.se = (ora_reg_v*)calloc(n ? n : 1, sizeof(ora_reg_v)); rec.pe = (ora_reg_v*)calloc(n ? n : 1, sizeof(ora_reg_v));
	rec.pair = (int64_t(*)[8])calloc(n ? n : 1, sizeof(int64_t[8]));
	ora_pe_dump = &rec;
	ora_process_seqs(opt, idx, 0, n, seqs, op->has_pes0 ? op->pes : 0);
	ora_pe_dump = 0;
	for (d = 0; d < 4; ++d) {
		ps[5*d] = rec.pes[d].low; ps[5*d+1] = rec.pes[d].high; ps[5*d+2] = rec.pes[d].failed;
		memcpy(&ps[5*d+3], &rec.pes[d].avg, 8); memcpy(&ps[5*d+4], &rec.pes[d].std, 8);
	}
	rec_write(out, TAG_PESTAT, 20, ps);
	for (i = 0; i < n; ++i) {
		int64_t hdr[2];
		hdr[0] = i; hdr[1] = seqs[i].l_seq;
		rec_write(out, TAG_READ, 2, hdr);
		dump_regs(out, TAG_REGS, rec.se[i].n, rec.se[i].a);
		dump_regs(out, TAG_REGS_PE, rec.pe[i].n, rec.pe[i].a);
		rec_write(out, TAG_PAIR, 8, rec.pair[i]);
		free(rec.se[i].a); free(rec.pe[i].a);
		free(seqs[i].name); free(seqs[i].comment); free(seqs[i].seq); free(seqs[i].qual); free(seqs[i].sam);
	}
	free(seqs); free(rec.se); free(rec.pe); free(rec.pair);
	fclose(out); gzclose(f1.fp); gzclose(f2.fp); free(f1.line); free(f2.line);
	return 0;
}

static int main_stages(int argc, char **argv)
{
	ora_opt_t opt;
	ora_index_t *idx;
	fq_t f = { 0, 0, 0, 0 };
	FILE *out;
	ora_read_t r;
	int64_t id = 0;
	optparse_t op;
	int c;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	argv += optind - 1;
	idx = ora_index_load(argv[1]);
	if (op.ignore_alt) for (c = 0; c < idx->ref->n_seqs; ++c) idx->ref->anns[c].is_alt = 0;
	if (optind + 4 <= argc) { c = stages_pe(&opt, &op, idx, argv[2], argv[3], argv[4]); ora_index_destroy(idx); return c; }
	f.fp = gzopen(argv[2], "r");
	out = fopen(argv[3], "wb");
	while (fq_read(&f, &r)) {
		int i, l_seq = r.l_seq;
		char *seq = r.seq;
		ora_aux_t *aux = ora_aux_new();
		ora_chain_v chn;
		ora_reg_v regs = { 0, 0, 0 };
		int64_t hdr[2];
		i64v v = { 0, 0, 0 };
		for (i = 0; i < l_seq; ++i) seq[i] = seq[i] < 4 ? seq[i] : ora_nt4_table[(uint8_t)seq[i]];
		hdr[0] = id++; hdr[1] = l_seq;
		rec_write(out, TAG_READ, 2, hdr);
		if (l_seq >= opt.min_seed_len) {
			ora_collect_intv(&opt, idx->fmi, l_seq, (uint8_t*)seq, aux);
			for (i = 0; i < aux->mem.n; ++i) { push(&v, aux->mem.a[i].x[0]); push(&v, aux->mem.a[i].x[1]); push(&v, aux->mem.a[i].x[2]); push(&v, aux->mem.a[i].info); }
		}
		rec_write(out, TAG_INTV, v.n, v.a); free(v.a);
		chn = ora_chain(&opt, idx, l_seq, (uint8_t*)seq, aux);
		dump_chains(out, TAG_CHAIN, chn.n, chn.a);
		chn.n = ora_chain_flt(&opt, chn.n, chn.a);
		ora_flt_chained_seeds(&opt, idx->ref, l_seq, (uint8_t*)seq, chn.n, chn.a);
		dump_chains(out, TAG_CHAIN_FLT, chn.n, chn.a);
		for (i = 0; i < chn.n; ++i) { ora_chain2aln(&opt, idx->ref, l_seq, (uint8_t*)seq, &chn.a[i], &regs); free(chn.a[i].seeds); }
		free(chn.a);
		dump_regs(out, TAG_REGS_PRE, regs.n, regs.a);
		regs.n = ora_sort_dedup_patch(&opt, idx->ref, (uint8_t*)seq, regs.n, regs.a);
		for (i = 0; i < regs.n; ++i)
			if (regs.a[i].rid >= 0 && idx->ref->anns[regs.a[i].rid].is_alt) regs.a[i].is_alt = 1;
		dump_regs(out, TAG_REGS, regs.n, regs.a);
		free(regs.a); ora_aux_free(aux);
		free(r.name); free(r.comment); free(r.seq); free(r.qual);
	}
	fclose(out); gzclose(f.fp);
	ora_index_destroy(idx);
	return 0;
}

/* katchain [options] <prefix> <cases.bin> <out.bin>: ora_kat_chain on caller seeds.  cases.bin, per read: TAG_READ [id, len], record 6
 * [(rbeg, qbeg, len, rid) per seed, look-up order], TAG_INTV [(x[2], qbeg, qend) per interval].  out.bin, per read: TAG_READ, TAG_CHAIN,
 * TAG_CHAIN_FLT as `stages` writes them, and TAG_CHAIN_STAT [B-tree nodes, tree height, chains sorted, depth limit reached] (ours only:
 * ref_driver.c's katchain stops at TAG_CHAIN_FLT). */
enum { TAG_SEEDS = 6, TAG_CHAIN_STAT = 30 };
static int main_katchain(int argc, char **argv)
{
	ora_opt_t opt;
	ora_index_t *idx;
	optparse_t op;
	FILE *in, *out;
	int64_t hdr[2], *rd[3] = { 0, 0, 0 }, rn[3] = { 0, 0, 0 };
	int c, k, rc = 0;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = ora_index_load(argv[optind]);
	if (!idx) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->ref->n_seqs; ++c) idx->ref->anns[c].is_alt = 0;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out) return 1;
	while (fread(hdr, 8, 2, in) == 2) {
		static const int64_t want[3] = { TAG_READ, TAG_SEEDS, TAG_INTV };
		ora_chain_v un, flt;
		int stat[4], i;
		int64_t st[4];
		for (k = 0; k < 3; ++k) {                              /* the three records of a read, in this order */
			if (k && fread(hdr, 8, 2, in) != 2) { rc = 1; break; }
			if (hdr[0] != want[k] || hdr[1] < 0) { rc = 1; break; }
			rn[k] = hdr[1]; rd[k] = (int64_t*)realloc(rd[k], (hdr[1] + 1) * 8);
			if (hdr[1] && fread(rd[k], 8, hdr[1], in) != (size_t)hdr[1]) { rc = 1; break; }
		}
		if (rc || rn[0] != 2 || rn[1] % 4 || rn[2] % 3) { rc = 1; break; }
		ora_kat_chain(&opt, idx, (int)rd[0][1], (int)(rn[1] / 4), rd[1], (int)(rn[2] / 3), rd[2], &un, &flt, stat);
		rec_write(out, TAG_READ, 2, rd[0]);
		dump_chains(out, TAG_CHAIN, un.n, un.a);
		dump_chains(out, TAG_CHAIN_FLT, flt.n, flt.a);
		for (i = 0; i < 4; ++i) st[i] = stat[i];
		rec_write(out, TAG_CHAIN_STAT, 4, st);
		for (i = 0; i < un.n; ++i) free(un.a[i].seeds);
		for (i = 0; i < flt.n; ++i) free(flt.a[i].seeds);
		free(un.a); free(flt.a);
	}
	for (k = 0; k < 3; ++k) free(rd[k]);
	fclose(in); fclose(out);
	ora_index_destroy(idx);
	if (rc) fprintf(stderr, "[bwa_oracle] katchain: malformed case file\n");
	return rc;
}

/* katmark [options] <prefix> <cases.bin> <out.bin>: ora_kat_mark on caller region lists (kat_mark_io.h has both file formats).  The index
 * is not read: <prefix> is there so that the command line is the one of the other sub-commands. */
static int main_katmark(int argc, char **argv)
{
	ora_opt_t opt;
	optparse_t op;
	km_file_t k;
	FILE *in, *out;
	const int64_t *regs;
	int64_t i, *rec = 0;
	int c, n, rc;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || km_read_opt(in, &opt, &k)) { fprintf(stderr, "[bwa_oracle] katmark: cannot open the files, or no option record\n"); return 1; }
	while ((rc = km_next_read(in, &k, &i, &n, &regs)) > 0) {
		int64_t hdr[2];
		rec = (int64_t*)realloc(rec, (4 + (size_t)KM_OUT_WORDS * n) * 8);
		ora_kat_mark(&opt, n, regs, km_read_id(&k, i), rec);
		hdr[0] = i; hdr[1] = n;
		rec_write(out, TAG_READ, 2, hdr);
		rec_write(out, KM_TAG_MARK, 4 + (int64_t)KM_OUT_WORDS * n, rec);
	}
	free(rec); free(k.buf);
	fclose(in); fclose(out);
	if (rc) fprintf(stderr, "[bwa_oracle] katmark: malformed case file\n");
	return rc ? 1 : 0;
}

/* katdedup [options] <prefix> <cases.bin> <out.bin>: ora_kat_dedup on caller region lists over the index's reference (kat_dedup_io.h has
 * both file formats). */
static int main_katdedup(int argc, char **argv)
{
	ora_opt_t opt;
	ora_index_t *idx;
	optparse_t op;
	kd_file_t k;
	FILE *in, *out;
	const int64_t *regs;
	uint8_t *seq;
	int64_t i, *rec = 0;
	int c, n, l, m, rc;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = ora_index_load(argv[optind]);
	if (!idx) return 1;
	if (op.ignore_alt) for (c = 0; c < idx->ref->n_seqs; ++c) idx->ref->anns[c].is_alt = 0;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || kd_read_opt(in, &opt, &k)) { fprintf(stderr, "[bwa_oracle] katdedup: cannot open the files, or no option record\n"); return 1; }
	while ((rc = kd_next_read(in, &k, &i, &l, &seq, &n, &regs)) > 0) {
		int64_t hdr[2];
		rec = (int64_t*)realloc(rec, (1 + KD_STAT_WORDS + (size_t)KD_REG_WORDS * n) * 8);
		m = ora_kat_dedup(&opt, idx->ref, l, seq, n, regs, rec + 1 + KD_STAT_WORDS, rec + 1);
		rec[0] = m;
		hdr[0] = i; hdr[1] = m;
		rec_write(out, TAG_READ, 2, hdr);
		rec_write(out, KD_TAG_OUT, 1 + KD_STAT_WORDS + (int64_t)KD_REG_WORDS * m, rec);
	}
	free(rec); free(k.buf); free(k.seq);
	fclose(in); fclose(out);
	ora_index_destroy(idx);
	if (rc) fprintf(stderr, "[bwa_oracle] katdedup: malformed case file\n");
	return rc ? 1 : 0;
}

/* katpair [options] <prefix> <cases.bin> <out.bin>: ora_kat_pair on caller pairs of region lists over the contig table of the index
 * (kat_pair_io.h has both file formats). */
static int main_katpair(int argc, char **argv)
{
	ora_opt_t opt;
	ora_index_t *idx;
	optparse_t op;
	kp_file_t k;
	FILE *in, *out;
	const int64_t *regs[2];
	int64_t i[2], *marked[2] = { 0, 0 }, *rec[2] = { 0, 0 }, pair5[5], extra[ORA_KAT_PAIR_EXTRA];
	int c, n[2], rc, e;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 3 > argc) return 1;
	idx = ora_index_load(argv[optind]);
	if (!idx) return 1;
	in = fopen(argv[optind + 1], "rb"); out = fopen(argv[optind + 2], "wb");
	if (!in || !out || kp_read_opt(in, &opt, &k)) { fprintf(stderr, "[bwa_oracle] katpair: cannot open the files, or no option record\n"); return 1; }
	while ((rc = kp_next_pair(in, &k, i, n, regs)) > 0) {
		for (e = 0; e < 2; ++e) {
			int j;
			marked[e] = (int64_t*)realloc(marked[e], (2 + (size_t)KM_REG_WORDS * n[e]) * 8);
			rec[e] = (int64_t*)realloc(rec[e], (KP_OUT_HDR + (size_t)KP_OUT_WORDS * n[e]) * 8);
			for (j = 0; j < n[e]; ++j) if (regs[e][KM_REG_WORDS * j + 4] < 0 || regs[e][KM_REG_WORDS * j + 4] >= idx->ref->n_seqs) rc = -1;
		}
		if (rc < 0) break;
		ora_kat_pair(&opt, idx->ref, k.pes, (k.n_processed >> 1) + (i[0] >> 1), n, regs, marked, rec, pair5, extra);
		for (e = 0; e < 2; ++e) {
			int64_t hdr[2];
			hdr[0] = i[e]; hdr[1] = n[e];
			rec_write(out, TAG_READ, 2, hdr);
			rec_write(out, KP_TAG_MARKED, 2 + (int64_t)KM_REG_WORDS * n[e], marked[e]);
			rec_write(out, KP_TAG_PAIR, KP_OUT_HDR + (int64_t)KP_OUT_WORDS * n[e], rec[e]);
			if (e == 0) { rec_write(out, KP_TAG_MEMPAIR, 5, pair5); rec_write(out, KP_TAG_EXTRA, ORA_KAT_PAIR_EXTRA, extra); }
		}
	}
	for (e = 0; e < 2; ++e) { free(marked[e]); free(rec[e]); }
	kp_free(&k);
	fclose(in); fclose(out);
	ora_index_destroy(idx);
	if (rc) fprintf(stderr, "[bwa_oracle] katpair: malformed case file\n");
	return rc ? 1 : 0;
}

static int main_mem(int argc, char **argv)
{
	ora_opt_t opt;
	int c, n;
	int64_t n_processed = 0;
	double t_align = 0;
	ora_index_t *idx;
	fq_t f1 = { 0, 0, 0, 0 }, f2 = { 0, 0, 0, 0 };
	ora_read_t *seqs;
	optparse_t op;
	ora_opt_init(&opt);
	optparse_init(&op, &opt);
	while ((c = getopt(argc, argv, OPT_GETOPT_STRING)) >= 0) if (optparse_one(&op, c, optarg)) return 1;
	if (optparse_finish(&op) || optind + 2 > argc) return 1;
	idx = ora_index_load(argv[optind]);
	if (op.ignore_alt) for (c = 0; c < idx->ref->n_seqs; ++c) idx->ref->anns[c].is_alt = 0;
	f1.fp = gzopen(argv[optind + 1], "r");
	if (optind + 2 < argc && !op.smart_pe) { f2.fp = gzopen(argv[optind + 2], "r"); opt.flag |= ORA_F_PE; }
	strcpy(ora_rg_id, op.rg_id);
	{
		int chunk = op.fixed_chunk > 0 ? op.fixed_chunk : opt.chunk_size * opt.n_threads;   /* fastmap.c:304 */
		while ((seqs = read_batch(chunk, &n, &f1, f2.fp ? &f2 : 0)) != 0) {
			int i;
			if (n == 0) { free(seqs); break; }
			if (!op.copy_comment) for (i = 0; i < n; ++i) { free(seqs[i].comment); seqs[i].comment = 0; }     /* stock behaviour without -C */
			{ double t0 = now_s(); ora_process_seqs(&opt, idx, n_processed, n, seqs, op.has_pes0 ? op.pes : 0); t_align += now_s() - t0; }
			n_processed += n;
			for (i = 0; i < n; ++i) {
				if (seqs[i].sam) fputs(seqs[i].sam, stdout);
				free(seqs[i].name); free(seqs[i].seq); free(seqs[i].qual); free(seqs[i].sam);
			}
			free(seqs);
		}
	}
	fprintf(stderr, "[bwa_oracle] aligned %lld reads in %.3f s with %d threads (process_seqs only)\n", (long long)n_processed, t_align, opt.n_threads);
	gzclose(f1.fp); if (f2.fp) gzclose(f2.fp);
	free(f1.line); free(f2.line);
	ora_index_destroy(idx);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && strcmp(argv[1], "mem") == 0) return main_mem(argc - 1, argv + 1);
	if (argc >= 2 && strcmp(argv[1], "stages") == 0) return main_stages(argc - 1, argv + 1);
	if (argc >= 2 && strcmp(argv[1], "katchain") == 0) return main_katchain(argc - 1, argv + 1);
	if (argc >= 2 && strcmp(argv[1], "katmark") == 0) return main_katmark(argc - 1, argv + 1);
	if (argc >= 2 && strcmp(argv[1], "katdedup") == 0) return main_katdedup(argc - 1, argv + 1);
	if (argc >= 2 && strcmp(argv[1], "katpair") == 0) return main_katpair(argc - 1, argv + 1);
	fprintf(stderr, "usage: bwa_oracle <mem|stages|katchain|katmark|katdedup|katpair> ...\n");
	return 1;
}
