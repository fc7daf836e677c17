/* TEST INFRASTRUCTURE ONLY.
 *
 * The case file of `bwa_oracle katpair` and `bwaref katpair` (tests/pair_cases.py writes it), read the same way by both front ends; the
 * includer has defined OPT_T and PES_T as for opt_parse.h and included kat_mark_io.h.  i64 records [tag][n][n words]:
 *   KP_TAG_OPT  once, in front: the option record of kat_mark_io.h without `paired` -- [bits of mask_level, bits of mapQ_coef_len,
 *               mapQ_coef_fac, bits of XA_drop_ratio, bits of drop_ratio, n_processed] -- then pen_unpaired and the flag word, both set on
 *               the option struct AFTER the command line, then the four insert-size records [low, high, failed, bits of avg, bits of std].
 *   per read:   TAG_READ [i, 0], then record 4 [n, 19 words per region], as in kat_mark_io.h.  Reads 2p and 2p + 1 are pair p, whose id
 *               is (n_processed >> 1) + p.
 * The answer, per read: TAG_READ [i, n]; KP_TAG_MARKED [n, n_pri, 19 words per region as marked, before mem_pair]; from the oracle
 * KP_TAG_PAIR [12 + 22 n words, see ora_kat_pair]; and with the first read of a pair KP_TAG_MEMPAIR [ret, sub, n_sub, z[0], z[1] of
 * mem_pair, z -1 where it set none; 0 0 0 -1 -1 when mem_sam_pe would not call it] and, from the oracle, KP_TAG_EXTRA (ora_kat_pair).
 */
#ifndef ORA_KAT_PAIR_IO_H
#define ORA_KAT_PAIR_IO_H
#include "kat_mark_io.h"

enum { KP_TAG_OPT = 42, KP_TAG_PAIR = 43, KP_TAG_EXTRA = 44, KP_TAG_MEMPAIR = 45, KP_TAG_MARKED = 46, KP_OPT_WORDS = 28, KP_OUT_HDR = 12, KP_OUT_WORDS = 22 };

typedef struct { int64_t n_processed; PES_T pes[4]; km_file_t km; int64_t *regs[2]; size_t m[2]; } kp_file_t;

static inline double kp_i2d(int64_t w) { double d; memcpy(&d, &w, 8); return d; }

/* the leading option record; 0 when it was there */
static int kp_read_opt(FILE *in, OPT_T *opt, kp_file_t *k)
{
	int64_t hdr[2], w[KP_OPT_WORDS];
	int d;
	memset(k, 0, sizeof *k);
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KP_TAG_OPT || hdr[1] != KP_OPT_WORDS || fread(w, 8, KP_OPT_WORDS, in) != KP_OPT_WORDS) return 1;
	opt->mask_level = km_i2f(w[0]); opt->mapQ_coef_len = km_i2f(w[1]); opt->mapQ_coef_fac = (int)w[2];
	opt->XA_drop_ratio = km_i2f(w[3]); opt->drop_ratio = km_i2f(w[4]);
	k->n_processed = w[5];
	opt->pen_unpaired = (int)w[6]; opt->flag = (int)w[7];
	for (d = 0; d < 4; ++d) {
		const int64_t *p = w + 8 + 5 * d;
		k->pes[d].low = (int)p[0]; k->pes[d].high = (int)p[1]; k->pes[d].failed = (int)p[2]; k->pes[d].avg = kp_i2d(p[3]); k->pes[d].std = kp_i2d(p[4]);
	}
	return 0;
}

/* the next pair: 1 with i[2], n[2] and regs[2] (n x 19 words each, owned by k) set, 0 at the end of the file, -1 for a malformed file */
static int kp_next_pair(FILE *in, kp_file_t *k, int64_t i[2], int n[2], const int64_t *regs[2])
{
	int e, rc;
	for (e = 0; e < 2; ++e) {
		const int64_t *r;
		size_t bytes;
		if ((rc = km_next_read(in, &k->km, &i[e], &n[e], &r)) <= 0) return e == 0 ? rc : -1;
		bytes = (size_t)n[e] * KM_REG_WORDS * 8;
		if (bytes + 8 > k->m[e]) { k->m[e] = bytes + 8; k->regs[e] = (int64_t*)realloc(k->regs[e], k->m[e]); }
		memcpy(k->regs[e], r, bytes);
		regs[e] = k->regs[e];
	}
	return i[1] == i[0] + 1 && !(i[0] & 1) ? 1 : -1;
}

static void kp_free(kp_file_t *k) { free(k->km.buf); free(k->regs[0]); free(k->regs[1]); }

#endif
