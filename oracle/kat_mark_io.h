/* TEST INFRASTRUCTURE ONLY.
 *
 * The case file of `bwa_oracle katmark` and `bwaref katmark` (tests/mark_cases.py writes it), read the same way by both front ends;
 * the includer has defined OPT_T as for opt_parse.h.  i64 records [tag][n][n words]:
 *   KM_TAG_OPT  once, in front: the option fields `bwa mem` has no flag for, set on the option struct AFTER the command line --
 *               [bits of mask_level, bits of mapQ_coef_len, mapQ_coef_fac, bits of XA_drop_ratio, bits of drop_ratio, n_processed,
 *               paired (the id given to mem_mark_primary_se: n_processed + i, or ((n_processed >> 1) + (i >> 1)) << 1 | (i & 1))]
 *   per read:   TAG_READ [i, 0], then record 4 [n, 19 words per region] as the stage dumps write a region list.
 * The answer, per read: TAG_READ [i, n], KM_TAG_MARK [n, n_pri, regions with a task, regions with a record, then per region of the
 * final order 25 words: the 19 of a stage record, hash, index in the input list, need, XA owner, mapQ, bad].
 */
#ifndef ORA_KAT_MARK_IO_H
#define ORA_KAT_MARK_IO_H
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { KM_TAG_OPT = 40, KM_TAG_MARK = 41, KM_TAG_READ = 100, KM_TAG_REGS = 4, KM_REG_WORDS = 19, KM_OUT_WORDS = 25 };

typedef struct { int64_t n_processed; int paired; int64_t *buf; size_t m; } km_file_t;

static inline float km_i2f(int64_t w) { uint32_t u = (uint32_t)w; float f; memcpy(&f, &u, 4); return f; }

/* the leading option record; 0 when it was there */
static int km_read_opt(FILE *in, OPT_T *opt, km_file_t *k)
{
	int64_t hdr[2], w[7];
	memset(k, 0, sizeof *k);
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KM_TAG_OPT || hdr[1] != 7 || fread(w, 8, 7, in) != 7) return 1;
	opt->mask_level = km_i2f(w[0]); opt->mapQ_coef_len = km_i2f(w[1]); opt->mapQ_coef_fac = (int)w[2];
	opt->XA_drop_ratio = km_i2f(w[3]); opt->drop_ratio = km_i2f(w[4]);
	k->n_processed = w[5]; k->paired = w[6] != 0;
	return 0;
}

/* the next read: 1 with *i, *n and *regs (n x 19 words, owned by k) set, 0 at the end of the file, -1 for a malformed file */
static int km_next_read(FILE *in, km_file_t *k, int64_t *i, int *n, const int64_t **regs)
{
	int64_t hdr[4];
	if (fread(hdr, 8, 2, in) != 2) return 0;
	if (hdr[0] != KM_TAG_READ || hdr[1] != 2 || fread(hdr + 2, 8, 2, in) != 2) return -1;
	*i = hdr[2];
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KM_TAG_REGS || hdr[1] < 1) return -1;
	if ((size_t)hdr[1] > k->m) { k->m = (size_t)hdr[1]; k->buf = (int64_t*)realloc(k->buf, k->m * 8); }
	if (fread(k->buf, 8, (size_t)hdr[1], in) != (size_t)hdr[1]) return -1;
	if (k->buf[0] < 0 || k->buf[0] * KM_REG_WORDS + 1 != hdr[1]) return -1;
	*n = (int)k->buf[0]; *regs = k->buf + 1;
	return 1;
}

static inline int64_t km_read_id(const km_file_t *k, int64_t i)
{
	return k->paired ? (((k->n_processed >> 1) + (i >> 1)) << 1 | (i & 1)) : k->n_processed + i;
}

#endif
