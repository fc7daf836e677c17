/* TEST INFRASTRUCTURE ONLY.
 *
 * The case file of `bwa_oracle katdedup` and `bwaref katdedup` (tests/dedup_cases.py writes it), read the same way by both front ends;
 * the includer has defined OPT_T as for opt_parse.h.  i64 records [tag][n][n words]:
 *   KD_TAG_OPT  once, in front: the option fields set on the option struct AFTER the command line -- [bits of mask_level_redun (`bwa mem`
 *               has no flag for it), max_chain_gap]
 *   per read:   TAG_READ [i, l], KD_TAG_SEQ [l base codes 0..4, one per word], then record 4 [n, 19 words per region] as the stage dumps
 *               write a region list.
 * The answer, per read: TAG_READ [i, n], KD_TAG_OUT [n, KD_STAT_WORDS words of what the function did (ora.h ORA_DS_*; bwaref writes
 * zeros: the reference does not count), then the 19 words of every region of the final list].
 */
#ifndef ORA_KAT_DEDUP_IO_H
#define ORA_KAT_DEDUP_IO_H
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { KD_TAG_OPT = 42, KD_TAG_SEQ = 43, KD_TAG_OUT = 44, KD_TAG_READ = 100, KD_TAG_REGS = 4, KD_REG_WORDS = 19, KD_STAT_WORDS = 9 };

typedef struct { int64_t *buf; size_t m; uint8_t *seq; size_t m_seq; } kd_file_t;

/* the leading option record; 0 when it was there */
static int kd_read_opt(FILE *in, OPT_T *opt, kd_file_t *k)
{
	int64_t hdr[2], w[2];
	uint32_t u;
	memset(k, 0, sizeof *k);
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KD_TAG_OPT || hdr[1] != 2 || fread(w, 8, 2, in) != 2) return 1;
	u = (uint32_t)w[0]; memcpy(&opt->mask_level_redun, &u, 4);
	opt->max_chain_gap = (int)w[1];
	return 0;
}

/* the next read: 1 with *i, *l, *seq (l codes), *n and *regs (n x 19 words), all owned by k; 0 at the end of the file, -1 for a malformed file */
static int kd_next_read(FILE *in, kd_file_t *k, int64_t *i, int *l, uint8_t **seq, int *n, const int64_t **regs)
{
	int64_t hdr[4], t;
	if (fread(hdr, 8, 2, in) != 2) return 0;
	if (hdr[0] != KD_TAG_READ || hdr[1] != 2 || fread(hdr + 2, 8, 2, in) != 2 || hdr[3] < 0 || hdr[3] > (1 << 20)) return -1;
	*i = hdr[2]; *l = (int)hdr[3];
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KD_TAG_SEQ || hdr[1] != *l) return -1;
	if ((size_t)*l + 1 > k->m) { k->m = (size_t)*l + 1; k->buf = (int64_t*)realloc(k->buf, k->m * 8); }
	if ((size_t)*l + 1 > k->m_seq) { k->m_seq = (size_t)*l + 1; k->seq = (uint8_t*)realloc(k->seq, k->m_seq); }
	if (fread(k->buf, 8, (size_t)*l, in) != (size_t)*l) return -1;
	for (t = 0; t < *l; ++t) { if (k->buf[t] < 0 || k->buf[t] > 4) return -1; k->seq[t] = (uint8_t)k->buf[t]; }
	*seq = k->seq;
	if (fread(hdr, 8, 2, in) != 2 || hdr[0] != KD_TAG_REGS || hdr[1] < 1) return -1;
	if ((size_t)hdr[1] > k->m) { k->m = (size_t)hdr[1]; k->buf = (int64_t*)realloc(k->buf, k->m * 8); }
	if (fread(k->buf, 8, (size_t)hdr[1], in) != (size_t)hdr[1]) return -1;
	if (k->buf[0] < 2 || k->buf[0] * KD_REG_WORDS + 1 != hdr[1]) return -1;
	*n = (int)k->buf[0]; *regs = k->buf + 1;
	return 1;
}

#endif
