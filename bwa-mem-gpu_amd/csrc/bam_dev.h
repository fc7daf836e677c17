// BAM records on the device (SAM specification section 4.2): the binary consumer of the resolved record of rec_dev.h, next to the
// text consumer of sam_dev.h.  Wavefront-collective like the text path; the same body sizes (dst == nullptr) and writes.  A record
// starts wherever the previous one ended, so every store is a single byte (one per lane): nothing is ever misaligned for its width.
// The variable part is written first (the name's length is known once it has been copied); the 36-byte fixed part, block_size
// included, goes last -- lanes 0..35 store one byte each of nine words held in registers.
#pragma once
#include "sam_dev.h"
#include "bam_rec.h"

namespace samdev {

// B/i tags by the rule of every SAM -> BAM converter: the smallest type that holds the value (negative: c s i, else C S I)
__device__ __forceinline__ void bam_tag_int(Emit &e, char t0, char t1, long long v)
{
	char ty; int nb;
	if (v < 0) { if (v >= -128) { ty = 'c'; nb = 1; } else if (v >= -32768) { ty = 's'; nb = 2; } else { ty = 'i'; nb = 4; } }
	else { if (v <= 255) { ty = 'C'; nb = 1; } else if (v <= 65535) { ty = 'S'; nb = 2; } else { ty = 'I'; nb = 4; } }
	e.word((unsigned long long)(uint8_t)t0 | (unsigned long long)(uint8_t)t1 << 8 | (unsigned long long)(uint8_t)ty << 16 | ((unsigned long long)v & 0xffffffffull) << 24, 3 + nb);
}
__device__ __forceinline__ void bam_tag_head(Emit &e, char t0, char t1, char ty) { e.word((unsigned long long)(uint8_t)t0 | (unsigned long long)(uint8_t)t1 << 8 | (unsigned long long)(uint8_t)ty << 16, 3); }

// The -C comment as tags.  The host has checked (bam_check_reads) that every tab-separated field is XX:Z:<printable>, XX:A:<char>
// or XX:i:<integer in [-2^31, 2^32)>.  All lanes scan the same bytes (uniform loads); the values are copied one byte per lane.
__device__ __forceinline__ void bam_comment_tags(Emit &e, const uint8_t *c)
{
	int i = 0;
	for (;;) {
		int j = i;
		while (c[j] && c[j] != '\t') ++j;
		const char t0 = (char)c[i], t1 = (char)c[i + 1], ty = (char)c[i + 3];   // (buffers are padded by 64)
		i += 5;
		if (j < i) ;                                                // not a tag (only where the host check was bypassed): dropped
		else if (ty == 'Z') { bam_tag_head(e, t0, t1, 'Z'); e.bytes(c + i, j - i); e.ch(0); }
		else if (ty == 'A') { bam_tag_head(e, t0, t1, 'A'); e.ch((char)c[i]); }
		else {
			long long v = 0;
			int k = i;
			const bool neg = c[k] == '-';
			if (c[k] == '-' || c[k] == '+') ++k;
			for (; k < j; ++k) v = v * 10 + (c[k] - '0');
			bam_tag_int(e, t0, t1, neg ? -v : v);
		}
		if (!c[j]) break;
		i = j + 1;
	}
}

// CIGAR operations of the pool are bwa's ("MIDSH": S = 3, H = 4); BAM's are "MIDNSHP=X" (S = 4, H = 5)
__device__ __forceinline__ uint32_t bam_cigar_word(const Tables &t, const Rec &R, const DevAln &p, uint32_t w)
{
	const int c = R.clip_op(t, p, (int)(w & 0xf));
	return (w & ~0xfu) | (uint32_t)(c < 3 ? c : c + 1);
}

__device__ void emit_bam_record(Emit &e, const Tables &t, const ReadText &s, int n, const DevAln *const *list, int which, const DevAln *m_,
                                int n_xa, const DevAln *const *xa)
{
	Rec R;
	resolve_record(R, n, list, which, m_, n_xa, xa);
	const DevAln &p = R.p, &mt = R.mt;
	const int64_t rec0 = e.pos;
	e.pos += 36;
	e.cstr(s.name); e.ch(0);
	const int l_read_name = (int)(e.pos - rec0 - 36);
	const int n_cigar = R.placed() ? p.n_cigar : 0;
	if (n_cigar) {
		const uint32_t *cg = cigar_of(t, p);
		if (e.dst) for (int i = e.l; i < 4 * n_cigar; i += 64) e.dst[e.pos + i] = (uint8_t)(bam_cigar_word(t, R, p, cg[i >> 2]) >> (8 * (i & 3)));
		e.pos += 4 * n_cigar;
	}
	int l_seq = 0;
	if (!R.no_seq()) {
		int qb, qe;
		R.seq_range(t, s, qb, qe);
		l_seq = qe - qb;
		const int nb = (l_seq + 1) >> 1;
		if (e.dst) {
			// codes 0..4 -> 1, 2, 4, 8, 15 ("=ACMGRSVTWYHKDBN"); reverse strand: complemented and reversed, as the text path does
			for (int i = e.l; i < nb; i += 64) {
				const int k0 = 2 * i, k1 = 2 * i + 1;
				int c0, c1 = -1;
				if (!p.is_rev) { c0 = s.seq[qb + k0]; if (k1 < l_seq) c1 = s.seq[qb + k1]; }
				else {
					c0 = s.seq[qe - 1 - k0]; c0 = c0 < 4 ? 3 - c0 : c0;
					if (k1 < l_seq) { c1 = s.seq[qe - 1 - k1]; c1 = c1 < 4 ? 3 - c1 : c1; }
				}
				const int h = c0 < 4 ? 1 << c0 : 15, lo = c1 < 0 ? 0 : c1 < 4 ? 1 << c1 : 15;
				e.dst[e.pos + i] = (uint8_t)(h << 4 | lo);
			}
		}
		e.pos += nb;
		if (e.dst) {
			if (!s.qual) for (int i = e.l; i < l_seq; i += 64) e.dst[e.pos + i] = 0xff;
			else if (!p.is_rev) for (int i = e.l; i < l_seq; i += 64) e.dst[e.pos + i] = (uint8_t)(s.qual[qb + i] - 33);
			else for (int i = e.l; i < l_seq; i += 64) e.dst[e.pos + i] = (uint8_t)(s.qual[qe - 1 - i] - 33);
		}
		e.pos += l_seq;
	}
	// optional tags, in the order of the text
	if (R.has_nm_md()) {
		bam_tag_int(e, 'N', 'M', (long long)p.NM);
		bam_tag_head(e, 'M', 'D', 'Z'); e.bytes(t.pool + p.md_off, p.md_len); e.ch(0);
	}
	if (R.has_mc()) { bam_tag_head(e, 'M', 'C', 'Z'); emit_cigar(e, t, R, mt); e.ch(0); }
	if (R.has_as()) bam_tag_int(e, 'A', 'S', p.score);
	if (R.has_xs()) bam_tag_int(e, 'X', 'S', p.sub);
	if (t.rg_len) { bam_tag_head(e, 'R', 'G', 'Z'); e.bytes(t.rg_id, t.rg_len); e.ch(0); }
	if (R.has_sa()) { bam_tag_head(e, 'S', 'A', 'Z'); emit_sa_value(e, t, R); e.ch(0); }
	if (R.has_pa()) {
		// the IEEE single nearest to the PRINTED three-decimal text
		const float v = (float)((double)f3_milli((double)p.score / p.alt_sc) / 1000.0);
		bam_tag_head(e, 'p', 'a', 'f'); e.word((unsigned long long)__float_as_uint(v), 4);
	}
	if (n_xa > 0) { bam_tag_head(e, 'X', (t.opt_flag & BWAHIP_F_XB) ? 'B' : 'A', 'Z'); emit_xa_value(e, t, R); e.ch(0); }
	if (s.comment) bam_comment_tags(e, s.comment);
	if (R.has_xr(t)) { bam_tag_head(e, 'X', 'R', 'Z'); emit_xr_value(e, t, R); e.ch(0); }
	// the fixed part
	if (e.dst && e.l < 36) {
		const int64_t pos = R.placed() ? p.pos : -1;
		int64_t end = pos + 1;
		if (R.placed() && !(p.flag & 0x4) && p.n_cigar) { const int rl = get_rlen(t, p); if (rl) end = pos + rl; }
		const uint32_t bin = bam_reg2bin(pos, end) & 0xffff, mapq = R.placed() ? p.mapq & 0xff : 0;
		const uint32_t w0 = (uint32_t)(e.pos - rec0 - 4), w1 = (uint32_t)(R.placed() ? p.rid : -1), w2 = (uint32_t)(int32_t)pos,
		               w3 = (uint32_t)l_read_name | mapq << 8 | bin << 16, w4 = (uint32_t)n_cigar | (uint32_t)R.out_flag() << 16, w5 = (uint32_t)l_seq,
		               w6 = (uint32_t)(R.mate_placed() ? mt.rid : -1), w7 = (uint32_t)(int32_t)(R.mate_placed() ? mt.pos : -1),
		               w8 = (uint32_t)(int32_t)(R.mate_placed() ? R.tlen(t) : 0);
		const int k = e.l >> 2;
		const uint32_t w = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : k == 3 ? w3 : k == 4 ? w4 : k == 5 ? w5 : k == 6 ? w6 : k == 7 ? w7 : w8;
		e.dst[rec0 + e.l] = (uint8_t)(w >> (8 * (e.l & 3)));
	}
}

struct BamFmt {
	static __device__ __forceinline__ void record(Emit &e, const Tables &t, const ReadText &s, int n, const DevAln *const *list, int which, const DevAln *m,
	                                              int n_xa, const DevAln *const *xa) { emit_bam_record(e, t, s, n, list, which, m, n_xa, xa); }
};

} // namespace samdev
