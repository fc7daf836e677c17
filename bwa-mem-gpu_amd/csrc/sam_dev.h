// SAM text on the device (mem_aln2sam, bwamem.c:832-956, and the kstring helpers it uses): the text consumer of the resolved
// record of rec_dev.h.  All functions are wavefront-collective: every lane makes the same calls with the same (uniform)
// arguments; `pos` advances identically in all lanes.  Bulk fields (name, SEQ, QUAL, MD) are copied one byte per lane.  The
// emitters of tag VALUES (CIGAR strings, SA, XA / XB, XR) are shared with the BAM encoding (bam_dev.h), where they are Z tags.
#pragma once
#include "rec_dev.h"

namespace samdev {

__device__ __forceinline__ void emit_f3(Emit &e, double x)
{
	const long long N = f3_milli(x);
	e.num(N / 1000);
	e.ch('.');
	const int fr = (int)(N % 1000);
	e.ch((char)('0' + fr / 100)); e.ch((char)('0' + fr / 10 % 10)); e.ch((char)('0' + fr % 10));
}

__device__ __forceinline__ void emit_ctg(Emit &e, const Tables &t, int rid) { e.bytes(t.ctg_names + t.ctg_name_off[rid], t.ctg_name_off[rid + 1] - t.ctg_name_off[rid]); }

// add_cigar (bwamem.c:819-830)
__device__ __forceinline__ void emit_cigar(Emit &e, const Tables &t, const Rec &R, const DevAln &p)
{
	if (p.n_cigar == 0) { e.ch('*'); return; }
	const uint32_t *cg = cigar_of(t, p);
	for (int i = 0; i < p.n_cigar; ++i) { e.num(cg[i] >> 4); e.ch("MIDSH"[R.clip_op(t, p, cg[i] & 0xf)]); }
}

// One XA / XB entry (mem_gen_alt, bwamem_extra.c:147-160)
__device__ __forceinline__ void emit_xa_entry(Emit &e, const Tables &t, const DevAln &q)
{
	emit_ctg(e, t, q.rid);
	e.ch(','); e.ch("+-"[q.is_rev]); e.num(q.pos + 1); e.ch(',');
	const uint32_t *cg = cigar_of(t, q);
	for (int i = 0; i < q.n_cigar; ++i) { e.num(cg[i] >> 4); e.ch("MIDSHN"[cg[i] & 0xf]); }
	e.ch(','); e.num(q.NM);
	if (t.opt_flag & BWAHIP_F_XB) { e.ch(','); e.num(q.score); }
	e.ch(';');
}

// values of the SA / XA (XB) / XR tags
__device__ __forceinline__ void emit_sa_value(Emit &e, const Tables &t, const Rec &R)
{
	for (int i = 0; i < R.n; ++i) {
		if (!R.in_sa(i)) continue;
		const DevAln &q = *R.list[i];
		emit_ctg(e, t, q.rid); e.ch(',');
		e.num(q.pos + 1); e.ch(',');
		e.ch("+-"[q.is_rev]); e.ch(',');
		const uint32_t *cg = cigar_of(t, q);
		for (int k = 0; k < q.n_cigar; ++k) { e.num(cg[k] >> 4); e.ch("MIDSH"[cg[k] & 0xf]); }
		e.ch(','); e.num(q.mapq);
		e.ch(','); e.num(q.NM);
		e.ch(';');
	}
}
__device__ __forceinline__ void emit_xa_value(Emit &e, const Tables &t, const Rec &R) { for (int i = 0; i < R.n_xa; ++i) emit_xa_entry(e, t, *R.xa[i]); }
__device__ __forceinline__ void emit_xr_value(Emit &e, const Tables &t, const Rec &R)   // bwamem.c:948-954: tabs become spaces
{
	const uint8_t *an = t.ctg_anno + t.ctg_anno_off[R.p.rid];
	const int la = t.ctg_anno_off[R.p.rid + 1] - t.ctg_anno_off[R.p.rid];
	if (e.dst) for (int i = e.l; i < la; i += 64) e.dst[e.pos + i] = an[i] == '\t' ? (uint8_t)' ' : an[i];
	e.pos += la;
}

// mem_aln2sam (bwamem.c:832-956) as text.  list: the read's records (n of them, pointers into the alignment array), `which` the one
// to print; m: the mate's primary record or nullptr; xa_* : the XA members of this record (alignments, in order).
__device__ void emit_record(Emit &e, const Tables &t, const ReadText &s, int n, const DevAln *const *list, int which, const DevAln *m_,
                            int n_xa, const DevAln *const *xa)
{
	Rec R;
	resolve_record(R, n, list, which, m_, n_xa, xa);
	const DevAln &p = R.p, &mt = R.mt;
	e.cstr(s.name); e.ch('\t');
	e.num(R.out_flag()); e.ch('\t');
	if (R.placed()) {
		emit_ctg(e, t, p.rid); e.ch('\t');
		e.num(p.pos + 1); e.ch('\t');
		e.num(p.mapq); e.ch('\t');
		emit_cigar(e, t, R, p);
	} else e.lit("*\t0\t0\t*", 7);
	e.ch('\t');
	if (R.mate_placed()) {                                        // mate position and template length (bwamem.c:863-875)
		if (p.rid == mt.rid) e.ch('='); else emit_ctg(e, t, mt.rid);
		e.ch('\t');
		e.num(mt.pos + 1); e.ch('\t');
		e.num(R.tlen(t));
	} else e.lit("*\t0\t0", 5);
	e.ch('\t');
	if (R.no_seq()) e.lit("*\t*", 3);
	else {
		int qb, qe;
		R.seq_range(t, s, qb, qe);
		const int len = qe - qb;
		if (e.dst) {
			if (!p.is_rev) for (int i = e.l; i < len; i += 64) e.dst[e.pos + i] = (uint8_t)"ACGTN"[s.seq[qb + i]];
			else for (int i = e.l; i < len; i += 64) e.dst[e.pos + i] = (uint8_t)"TGCAN"[s.seq[qe - 1 - i]];
		}
		e.pos += len;
		e.ch('\t');
		if (s.qual) {
			if (e.dst) {
				if (!p.is_rev) for (int i = e.l; i < len; i += 64) e.dst[e.pos + i] = s.qual[qb + i];
				else for (int i = e.l; i < len; i += 64) e.dst[e.pos + i] = s.qual[qe - 1 - i];
			}
			e.pos += len;
		} else e.ch('*');
	}
	// optional tags
	if (R.has_nm_md()) {
		e.lit("\tNM:i:", 6); e.num(p.NM);
		e.lit("\tMD:Z:", 6); e.bytes(t.pool + p.md_off, p.md_len);
	}
	if (R.has_mc()) { e.lit("\tMC:Z:", 6); emit_cigar(e, t, R, mt); }
	if (R.has_as()) { e.lit("\tAS:i:", 6); e.num(p.score); }
	if (R.has_xs()) { e.lit("\tXS:i:", 6); e.num(p.sub); }
	if (t.rg_len) { e.lit("\tRG:Z:", 6); e.bytes(t.rg_id, t.rg_len); }
	if (R.has_sa()) { e.lit("\tSA:Z:", 6); emit_sa_value(e, t, R); }
	if (R.has_pa()) { e.lit("\tpa:f:", 6); emit_f3(e, (double)p.score / p.alt_sc); }
	if (n_xa > 0) {
		e.lit((t.opt_flag & BWAHIP_F_XB) ? "\tXB:Z:" : "\tXA:Z:", 6);
		emit_xa_value(e, t, R);
	}
	if (s.comment) { e.ch('\t'); e.cstr(s.comment); }
	if (R.has_xr(t)) { e.lit("\tXR:Z:", 6); emit_xr_value(e, t, R); }
	e.ch('\n');
}

struct TextFmt {
	static __device__ __forceinline__ void record(Emit &e, const Tables &t, const ReadText &s, int n, const DevAln *const *list, int which, const DevAln *m,
	                                              int n_xa, const DevAln *const *xa) { emit_record(e, t, s, n, list, which, m, n_xa, xa); }
};

} // namespace samdev
