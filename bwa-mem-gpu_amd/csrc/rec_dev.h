// The output records of a read, resolved: everything mem_reg2sam / mem_sam_pe / mem_aln2sam DECIDE (which regions become records,
// supplementary flag, mapQ cap, XS of secondaries, extra flags, proper-pair bit, mate fields and the bwamem.c:842-845 swaps, hard-clip
// trimming of SEQ / QUAL, which tags appear, XA ownership), kept apart from how a record is written.  Two consumers: the SAM text
// (sam_dev.h, k_sam.hip) and the BAM encoding (bam_dev.h, k_bam.hip) -- both run the code below, so the formats cannot drift.
// All functions are wavefront-collective: every lane makes the same calls with the same (uniform) arguments.
#pragma once
#include "bwahip_internal.h"

namespace samdev {

// Byte sink of one wavefront.  `pos` advances identically in all lanes; in the sizing pass (dst == nullptr) nothing is stored, so one
// body serves both passes and the two can never disagree about a length.  Bulk fields are copied one byte per lane.
struct Emit {
	uint8_t *dst; int64_t pos; int l;
	__device__ __forceinline__ void ch(char c) { if (dst && l == 0) dst[pos] = (uint8_t)c; ++pos; }
	__device__ __forceinline__ void lit(const char *s, int n) { if (dst && l < n) dst[pos + l] = (uint8_t)s[l]; pos += n; }   // n <= 64
	__device__ __forceinline__ void bytes(const uint8_t *s, int n) { if (dst) for (int i = l; i < n; i += 64) dst[pos + i] = s[i]; pos += n; }
	// the low n (<= 8) bytes of w, least significant first: byte stores, so nothing is misaligned wherever pos is
	__device__ __forceinline__ void word(unsigned long long w, int n) { if (dst && l < n) dst[pos + l] = (uint8_t)(w >> (8 * l)); pos += n; }
	// NUL-terminated string of unknown length in global memory
	__device__ __forceinline__ void cstr(const uint8_t *s)
	{
		int n = 0;
		for (;; n += 64) {
			const bool z = s[n + l] == 0;                          // reads up to 63 bytes past the NUL: buffers are padded by 64
			const unsigned long long m = __ballot(z);
			if (m) { const int k = __ffsll((long long)m) - 1; if (dst && l < k) dst[pos + n + l] = s[n + l]; n += k; break; }
			if (dst) dst[pos + n + l] = s[n + l];
		}
		pos += n;
	}
	// kputw / kputl: decimal, '-' for negatives
	__device__ __forceinline__ void num(long long v)
	{
		unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
		int nd = 1;
		for (unsigned long long t = u; t >= 10; t /= 10) ++nd;
		if (v < 0) ch('-');
		if (dst && l < nd) {                                       // lane k writes the k-th digit from the left
			unsigned long long t = u;
			for (int s = nd - 1 - l; s > 0; --s) t /= 10;
			dst[pos + l] = (uint8_t)('0' + t % 10);
		}
		pos += nd;
	}
};

struct Tables {
	const uint8_t *ctg_names; const int *ctg_name_off; const uint8_t *ctg_anno; const int *ctg_anno_off;
	const uint8_t *pool; const uint8_t *rg_id; int rg_len; int opt_flag;
};
struct ReadText { const uint8_t *name, *comment, *seq /* codes 0..4 */, *qual; int l_seq; };

__device__ __forceinline__ const uint32_t *cigar_of(const Tables &t, const DevAln &p) { return reinterpret_cast<const uint32_t*>(t.pool + p.cigar_off); }
__device__ __forceinline__ int get_rlen(const Tables &t, const DevAln &p)   // bwamem.c:808
{
	int rl = 0;
	const uint32_t *cg = cigar_of(t, p);
	for (int i = 0; i < p.n_cigar; ++i) { const int op = cg[i] & 0xf; if (op == 0 || op == 2) rl += (int)(cg[i] >> 4); }
	return rl;
}

// One record of mem_aln2sam (bwamem.c:832-956) after its decisions.  list: the read's records (n of them), `which` the one being
// written; xa: the XA members of this record.  p / mt are copies with the flags and the swaps of bwamem.c:837-847 applied.
struct Rec {
	DevAln p, mt; bool has_m;
	int n, which, n_xa; const DevAln *const *list, *const *xa;

	__device__ __forceinline__ int out_flag() const { return (p.flag & 0xffff) | ((p.flag & 0x10000) ? 0x100 : 0); }
	__device__ __forceinline__ bool placed() const { return p.rid >= 0; }                    // RNAME / POS / MAPQ / CIGAR are printed (else "*", 0, 0, "*")
	__device__ __forceinline__ bool mate_placed() const { return has_m && mt.rid >= 0; }     // RNEXT / PNEXT / TLEN
	__device__ __forceinline__ bool no_seq() const { return (p.flag & 0x100) != 0; }         // secondary: SEQ and QUAL are "*"
	// add_cigar (bwamem.c:819-830): clip operations of a supplementary line (which != 0) are H, unless -Y or an ALT hit
	__device__ __forceinline__ int clip_op(const Tables &t, const DevAln &q, int c) const
	{
		if (!(t.opt_flag & BWAHIP_F_SOFTCLIP) && !q.is_alt && (c == 3 || c == 4)) c = which ? 4 : 3;
		return c;
	}
	__device__ __forceinline__ int64_t tlen(const Tables &t) const                           // bwamem.c:868-873
	{
		if (p.rid != mt.rid) return 0;
		const int64_t p0 = p.pos + (p.is_rev ? get_rlen(t, p) - 1 : 0);
		const int64_t p1 = mt.pos + (mt.is_rev ? get_rlen(t, mt) - 1 : 0);
		if (mt.n_cigar == 0 || p.n_cigar == 0) return 0;
		return -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
	}
	// the part of the read a record shows: all of it, less what a supplementary line hard-clips (bwamem.c:879-888)
	__device__ __forceinline__ void seq_range(const Tables &t, const ReadText &s, int &qb, int &qe) const
	{
		qb = 0; qe = s.l_seq;
		const bool hard = p.n_cigar && which && !(t.opt_flag & BWAHIP_F_SOFTCLIP) && !p.is_alt;
		if (hard) {
			const uint32_t *cg = cigar_of(t, p);
			const int o0 = cg[0] & 0xf, o1 = cg[p.n_cigar - 1] & 0xf;
			if (!p.is_rev) { if (o0 == 4 || o0 == 3) qb += (int)(cg[0] >> 4); if (o1 == 4 || o1 == 3) qe -= (int)(cg[p.n_cigar - 1] >> 4); }
			else { if (o0 == 4 || o0 == 3) qe -= (int)(cg[0] >> 4); if (o1 == 4 || o1 == 3) qb += (int)(cg[p.n_cigar - 1] >> 4); }
		}
	}
	// tag presence, in the order the tags are written: NM MD | MC | AS | XS | RG | SA | pa | XA or XB | comment | XR
	__device__ __forceinline__ bool has_nm_md() const { return p.n_cigar != 0; }
	__device__ __forceinline__ bool has_mc() const { return has_m && mt.n_cigar; }
	__device__ __forceinline__ bool has_as() const { return p.score >= 0; }
	__device__ __forceinline__ bool has_xs() const { return p.sub >= 0; }
	__device__ __forceinline__ bool has_sa() const                                           // other primary hits (bwamem.c:922-943)
	{
		if (p.flag & 0x100) return false;
		for (int i = 0; i < n; ++i) if (i != which && !(list[i]->flag & 0x100)) return true;
		return false;
	}
	__device__ __forceinline__ bool in_sa(int i) const { return i != which && !(list[i]->flag & 0x100); }
	__device__ __forceinline__ bool has_pa() const { return !(p.flag & 0x100) && p.alt_sc > 0; }
	__device__ __forceinline__ bool has_xr(const Tables &t) const { return (t.opt_flag & BWAHIP_F_REF_HDR) && p.rid >= 0 && t.ctg_anno_off[p.rid + 1] > t.ctg_anno_off[p.rid]; }
};

__device__ __forceinline__ void resolve_record(Rec &R, int n, const DevAln *const *list, int which, const DevAln *m_, int n_xa, const DevAln *const *xa)
{
	DevAln &p = R.p, &mt = R.mt;
	p = *list[which];
	const bool has_m = m_ != nullptr;
	if (has_m) mt = *m_;
	p.flag |= has_m ? 0x1 : 0;
	p.flag |= p.rid < 0 ? 0x4 : 0;
	p.flag |= has_m && mt.rid < 0 ? 0x8 : 0;
	if (p.rid < 0 && has_m && mt.rid >= 0) { p.rid = mt.rid; p.pos = mt.pos; p.is_rev = mt.is_rev; p.n_cigar = 0; }   // bwamem.c:842-845
	if (has_m && mt.rid < 0 && p.rid >= 0) { mt.rid = p.rid; mt.pos = p.pos; mt.is_rev = p.is_rev; mt.n_cigar = 0; }
	p.flag |= p.is_rev ? 0x10 : 0;
	p.flag |= has_m && mt.is_rev ? 0x20 : 0;
	R.has_m = has_m; R.n = n; R.which = which; R.n_xa = n_xa; R.list = list; R.xa = xa;
}

// "%.3f" of a positive double exactly as printf rounds it (round-half-even on the exact binary value; bwamem.c:945): round(x * 1000)
__device__ __forceinline__ long long f3_milli(double x)
{
	unsigned long long bits = (unsigned long long)__double_as_longlong(x);
	const int ex = (int)(bits >> 52 & 0x7ff);
	unsigned long long m = bits & 0xfffffffffffffull;
	long long N;
	if (ex == 0) N = 0;                                            // zero / subnormal
	else {
		m |= 1ull << 52;
		const int sh = 1075 - ex;                                  // x = m * 2^-sh
		const unsigned long long p = m * 1000ull;                  // < 2^63
		if (sh <= 0) N = (long long)(p << -sh);                    // (huge values are not expected here)
		else if (sh >= 64) N = 0;
		else {
			const unsigned long long q = p >> sh, rem = p & ((1ull << sh) - 1), half = 1ull << (sh - 1);
			N = (long long)(q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0));
		}
	}
	return N;
}

__device__ __forceinline__ int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)   // bwamem_pair.c:48
{
	const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
	const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// ---- the records of one read, one read per wavefront ----------------------------------------------------------------------------
// Two launches of the same code per batch: the first (WRITE = false) computes each read's output length and applies the per-record
// adjustments ONCE to the alignment array (so a batch is sized for exactly one format), an exclusive scan turns lengths into offsets,
// the second writes -- the output of read i always lands at a fixed place, no atomics, deterministic.  Fmt::record(e, t, s, n, list,
// which, mate, n_xa, xa) writes one record.

// Single-end: mem_reg2sam's record list (bwamem.c:1025-1056: supplementary flag, mapQ cap of supplementary hits, XS of secondaries, XA)
template <bool WRITE, class Fmt>
__device__ __forceinline__ void records_se(const FinLaunch &a)
{
	const int r = (int)blockIdx.x + a.read_lo, l = (int)(threadIdx.x & 63);
	const DevOpt &opt = a.opt;
	const int n = a.freg_n[r];
	const int64_t rb0 = a.reg_base[r];
	const FinReg *f = a.fregs + rb0;
	const uint8_t *need = a.need + rb0;
	const int *aln_of = a.aln_of_reg + rb0;
	const DevAln **list = a.rec_list + rb0;                     // this read's records / XA members: pointer lists in its region slots
	const DevAln **xa = a.xa_list + rb0;
	int n_rec = 0;
	if (!WRITE) {
		// mem_reg2sam's adjustments of the record copies (bwamem.c:1033-1041), applied once to the alignment array
		if (l == 0) {
			int mapq0 = 0;
			for (int k = 0; k < n; ++k) {
				if (!(need[k] & NEED_REC)) continue;
				DevAln *q = a.alns + aln_of[k];
				if (f[k].secondary >= 0) q->sub = -1;
				if (n_rec && f[k].secondary < 0) q->flag |= (opt.flag & BWAHIP_F_NO_MULTI) ? 0x10000 : 0x800;
				if (!(opt.flag & BWAHIP_F_KEEP_SUPP_MAPQ) && n_rec && !f[k].is_alt && q->mapq > (uint32_t)mapq0) q->mapq = (uint32_t)mapq0;
				if (n_rec == 0) mapq0 = (int)q->mapq;
				list[n_rec++] = q;
			}
		}
		n_rec = __shfl(n_rec, 0);
		__threadfence_block(); __syncthreads();
	} else {
		n_rec = a.rec_n[r];                                       // the list was built by the sizing pass
	}
	Tables t = { a.ctg_names, a.ctg_name_off, a.ctg_anno, a.ctg_anno_off, a.pool, a.rg_id, a.rg_len, opt.flag };
	ReadText s;
	s.name = a.names + a.name_off[r];
	s.comment = a.comments && a.comment_off[r + 1] > a.comment_off[r] ? a.comments + a.comment_off[r] : nullptr;
	s.seq = a.seq + a.off[r]; s.qual = a.qual && a.qual_off[r] >= 0 ? a.qual + a.qual_off[r] : nullptr; s.l_seq = (int)(a.off[r + 1] - a.off[r]);
	Emit e = { WRITE ? a.sam + a.sam_off[r] : nullptr, 0, l };
	if (n_rec == 0) {
		// unaligned read (bwamem.c:1043-1047): mem_reg2aln(..., 0) gives rid = pos = -1, flag 0x4, everything else 0
		__shared__ __attribute__((aligned(16))) DevAln s_un;
		__shared__ const DevAln *s_unp;
		if (l == 0) {
			DevAln u;
			memset(&u, 0, sizeof u);
			u.rid = -1; u.pos = -1; u.flag = 0x4;
			s_un = u; s_unp = &s_un;
		}
		__syncthreads();
		Fmt::record(e, t, s, 1, &s_unp, 0, nullptr, 0, nullptr);
	} else {
		int which = 0;
		for (int k = 0; k < n; ++k) {
			if (!(need[k] & NEED_REC)) continue;
			// XA members of record k: regions i (ascending) whose owner is k (bwamem_extra.c:141-160)
			int n_xa = 0;
			if (!(opt.flag & BWAHIP_F_ALL)) {
				if (l == 0) for (int i = 0; i < n; ++i) if ((need[i] & NEED_XA) && a.xa_owner[rb0 + i] == k) xa[n_xa++] = a.alns + aln_of[i];
				n_xa = __shfl(n_xa, 0);
				__threadfence_block(); __syncthreads();
			}
			Fmt::record(e, t, s, n_rec, list, which, nullptr, n_xa, xa);
			++which;
			__syncthreads();
		}
	}
	if (!WRITE && l == 0) { a.sam_len[r] = (int)e.pos; a.rec_n[r] = n_rec; }
}

// One end of a pair (mem_sam_pe's output part, bwamem_pair.c:366-385 and 397-418).  The decisions come from k_pair (PeRead), the
// mate's best hit h[!i] is attached to every record (mate fields, MC, TLEN).
template <bool WRITE, class Fmt>
__device__ __forceinline__ void records_pe(const FinLaunch &a)
{
	__shared__ __attribute__((aligned(16))) DevAln s_un[2];      // [0] unaligned record of this read, [1] unaligned mate (DevAln is padded to 80 bytes)
	__shared__ const DevAln *s_unp;
	const int r = (int)blockIdx.x + a.read_lo, l = (int)(threadIdx.x & 63), rm = r ^ 1, end = r & 1;
	const DevOpt &opt = a.opt;
	const int n = a.freg_n[r];
	const int64_t rb0 = a.reg_base[r], rbm = a.reg_base[rm];
	const FinReg *f = a.fregs + rb0;
	const uint8_t *need = a.need + rb0;
	const int *aln_of = a.aln_of_reg + rb0;
	const DevAln **list = a.rec_list + rb0;
	const DevAln **xa = a.xa_list + rb0;
	const PeRead pr = a.pe_read[r], prm = a.pe_read[rm];
	if (l == 0) {
		DevAln u;
		memset(&u, 0, sizeof u);
		u.rid = -1; u.pos = -1; u.flag = 0x4;
		s_un[0] = u; s_un[1] = u; s_unp = &s_un[0];
	}
	__syncthreads();
	const DevAln *m = prm.h_reg >= 0 ? a.alns + a.aln_of_reg[rbm + prm.h_reg] : &s_un[1];
	const DevAln *h = pr.h_reg >= 0 ? a.alns + aln_of[pr.h_reg] : &s_un[0];
	int extra = pr.extra_flag;
	if (pr.mode == 0) {
		// proper-pair bit of the unpaired path (bwamem_pair.c:406-411): the two best hits on one contig within the insert range
		if (!(opt.flag & BWAHIP_F_NOPAIRING) && h->rid == m->rid && h->rid >= 0) {
			int64_t dist;
			const int64_t b_own = f[0].rb, b_mate = a.fregs[rbm].rb;
			const int d = end == 0 ? infer_dir(a.ix.l_pac, b_own, b_mate, &dist) : infer_dir(a.ix.l_pac, b_mate, b_own, &dist);
			if (!a.pes[d].failed && dist >= a.pes[d].low && dist <= a.pes[d].high) extra |= 2;
		}
		extra |= end == 0 ? 0x40 : 0x80;
	}
	int n_rec = 0;
	if (!WRITE) {
		if (l == 0) {
			if (pr.mode == 1) {                                   // bwamem_pair.c:366-377: h[i], then the ALT hit as supplementary
				DevAln *q = a.alns + aln_of[pr.h_reg];
				q->mapq = (uint32_t)pr.mapq & 0xff;
				q->flag |= (0x40 << end) | extra;
				list[n_rec++] = q;
				if (pr.alt_reg >= 0) {
					DevAln *g = a.alns + aln_of[pr.alt_reg];
					g->flag |= 0x800 | (0x40 << end) | extra;
					list[n_rec++] = g;
				}
			} else {                                              // mem_reg2sam with extra_flag and the mate (bwamem.c:1033-1041)
				int mapq0 = 0;
				for (int k = 0; k < n; ++k) {
					if (!(need[k] & NEED_REC)) continue;
					DevAln *q = a.alns + aln_of[k];
					q->flag |= extra;
					if (f[k].secondary >= 0) q->sub = -1;
					if (n_rec && f[k].secondary < 0) q->flag |= (opt.flag & BWAHIP_F_NO_MULTI) ? 0x10000 : 0x800;
					if (!(opt.flag & BWAHIP_F_KEEP_SUPP_MAPQ) && n_rec && !f[k].is_alt && q->mapq > (uint32_t)mapq0) q->mapq = (uint32_t)mapq0;
					if (n_rec == 0) mapq0 = (int)q->mapq;
					list[n_rec++] = q;
				}
			}
		}
		n_rec = __shfl(n_rec, 0);
		__threadfence_block(); __syncthreads();
	} else n_rec = a.rec_n[r];
	Tables t = { a.ctg_names, a.ctg_name_off, a.ctg_anno, a.ctg_anno_off, a.pool, a.rg_id, a.rg_len, opt.flag };
	ReadText s;
	s.name = a.names + a.name_off[r];
	s.comment = a.comments && a.comment_off[r + 1] > a.comment_off[r] ? a.comments + a.comment_off[r] : nullptr;
	s.seq = a.seq + a.off[r]; s.qual = a.qual && a.qual_off[r] >= 0 ? a.qual + a.qual_off[r] : nullptr; s.l_seq = (int)(a.off[r + 1] - a.off[r]);
	Emit e = { WRITE ? a.sam + a.sam_off[r] : nullptr, 0, l };
	if (n_rec == 0) {
		if (l == 0) s_un[0].flag = 0x4 | extra;                     // t.flag |= extra_flag (bwamem.c:1045)
		__syncthreads();
		Fmt::record(e, t, s, 1, &s_unp, 0, m, 0, nullptr);
	} else {
		for (int which = 0; which < n_rec; ++which) {
			// the region this record came from: its XA members are the regions it owns
			int k_reg = -1, n_xa = 0;
			if (pr.mode == 1) k_reg = which == 0 ? pr.h_reg : pr.alt_reg;
			else { int c = 0; for (int k = 0; k < n; ++k) if (need[k] & NEED_REC) { if (c == which) { k_reg = k; break; } ++c; } }
			if (!(opt.flag & BWAHIP_F_ALL)) {
				if (l == 0) for (int i = 0; i < n; ++i) if ((need[i] & NEED_XA) && a.xa_owner[rb0 + i] == k_reg) xa[n_xa++] = a.alns + aln_of[i];
				n_xa = __shfl(n_xa, 0);
				__threadfence_block(); __syncthreads();
			}
			Fmt::record(e, t, s, n_rec, list, which, m, n_xa, xa);
			__syncthreads();
		}
	}
	if (!WRITE && l == 0) { a.sam_len[r] = (int)e.pos; a.rec_n[r] = n_rec; }
}

} // namespace samdev
