// K9g -- duplicate marking of device-merged, coordinate-sorted BAM, before the deflate.  The rule is in include/bwahip.h.  Three parts:
//
//   per batch      k_dup_desc: one descriptor per template (the two end words, the score, the kind) from the records in input order
//                  (c->bs.raw with the per-read offsets), where the mates are still neighbours; k_tmpl_fill / k_tmpl_sorted: per record the
//                  index of its template, carried through the sort's final permutation.  Queued by bam_sort_batch for OutForm::BamSortedDup only;
//   decision       markdup_decide over the descriptors of all runs in run order (template index = input order).  Pairs: the ordinals
//                  sorted by end[1], then end[0], then "is a pair" (three calls of the stable radix sort of k_bamsort.hip), neighbours
//                  compared for segment heads, an exclusive scan of the heads numbers the segments, a 64-bit atomicMax of
//                  score << 32 | ~template per segment finds the survivor.  Then the same over the end-word table (entry 2t = the
//                  fragment's or the pair's first end word, 2t + 1 = a pair's second): per segment "a pair is present" (every writer writes
//                  1) and the best fragment.  Maxima and ORs: the result does not depend on the order in which the atomics land;
//   marking        k_md_mark: one thread per record of a run ORs 0x04 into the byte at record offset 19 (flag 0x400) when the record's
//                  template is a duplicate and 0x4 is clear; a plain byte store, each thread its own record.
//
// No kernel here uses LDS.  k_dup_desc gives a template 16 lanes: all of them follow the block_size chain and the primaries' CIGARs (the
// same addresses in all 16 lanes: one request), and share the quality bytes -- 4 bytes per lane and step at any alignment, so one
// step of a template reads 64 consecutive bytes, where one lane per template would touch a different cache line in every lane.
#include "ctx_internal.h"

namespace {

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }   // records start at any byte
__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

__host__ __device__ __forceinline__ uint64_t end_word(int32_t refID, int32_t u5, bool reverse)
{
	return (uint64_t)(int64_t)refID << 33 | (uint64_t)((int64_t)u5 + (1ll << 31)) << 1 | (reverse ? 1u : 0u);
}

// The records of one read, raw[o .. e): the chain is followed and every record's fields are checked against its length (*err otherwise,
// and the read counts as unmapped); the first primary record, when mapped, gives its end word, and this lane's share of its quality
// bytes >= 15 is added to *part (lane l of 16).  Nothing outside [o, e) is read.
__device__ bool read_primary(const uint8_t *raw, int64_t o, const int64_t e, int l, int *err, uint64_t *word, uint32_t *part)
{
	int64_t prim = -1;
	bool bad = false;
	while (o + 36 <= e) {
		const int32_t bs = (int32_t)ld_u32(raw + o);
		if (bs < 32 || o + 4 + bs > e) break;
		const int64_t l_name = raw[o + 12], n_cig = ld_u16(raw + o + 16), l_seq = (int32_t)ld_u32(raw + o + 20);
		if (l_seq < 0 || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) bad = true;
		else if (prim < 0 && !(ld_u16(raw + o + 18) & 0x900)) prim = o;
		o += 4 + (int64_t)bs;
	}
	if (o != e || bad) { *err = 1; return false; }                // every writer writes 1
	if (prim < 0) return false;
	const uint32_t flag = ld_u16(raw + prim + 18);
	if (flag & 0x4) return false;
	const int l_name = raw[prim + 12], n_cig = (int)ld_u16(raw + prim + 16), l_seq = (int32_t)ld_u32(raw + prim + 20);
	const uint8_t *cig = raw + prim + 36 + l_name;
	int64_t lead = 0, trail = 0, rlen = 0;
	bool seen = false;                                            // an operation that is neither S nor H
	for (int k = 0; k < n_cig; ++k) {
		const uint32_t v = ld_u32(cig + 4 * k), op = v & 15, len = v >> 4;
		if (op == 4 || op == 5) { if (!seen) lead += len; trail += len; }
		else { seen = true; trail = 0; }
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += len;
	}
	const bool rev = (flag & 0x10) != 0;
	const int64_t pos = (int32_t)ld_u32(raw + prim + 8);
	const int64_t u5 = rev ? pos + (rlen > 1 ? rlen : 1) - 1 + trail : pos - lead;
	*word = end_word((int32_t)ld_u32(raw + prim + 4), (int32_t)u5, rev);
	const uint8_t *q = cig + 4 * n_cig + (l_seq + 1) / 2;
	if (l_seq > 0 && q[0] != 0xff) {
		uint32_t s = 0;
		const int body = l_seq & ~3;
		for (int k = 4 * l; k < body; k += 64) {
			const uint32_t v = ld_u32(q + k);
#pragma unroll
			for (int b = 0; b < 4; ++b) { const uint32_t x = v >> (8 * b) & 255u; s += x >= 15 ? x : 0; }
		}
		for (int k = body + l; k < l_seq; k += 16) { const uint32_t x = q[k]; s += x >= 15 ? x : 0; }
		*part += s;
	}
	return true;
}

// 16 lanes per template; template t = read t, or reads 2t and 2t + 1
__global__ __launch_bounds__(256) void k_dup_desc(const uint8_t *raw, const int64_t *off, int n_tmpl, int paired, bwahip_dup_desc_t *desc, int *err)
{
	const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	const int l = threadIdx.x & 15;
	if (t >= n_tmpl) return;                                       // the 16 lanes of a template leave together
	uint64_t w[2] = { 0, 0 };
	uint32_t part = 0;
	int kind = 0;
	const int64_t r0 = paired ? 2 * t : t;
	for (int k = 0; k <= (paired ? 1 : 0); ++k) {
		uint64_t x = 0;
		if (read_primary(raw, off[r0 + k], off[r0 + k + 1], l, err, &x, &part)) w[kind++] = x;
	}
	for (int d = 8; d; d >>= 1) part += __shfl_xor(part, d);      // within the 16 lanes, which took the same branches
	if (l) return;
	bwahip_dup_desc_t out;
	out.end[0] = kind == 2 && w[1] < w[0] ? w[1] : w[0];
	out.end[1] = kind == 2 ? (w[1] < w[0] ? w[0] : w[1]) : 0;
	out.score = kind ? part : 0; out.kind = (uint32_t)kind;
	if (!kind) out.end[0] = 0;
	desc[t] = out;
}

// thread = read: the template of each of its records, in input order
__global__ __launch_bounds__(256) void k_tmpl_fill(const int64_t *rec_base, int n, int paired, uint32_t *tmpl)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t t = (uint32_t)(paired ? i >> 1 : i);
	for (int64_t r = rec_base[i]; r < rec_base[i + 1]; ++r) tmpl[r] = t;
}

__global__ __launch_bounds__(256) void k_tmpl_sorted(const unsigned *idx, const uint32_t *tmpl, int n, uint32_t *out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = tmpl[idx[i]];
}

// ---- decision ---------------------------------------------------------------------------------------------------------------------
// An entry of a stage: mode 0 (pairs) entry e = template e, valid when it is a pair, key words end[0], end[1]; mode 1 (end-word table)
// entry e = end word e & 1 of template e >> 1, valid when the template has that many, one key word.
struct Entry { uint32_t t; bool valid, of_pair; uint64_t key[2]; uint32_t score; };
__device__ __forceinline__ Entry entry_of(const bwahip_dup_desc_t *desc, uint32_t e, int mode)
{
	Entry x;
	x.t = mode ? e >> 1 : e;
	const bwahip_dup_desc_t d = desc[x.t];
	x.of_pair = d.kind == 2; x.score = d.score;
	if (mode) { x.valid = (e & 1) ? d.kind == 2 : d.kind >= 1; x.key[0] = d.end[e & 1]; x.key[1] = 0; }
	else { x.valid = d.kind == 2; x.key[0] = d.end[0]; x.key[1] = d.end[1]; }
	return x;
}

// the sort key of pass `which` for the entries in their present order: 0 / 1 a key word, 2 validity (valid entries first)
__global__ __launch_bounds__(256) void k_md_keys(const bwahip_dup_desc_t *desc, const unsigned *idx, int n, int mode, int which, uint64_t *keys)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const Entry x = entry_of(desc, idx[i], mode);
	keys[i] = which == 2 ? (x.valid ? 0 : 1) : x.key[which];
}

__global__ __launch_bounds__(256) void k_md_heads(const bwahip_dup_desc_t *desc, const unsigned *idx, int n, int mode, int *head)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const Entry x = entry_of(desc, idx[i], mode);
	int h = 0;
	if (x.valid) {
		h = 1;
		if (i) { const Entry p = entry_of(desc, idx[i - 1], mode); h = !(p.valid && p.key[0] == x.key[0] && p.key[1] == x.key[1]); }
	}
	head[i] = h;
}

// seg: the exclusive scan of head; the segment of a valid entry is seg + head - 1 (a valid entry that is no head has a head before it)
__global__ __launch_bounds__(256) void k_md_best(const bwahip_dup_desc_t *desc, const unsigned *idx, int n, int mode, const int *head, const int64_t *seg,
                                                 unsigned long long *best, uint8_t *pair_here)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const Entry x = entry_of(desc, idx[i], mode);
	if (!x.valid) return;
	const int64_t s = seg[i] + head[i] - 1;
	if (mode && x.of_pair) pair_here[s] = 1;                       // every writer writes 1
	else atomicMax(&best[s], (unsigned long long)x.score << 32 | (0xffffffffu - x.t));   // the highest score, then the earliest template: a maximum, the same in any order
}

// mode 0 decides the pairs, mode 1 the fragments: every template is written by at most one thread
__global__ __launch_bounds__(256) void k_md_verdict(const bwahip_dup_desc_t *desc, const unsigned *idx, int n, int mode, const int *head, const int64_t *seg,
                                                    const unsigned long long *best, const uint8_t *pair_here, uint8_t *dup)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const Entry x = entry_of(desc, idx[i], mode);
	if (!x.valid || (mode && x.of_pair)) return;
	const int64_t s = seg[i] + head[i] - 1;
	const bool kept = (uint32_t)best[s] == 0xffffffffu - x.t && !(mode && pair_here[s]);
	dup[x.t] = kept ? 0 : 1;
}

// cnt[k] templates of kind k, cnt[3 + k] duplicates among them (sums: the same in any order)
__global__ __launch_bounds__(256) void k_md_stats(const bwahip_dup_desc_t *desc, const uint8_t *dup, int n, unsigned long long *cnt)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const int kind = i < n ? (int)desc[i].kind : -1;
	const bool d = i < n && dup[i];
	for (int k = 0; k < 3; ++k) {
		const unsigned long long a = __ballot(kind == k), b = __ballot(kind == k && d);
		if ((threadIdx.x & 63) == 0) { if (a) atomicAdd(&cnt[k], (unsigned long long)__popcll(a)); if (b) atomicAdd(&cnt[3 + k], (unsigned long long)__popcll(b)); }
	}
}

// thread = record of one run.  dup: the verdicts of this run's templates.  err: an offset or a template index outside the run (never
// expected: add_dup checked the host's, the batch kernels produced the device's); such a record is left alone.
__global__ __launch_bounds__(256) void k_md_mark(uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, const uint32_t *tmpl, int64_t n_tmpl, const uint8_t *dup,
                                                 unsigned long long *marked, int *err)
{
	const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
	bool mark = false;
	if (r < n_rec) {
		const int64_t o = off[r];
		const uint32_t t = tmpl[r];
		if (o < 0 || o + 36 > len || off[r + 1] < o + 36 || t >= n_tmpl) *err = 1;
		else if (dup[t] && !(rec[o + 18] & 0x4)) { rec[o + 19] |= 0x04; mark = true; }   // flag 0x400: bit 2 of the flag's high byte
	}
	const unsigned long long b = __ballot(mark);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(marked, (unsigned long long)__popcll(b));
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }
inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// One stage of the decision over n entries: the order into c->bs.idx, heads, segments, best, verdict.  The sorts are stable and least
// significant key first, so the final order is (validity, key[0], key[1], entry).
int decide_stage(MarkdupStage *s, bwahip_ctx *c, const bwahip_dup_desc_t *desc, int n, int mode)
{
	BamSort &bs = c->bs;
	int rc, cur = 0;
	if ((rc = bam_sort_iota(bs.idx[0].as<unsigned>(), n, c->stream))) return rc;
	const int passes[3] = { 1, 0, 2 };
	for (int p = mode ? 1 : 0; p < 3; ++p) {                       // the table has one key word
		if (cur) HIP_TRY(hipMemcpyAsync(bs.idx[0].p, bs.idx[1].p, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));   // the sort reads set 0
		hipLaunchKernelGGL(k_md_keys, grid_of(n), dim3(256), 0, c->stream, desc, bs.idx[0].as<unsigned>(), n, mode, passes[p], bs.keys[0].as<uint64_t>());
		if ((rc = launched()) || (rc = bam_sort_radix(c, n, passes[p] == 2 ? 8 : 64, &cur))) return rc;
	}
	const unsigned *idx = bs.idx[cur].as<unsigned>();
	hipLaunchKernelGGL(k_md_heads, grid_of(n), dim3(256), 0, c->stream, desc, idx, n, mode, s->head.as<int>());
	if ((rc = launched()) || (rc = launch_scan(s->head.as<int>(), s->seg.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	HIP_TRY(hipMemsetAsync(s->best.p, 0, (size_t)n * 8, c->stream));
	HIP_TRY(hipMemsetAsync(s->pair_here.p, 0, (size_t)n, c->stream));
	hipLaunchKernelGGL(k_md_best, grid_of(n), dim3(256), 0, c->stream, desc, idx, n, mode, s->head.as<int>(), s->seg.as<int64_t>(), s->best.as<unsigned long long>(), s->pair_here.as<uint8_t>());
	if ((rc = launched())) return rc;
	hipLaunchKernelGGL(k_md_verdict, grid_of(n), dim3(256), 0, c->stream, desc, idx, n, mode, s->head.as<int>(), s->seg.as<int64_t>(), s->best.as<unsigned long long>(), s->pair_here.as<uint8_t>(),
	                   s->dup.as<uint8_t>());
	return launched();
}

} // namespace

extern "C" int64_t bwahip_bam_devmerge_markdup_hbm_need(int64_t n_records, int64_t n_templates)
{
	if (n_records < 0 || n_templates < 0) return -1;
	const int64_t runs = 4 * n_records + 24 * n_templates;
	const int64_t work = 115 * n_templates + 4096;
	return runs + work + work / 8;
}

// s->desc holds n_tmpl descriptors in input order; the verdicts into s->dup (one byte per template).  Queued on c->stream (the sorts
// await a small read-back each); the context's sort buffers are used.
int markdup_decide(MarkdupStage *s, bwahip_ctx *c, int64_t n_tmpl)
{
	if (!s || !c || n_tmpl < 0) return BWAHIP_EINVAL;
	if (n_tmpl > 0x3fffffffll) return BWAHIP_ECAPACITY;            // the table has two entries per template and the sort takes an int
	if (!n_tmpl) return 0;
	const int n = (int)n_tmpl;
	const size_t N = 2 * (size_t)n;
	BamSort &bs = c->bs;
	int rc;
	if ((rc = bs.keys[0].ensure(N * 8)) || (rc = bs.keys[1].ensure(N * 8)) || (rc = bs.idx[0].ensure(N * 4)) || (rc = bs.idx[1].ensure(N * 4)) ||
	    (rc = s->head.ensure(N * 4)) || (rc = s->seg.ensure((N + 1) * 8)) || (rc = s->best.ensure(N * 8)) || (rc = s->pair_here.ensure(N)) || (rc = s->dup.ensure((size_t)n))) return rc;
	HIP_TRY(hipMemsetAsync(s->dup.p, 0, (size_t)n, c->stream));
	const bwahip_dup_desc_t *desc = s->desc.as<bwahip_dup_desc_t>();
	if ((rc = decide_stage(s, c, desc, n, 0)) || (rc = decide_stage(s, c, desc, 2 * n, 1))) return rc;
	return 0;
}

// cnt[0..5] of k_md_stats, cnt[6] records marked so far, cnt[7] (as int) the marking pass's error: zeroed here
int markdup_counters_reset(MarkdupStage *s, bwahip_ctx *c)
{
	int rc = s->cnt.ensure(64);
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(s->cnt.p, 0, 64, c->stream));
	return 0;
}

int markdup_count(MarkdupStage *s, bwahip_ctx *c, int64_t n_tmpl)
{
	if (!n_tmpl) return 0;
	hipLaunchKernelGGL(k_md_stats, grid_of(n_tmpl), dim3(256), 0, c->stream, s->desc.as<bwahip_dup_desc_t>(), s->dup.as<uint8_t>(), (int)n_tmpl, s->cnt.as<unsigned long long>());
	return launched();
}

int markdup_mark_run(MarkdupStage *s, bwahip_ctx *c, uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, const uint32_t *tmpl, int64_t first_tmpl, int64_t n_tmpl,
                     unsigned long long *marked_to)
{
	if (!n_rec) return 0;
	hipLaunchKernelGGL(k_md_mark, grid_of(n_rec), dim3(256), 0, c->stream, rec, off, n_rec, len, tmpl, n_tmpl, s->dup.as<uint8_t>() + first_tmpl,
	                   marked_to ? marked_to : s->cnt.as<unsigned long long>() + 6, (int*)(s->cnt.as<unsigned long long>() + 7));
	return launched();
}

// ---- per batch (bam_sort_batch) ----------------------------------------------------------------------------------------------------
// after k_rec_fill: the descriptors of the batch's templates into c->out->d_desc, the records' templates in input order into c->bs.tmpl
int dup_batch_desc(bwahip_ctx *c, int n_reads, bool paired, int64_t n_rec)
{
	BatchOut &o = *c->out;
	const int n_tmpl = paired ? n_reads / 2 : n_reads;
	o.n_tmpl = n_tmpl;
	int rc;
	if ((rc = o.d_desc.ensure((size_t)(n_tmpl ? n_tmpl : 1) * sizeof(bwahip_dup_desc_t) + 16)) || (rc = c->bs.tmpl.ensure((size_t)(n_rec ? n_rec : 1) * 4)) ||
	    (rc = o.d_tmpl.ensure((size_t)(n_rec ? n_rec : 1) * 4))) return rc;
	int *err = (int*)(o.d_desc.as<bwahip_dup_desc_t>() + n_tmpl);  // behind the descriptors
	HIP_TRY(hipMemsetAsync(err, 0, 4, c->stream));
	if (!n_tmpl) return 0;
	hipLaunchKernelGGL(k_dup_desc, grid_of((int64_t)n_tmpl * 16), dim3(256), 0, c->stream, c->bs.raw.as<uint8_t>(), o.d_sam_off.as<int64_t>(), n_tmpl, paired ? 1 : 0,
	                   o.d_desc.as<bwahip_dup_desc_t>(), err);
	if ((rc = launched())) return rc;
	hipLaunchKernelGGL(k_tmpl_fill, grid_of(n_reads), dim3(256), 0, c->stream, c->bs.rec_base.as<int64_t>(), n_reads, paired ? 1 : 0, c->bs.tmpl.as<uint32_t>());
	return launched();
}

// after the radix sort: the templates in sorted order into c->out->d_tmpl; the descriptor kernel's verdict on the records is awaited
int dup_batch_tmpl(bwahip_ctx *c, int n_rec, const unsigned *idx)
{
	BatchOut &o = *c->out;
	int rc;
	if (n_rec > 0) {
		hipLaunchKernelGGL(k_tmpl_sorted, grid_of(n_rec), dim3(256), 0, c->stream, idx, c->bs.tmpl.as<uint32_t>(), n_rec, o.d_tmpl.as<uint32_t>());
		if ((rc = launched())) return rc;
	}
	int err = 0;
	HIP_TRY(hipMemcpyAsync(&err, o.d_desc.as<bwahip_dup_desc_t>() + o.n_tmpl, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (err) { fprintf(stderr, "[bwahip] duplicate marking: a record of the batch is shorter than its fields\n"); return BWAHIP_EINTERNAL; }
	return 0;
}

// ---- known answers -----------------------------------------------------------------------------------------------------------------
extern "C" int bwahip_kat_dup_desc(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_reads, int paired, bwahip_dup_desc_t *desc_out)
{
	if (!c || n_reads < 0 || n_reads > 0x7fffffffll || (n_reads && (!rec || !off || !desc_out)) || (paired && (n_reads & 1))) return BWAHIP_EINVAL;
	if (!n_reads) return 0;
	if (off[0] < 0) return BWAHIP_EINVAL;
	for (int64_t i = 0; i < n_reads; ++i) if (off[i + 1] < off[i]) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	const int64_t n_tmpl = paired ? n_reads / 2 : n_reads, len = off[n_reads];
	DevBuf d_rec, d_off, d_desc;
	Event ev[2];
	int rc, err = 0;
	if (!(rc = ev[0].make()) && !(rc = ev[1].make()) && !(rc = d_rec.ensure((size_t)len + 1)) && !(rc = d_off.ensure((size_t)(n_reads + 1) * 8)) && !(rc = d_desc.ensure((size_t)n_tmpl * sizeof(bwahip_dup_desc_t) + 16))) {
		int *d_err = (int*)(d_desc.as<bwahip_dup_desc_t>() + n_tmpl);
		hipError_t e = len ? hipMemcpyAsync(d_rec.p, rec, (size_t)len, hipMemcpyHostToDevice, c->stream) : hipSuccess;
		if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, c->stream);
		if (e == hipSuccess) {
			(void)hipEventRecord(ev[0], c->stream);
			hipLaunchKernelGGL(k_dup_desc, grid_of(n_tmpl * 16), dim3(256), 0, c->stream, d_rec.as<uint8_t>(), d_off.as<int64_t>(), (int)n_tmpl, paired ? 1 : 0, d_desc.as<bwahip_dup_desc_t>(), d_err);
			rc = launched();
			(void)hipEventRecord(ev[1], c->stream);
		}
		if (e == hipSuccess && !rc) e = hipMemcpyAsync(desc_out, d_desc.p, (size_t)n_tmpl * sizeof(bwahip_dup_desc_t), hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess && !rc) e = hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = hipStreamSynchronize(c->stream);      // nothing of the buffers is in use when they go
		if (!rc && (e != hipSuccess || e2 != hipSuccess)) rc = BWAHIP_ENODEV;
		if (rc || hipEventElapsedTime(&c->dup_desc_ms, ev[0], ev[1]) != hipSuccess) c->dup_desc_ms = 0;
	}
	return rc ? rc : err ? BWAHIP_EINVAL : 0;
}

extern "C" float bwahip_kat_dup_desc_ms(bwahip_ctx *c) { return c ? c->dup_desc_ms : 0; }

extern "C" int bwahip_kat_markdup(bwahip_ctx *c, const bwahip_dup_desc_t *desc, int64_t n_tmpl, uint8_t *dup_out)
{
	if (!c || n_tmpl < 0 || (n_tmpl && (!desc || !dup_out))) return BWAHIP_EINVAL;
	if (!n_tmpl) return 0;
	for (int64_t i = 0; i < n_tmpl; ++i) if (desc[i].kind > 2) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	MarkdupStage s;
	int rc = s.desc.ensure((size_t)n_tmpl * sizeof(bwahip_dup_desc_t));
	if (!rc && hipMemcpyAsync(s.desc.p, desc, (size_t)n_tmpl * sizeof(bwahip_dup_desc_t), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = BWAHIP_ENODEV;
	if (!rc) rc = markdup_decide(&s, c, n_tmpl);
	if (!rc && hipMemcpyAsync(dup_out, s.dup.p, (size_t)n_tmpl, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = BWAHIP_ENODEV;
	if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = BWAHIP_ENODEV;
	return rc;
}
