// K9c -- the batch's BAM records in coordinate order, on the GPU.  Input: the records k_bam.hip wrote in input order (c->bs.raw) and the
// per-read offsets.  Three stages, all deterministic (no output position depends on the order in which atomics land):
//
//   record table   a read owns one or more records: k_rec_count follows the block_size chain of every read, an exclusive scan gives
//                  every read its first ordinal, k_rec_fill writes per record its key (bam_sort_key.h), byte offset and length;
//   radix sort     stable LSD sort of (key, ordinal), 8 bits per pass, only the passes that cover key bits which differ between the
//                  keys (k_key_bits: OR and AND over all keys).  A pass = k_rs_hist (digit counts per workgroup tile), an exclusive scan
//                  over (digit, workgroup), k_rs_scatter (rank inside the tile by wavefront match + per-wavefront counters in LDS);
//   gather         lengths in sorted order, an exclusive scan to the output offsets, k_gather_copy moves every record to its place.
//
// The tile of a workgroup is RS_TILE consecutive items; wavefront w owns items [w * 64 * RS_ROUNDS, (w + 1) * 64 * RS_ROUNDS) of it and
// takes them 64 at a time, so "earlier in the input" is (workgroup, wavefront, round, lane) in that order -- the order the ranks follow.
#include "ctx_internal.h"
#include "bam_sort_key.h"

namespace {

constexpr int RS_T = 256, RS_WAVES = RS_T / 64, RS_ROUNDS = 16, RS_TILE = RS_T * RS_ROUNDS;

typedef __attribute__((address_space(3))) unsigned lds_u32;   // a pointer into LDS that says so: the counter update below is a ds_ instruction by type

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }   // records start at any byte
__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// ---- record table ---------------------------------------------------------------------------------------------------------------
// err: a chain that does not end exactly at the read's end (never expected: the write pass produced it)
__global__ __launch_bounds__(256) void k_rec_count(const uint8_t *raw, const int64_t *off, int n, int *cnt, int *err)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	int64_t o = off[i];
	const int64_t e = off[i + 1];
	int k = 0;
	while (o + 36 <= e) {
		const int32_t bs = (int32_t)ld_u32(raw + o);
		if (bs < 32 || o + 4 + bs > e) break;
		o += 4 + (int64_t)bs; ++k;
	}
	if (o != e) *err = 1;
	cnt[i] = k;
}

__global__ __launch_bounds__(256) void k_rec_fill(const uint8_t *raw, const int64_t *off, const int64_t *rec_base, int n, int32_t n_seqs, int pos_bits,
                                                  uint64_t *keys, unsigned *idx, int64_t *rec_off, int *rec_len)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	int64_t o = off[i];
	const int64_t r1 = rec_base[i + 1];
	for (int64_t r = rec_base[i]; r < r1; ++r) {
		const int32_t bs = (int32_t)ld_u32(raw + o);
		keys[r] = bam_key_pack(n_seqs, pos_bits, (int32_t)ld_u32(raw + o + 4), (int32_t)ld_u32(raw + o + 8), (ld_u16(raw + o + 18) & 0x10) != 0);
		idx[r] = (unsigned)r; rec_off[r] = o; rec_len[r] = 4 + bs;
		o += 4 + (int64_t)bs;
	}
}

__global__ __launch_bounds__(256) void k_iota(unsigned *idx, int n)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) idx[i] = (unsigned)i;
}

// ---- radix sort -------------------------------------------------------------------------------------------------------------------
// bits[0] |= every key, bits[1] &= every key: a bit that is equal in both is the same in all keys (the results of OR / AND do not depend
// on the order of the atomics)
__global__ __launch_bounds__(256) void k_key_bits(const uint64_t *keys, int n, unsigned long long *bits)
{
	unsigned long long o = 0, a = ~0ull;
	for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { const unsigned long long k = keys[i]; o |= k; a &= k; }
	for (int d = 32; d; d >>= 1) { o |= __shfl_xor(o, d); a &= __shfl_xor(a, d); }
	if ((threadIdx.x & 63) == 0) { atomicOr(&bits[0], o); atomicAnd(&bits[1], a); }
}

// hist[digit * n_wg + workgroup] = items of the workgroup's tile with that digit (sums: the same in any order)
__global__ __launch_bounds__(RS_T) void k_rs_hist(const uint64_t *keys, int n, int shift, int *hist, int n_wg)
{
	__shared__ unsigned h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const int64_t base = (int64_t)blockIdx.x * RS_TILE;
#pragma unroll 4
	for (int r = 0; r < RS_ROUNDS; ++r) {
		const int64_t i = base + r * RS_T + threadIdx.x;
		if (i < n) __hip_atomic_fetch_add((lds_u32*)h + ((unsigned)(keys[i] >> shift) & 255u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	}
	__syncthreads();
	hist[(size_t)threadIdx.x * n_wg + blockIdx.x] = (int)h[threadIdx.x];
}

// base[digit * n_wg + workgroup]: the exclusive scan of hist = where the workgroup's first item of that digit goes
__global__ __launch_bounds__(RS_T) void k_rs_scatter(const uint64_t *keys_in, const unsigned *idx_in, uint64_t *keys_out, unsigned *idx_out, int n, int shift,
                                                     const int64_t *base, int n_wg)
{
	__shared__ unsigned cnt[RS_WAVES * 256];     // per wavefront: items of each digit seen so far; afterwards: items of the digit in earlier wavefronts
	__shared__ long long gbase[256];
	const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
#pragma unroll
	for (int k = 0; k < RS_WAVES; ++k) cnt[k * 256 + tid] = 0;
	__syncthreads();
	const int64_t wave_base = (int64_t)blockIdx.x * RS_TILE + (int64_t)w * 64 * RS_ROUNDS;
	const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
	uint64_t key[RS_ROUNDS];
	unsigned ord[RS_ROUNDS], loc[RS_ROUNDS];
#pragma unroll
	for (int r = 0; r < RS_ROUNDS; ++r) {
		const int64_t i = wave_base + r * 64 + lane;
		const bool valid = i < n;
		key[r] = valid ? keys_in[i] : 0;
		ord[r] = valid ? idx_in[i] : 0;
		const unsigned d = (unsigned)(key[r] >> shift) & 255u;
		// the lanes of this round that hold the same digit
		unsigned long long same = __ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; ++b) {
			const bool bit = (d >> b & 1u) != 0;
			const unsigned long long bal = __ballot(bit);
			same &= bit ? bal : ~bal;
		}
		if (!valid) same = 0;
		const int leader = same ? __ffsll((long long)same) - 1 : lane;
		unsigned before = 0;
		if (valid && lane == leader) { before = cnt[w * 256 + d]; cnt[w * 256 + d] = before + (unsigned)__popcll(same); }   // one lane per digit: no atomics
		before = __shfl(before, leader);
		loc[r] = before + (unsigned)__popcll(same & below);
		__builtin_amdgcn_wave_barrier();         // the next round's read of a counter comes after this round's write
	}
	__syncthreads();
	{                                            // thread = digit: counts of the wavefronts -> exclusive prefix over the wavefronts
		unsigned run = 0;
#pragma unroll
		for (int k = 0; k < RS_WAVES; ++k) { const unsigned t = cnt[k * 256 + tid]; cnt[k * 256 + tid] = run; run += t; }
		gbase[tid] = base[(size_t)tid * n_wg + blockIdx.x];
	}
	__syncthreads();
#pragma unroll
	for (int r = 0; r < RS_ROUNDS; ++r) {
		const int64_t i = wave_base + r * 64 + lane;
		if (i >= n) continue;
		const unsigned d = (unsigned)(key[r] >> shift) & 255u;
		// first place of the digit for this workgroup + items of the digit in earlier wavefronts + in earlier rounds and lanes of this one:
		// below the workgroup's count of the digit in k_rs_hist (same keys, same tile), so below the next base and below n
		const int64_t p = gbase[d] + cnt[w * 256 + d] + loc[r];
		keys_out[p] = key[r]; idx_out[p] = ord[r];
	}
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_len(const unsigned *idx, const int *rec_len, int n, int *len_sorted)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) len_sorted[i] = rec_len[idx[i]];
}

// 16 lanes per record: bytes up to the first 16-byte boundary of the destination, then 16 bytes per lane and step (the source is read
// unaligned), then the bytes that are left.  A record of 300 bytes takes two steps.
__global__ __launch_bounds__(256) void k_gather_copy(const uint8_t *raw, const unsigned *idx, const int64_t *rec_off, const int64_t *out_off, int n, uint8_t *out)
{
	const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	const int l = threadIdx.x & 15;
	if (g >= n) return;
	const uint8_t *src = raw + rec_off[idx[g]];
	const int64_t o = out_off[g];
	const int len = (int)(out_off[g + 1] - o);
	uint8_t *dst = out + o;
	int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
	if (head > len) head = len;
	if (l < head) dst[l] = src[l];
	const int body = (len - head) >> 4;
	for (int k = l; k < body; k += 16) {
		uint4 v;
		__builtin_memcpy(&v, src + head + 16 * k, 16);
		*reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
	}
	for (int k = head + 16 * body + l; k < len; k += 16) dst[k] = src[k];
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }

} // namespace

int bam_sort_tile() { return RS_TILE; }

int bam_sort_iota(unsigned *idx, int n, hipStream_t st)
{
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, st, idx, n);
	return launched();
}

int bam_sort_radix(bwahip_ctx *c, int n, int key_bits, int *which)
{
	BamSort &s = c->bs;
	*which = 0; s.n_passes = 0;
	if (n <= 1) return 0;                                          // nothing to order: nothing is launched
	if (key_bits < 1) key_bits = 1;
	if (key_bits > 64) key_bits = 64;
	const int n_wg = (n + RS_TILE - 1) / RS_TILE;
	int rc;
	if ((rc = s.hist.ensure((size_t)256 * n_wg * 4)) || (rc = s.hist_base.ensure(((size_t)256 * n_wg + 1) * 8)) || (rc = s.bits.ensure(16))) return rc;
	unsigned long long bits[2] = { 0, ~0ull };
	HIP_TRY(hipMemcpyAsync(s.bits.p, bits, 16, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_key_bits, dim3(n_wg < 1024 ? n_wg : 1024), dim3(256), 0, c->stream, s.keys[0].as<uint64_t>(), n, s.bits.as<unsigned long long>());
	if ((rc = launched())) return rc;
	HIP_TRY(hipMemcpyAsync(bits, s.bits.p, 16, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	unsigned long long differ = bits[0] ^ bits[1];                 // bits that are not the same in all keys
	if (key_bits < 64) differ &= (1ull << key_bits) - 1;          // bits above the key's width are not part of the order
	int cur = 0;
	for (int shift = 0; shift < key_bits; shift += 8) {
		if (!(differ >> shift & 0xff)) continue;                    // every key has the same digit here: the pass would move nothing
		hipLaunchKernelGGL(k_rs_hist, dim3(n_wg), dim3(RS_T), 0, c->stream, s.keys[cur].as<uint64_t>(), n, shift, s.hist.as<int>(), n_wg);
		if ((rc = launched()) || (rc = launch_scan(s.hist.as<int>(), s.hist_base.as<int64_t>(), 256 * n_wg, c->d_scan, c->stream))) return rc;
		hipLaunchKernelGGL(k_rs_scatter, dim3(n_wg), dim3(RS_T), 0, c->stream, s.keys[cur].as<uint64_t>(), s.idx[cur].as<unsigned>(),
		                   s.keys[cur ^ 1].as<uint64_t>(), s.idx[cur ^ 1].as<unsigned>(), n, shift, s.hist_base.as<int64_t>(), n_wg);
		if ((rc = launched())) return rc;
		cur ^= 1; ++s.n_passes;
	}
	*which = cur;
	return 0;
}

int bam_sort_batch(bwahip_ctx *c, int n, int64_t total, int dup_tmpl)
{
	BamSort &s = c->bs;
	c->out->n_rec = 0; s.n_passes = 0;
	if (n <= 0) return 0;
	int rc;
	for (auto &e : c->out->ev_sort) if (!e && (rc = e.make())) return rc;
	if ((rc = s.rec_cnt.ensure((size_t)n * 4)) || (rc = s.rec_base.ensure(((size_t)n + 1) * 8)) || (rc = s.bits.ensure(16))) return rc;
	const uint8_t *raw = s.raw.as<uint8_t>();
	const int64_t *off = c->out->d_sam_off.as<int64_t>();
	const int grid_n = (n + 255) / 256;
	HIP_TRY(hipEventRecord(c->out->ev_sort[0], c->stream));
	HIP_TRY(hipMemsetAsync(s.bits.p, 0, 16, c->stream));
	hipLaunchKernelGGL(k_rec_count, dim3(grid_n), dim3(256), 0, c->stream, raw, off, n, s.rec_cnt.as<int>(), s.bits.as<int>());
	if ((rc = launched()) || (rc = launch_scan(s.rec_cnt.as<int>(), s.rec_base.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	int64_t n_rec = 0; int err = 0;
	HIP_TRY(hipMemcpyAsync(&n_rec, s.rec_base.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(&err, s.bits.p, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (err || n_rec < 0 || n_rec > 0x7fffffff) { fprintf(stderr, "[bwahip] sorted BAM: the records of the batch do not chain (%lld records)\n", (long long)n_rec); return BWAHIP_EINTERNAL; }
	const size_t R = (size_t)(n_rec ? n_rec : 1);
	if ((rc = s.keys[0].ensure(R * 8)) || (rc = s.keys[1].ensure(R * 8)) || (rc = s.idx[0].ensure(R * 4)) || (rc = s.idx[1].ensure(R * 4)) || (rc = s.off.ensure(R * 8)) ||
	    (rc = s.len.ensure(R * 4)) || (rc = s.len_sorted.ensure(R * 4)) || (rc = c->out->d_keys.ensure(R * 8)) || (rc = c->out->d_rec_off.ensure((R + 1) * 8))) return rc;
	const bwahip_bns_t *bns = &c->host.bns;
	hipLaunchKernelGGL(k_rec_fill, dim3(grid_n), dim3(256), 0, c->stream, raw, off, s.rec_base.as<int64_t>(), n, bns->n_seqs, bam_key_pos_bits(bns),
	                   s.keys[0].as<uint64_t>(), s.idx[0].as<unsigned>(), s.off.as<int64_t>(), s.len.as<int>());
	if ((rc = launched())) return rc;
	if (dup_tmpl && (rc = dup_batch_desc(c, n, dup_tmpl == 2, n_rec))) return rc;   // the mates are still neighbours here
	HIP_TRY(hipEventRecord(c->out->ev_sort[1], c->stream));
	int cur = 0;
	if ((rc = bam_sort_radix(c, (int)n_rec, bam_key_bits(bns), &cur))) return rc;
	HIP_TRY(hipEventRecord(c->out->ev_sort[2], c->stream));
	const int nr = (int)n_rec, grid_r = (nr + 255) / 256;
	if (nr > 0) {
		hipLaunchKernelGGL(k_gather_len, dim3(grid_r), dim3(256), 0, c->stream, s.idx[cur].as<unsigned>(), s.len.as<int>(), nr, s.len_sorted.as<int>());
		if ((rc = launched()) || (rc = launch_scan(s.len_sorted.as<int>(), c->out->d_rec_off.as<int64_t>(), nr, c->d_scan, c->stream))) return rc;
		HIP_TRY(hipMemcpyAsync(c->out->d_keys.p, s.keys[cur].p, (size_t)nr * 8, hipMemcpyDeviceToDevice, c->stream));
		hipLaunchKernelGGL(k_gather_copy, dim3((unsigned)(((int64_t)nr * 16 + 255) / 256)), dim3(256), 0, c->stream, raw, s.idx[cur].as<unsigned>(), s.off.as<int64_t>(),
		                   c->out->d_rec_off.as<int64_t>(), nr, c->out->d_sam.as<uint8_t>());
		if ((rc = launched())) return rc;
	} else HIP_TRY(hipMemsetAsync(c->out->d_rec_off.p, 0, 8, c->stream));
	if (dup_tmpl && (rc = dup_batch_tmpl(c, nr, s.idx[cur].as<unsigned>()))) return rc;
	HIP_TRY(hipEventRecord(c->out->ev_sort[3], c->stream));
	c->out->n_rec = n_rec;
	(void)total;
	return 0;
}
