// K9d -- the BGZF blocks of the BAM output on the GPU: deflate (RFC 1951) and CRC32 of every block of at most 65 280 input bytes, the
// blocks cut exactly as bwahip_bgzf_write (bam_host.cpp) cuts them.  One workgroup per block on a grid that takes blocks in turn; the
// member is formed in the block's 64 KiB slot, a scan over the members' lengths and one copy make the contiguous output.
//
// Every stage gives the same result whatever the order in which lanes and wavefronts run (the same input gives the same bytes on every
// run, context and grid):
//
//   CRC32          64 input bytes per thread by slice-by-4, every chunk's CRC multiplied by x^(8 * bytes behind it) mod P (the arithmetic of
//                  zlib's crc32_combine) and all of them XORed;
//   match search   a table in LDS: hash of 4 bytes -> most recent earlier position.  Windows of 256 positions, one per thread: all look-ups of
//                  a window, a barrier, then its insertions by atomicMax on the position, a barrier.  Within its own wavefront a position
//                  also sees the nearest lower lane with the same hash (ballots); the positions of the window's earlier wavefronts it does
//                  not see.  The candidate is verified byte by byte (8 at a time): length 4..258, distance 1..32 768, never past the block;
//   greedy parse   next[p] = p + len[p] or p + 1; per 64-position window six rounds of pointer doubling by shuffles give every position
//                  its exit from the window, one lane follows the exits (one step per window at the most, from LDS), six more rounds mark
//                  the positions reachable from the window's entry;
//   counts         literal/length and distance symbols by integer LDS adds;
//   codes          per block (BTYPE = 2): the symbols ranked by (count, symbol) across a wavefront, the Huffman tree by the two-queue
//                  merge on one lane, every node's depth by a walk to the root on a lane of its own, depths limited to 15 (7 for the
//                  code-length alphabet) by the count-per-length repair that keeps the Kraft sum exact, lengths dealt by rank, canonical
//                  codes by ballots; an alphabet with fewer than two symbols in use gets a second one, so every set is complete; the
//                  sum is checked and a block whose set is not complete leaves stored;
//   emission       bits per token, window totals, an exclusive scan, every lane ORs its own token into zeroed words in LDS; the finished
//                  member goes to its slot 16 bytes per lane;
//   choice         the dynamic block, or the stored form (5 + n bytes, as bgzf_block at level 0) when that is not larger.
#include "ctx_internal.h"

namespace {

constexpr int BZ_IN = 65280, BZ_SLOT = 65536, BZ_T = 1024, BZ_WAVES = BZ_T / 64;
constexpr int BZ_HASH_BITS = 14, BZ_HWIN = 256, BZ_PRE = 8;
constexpr int BZ_GRP = 4;                    // windows whose per-position words a wavefront fetches together (one memory round trip per group)
constexpr int BZ_NLL = 286, BZ_ND = 30, BZ_NCL = 19;
constexpr int BZ_R_WORDS = 32768;            // the area the stages share in turn: CRC tables, hash table, window exits (u16 per position), output words
constexpr int BZ_OUT_WORDS = 16400;          // output words: BSIZE (2 bytes) + at most 5 + 65 280 deflate bytes + 8 trailer bytes, rounded up to 16 bytes
// code construction works above the output words
constexpr int BZ_HS_WORDS = 288 + 576 * 3 + 16;    // per builder: order, node weight, parent, depth, count per length
constexpr int BZ_HS0 = 17000, BZ_HS1 = BZ_HS0 + BZ_HS_WORDS, BZ_HDR = BZ_HS1 + BZ_HS_WORDS, BZ_HDR_WORDS = 160, BZ_CLS = BZ_HDR + BZ_HDR_WORDS, BZ_CLS_WORDS = 330;
static_assert(BZ_CLS + BZ_CLS_WORDS <= BZ_R_WORDS && BZ_OUT_WORDS <= BZ_HS0, "stage areas overlap");

typedef __attribute__((address_space(3))) uint32_t lds_u32;   // pointers into LDS that say so
typedef __attribute__((address_space(3))) uint16_t lds_u16;

// ---- CRC32 (IEEE, reflected): slice-by-4 tables and x^(2^k) mod P, made by the compiler ---------------------------------------------
constexpr uint32_t CRC_POLY = 0xedb88320u;
constexpr uint32_t crc_mul(uint32_t a, uint32_t b)      // a * b mod P, bit 31 = x^0
{
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {
		if (a & m) p ^= b;
		b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
	}
	return p;
}
struct CrcTab { uint32_t t[4][256]; uint32_t x2n[32]; };
constexpr CrcTab make_crc_tab()
{
	CrcTab c = {};
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t v = i;
		for (int k = 0; k < 8; ++k) v = v & 1 ? (v >> 1) ^ CRC_POLY : v >> 1;
		c.t[0][i] = v;
	}
	for (int s = 1; s < 4; ++s) for (uint32_t i = 0; i < 256; ++i) c.t[s][i] = (c.t[s - 1][i] >> 8) ^ c.t[0][c.t[s - 1][i] & 0xff];
	uint32_t p = 1u << 30;                              // x^1
	c.x2n[0] = p;
	for (int k = 1; k < 32; ++k) c.x2n[k] = p = crc_mul(p, p);
	return c;
}
__constant__ const CrcTab d_crc = make_crc_tab();

__device__ __forceinline__ uint32_t crc_mul_dev(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
#pragma unroll 4
	for (int k = 0; k < 32; ++k) {
		if (a & (0x80000000u >> k)) p ^= b;
		b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
	}
	return p;
}
// x^(8 * n) mod P
__device__ __forceinline__ uint32_t crc_x8n(uint32_t n)
{
	uint32_t p = 1u << 31;
	for (int k = 3; n; n >>= 1, ++k) if (n & 1) p = crc_mul_dev(d_crc.x2n[k & 31], p);
	return p;
}

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }   // the input starts at any byte
__device__ __forceinline__ uint64_t ld64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

// ---- deflate symbols -----------------------------------------------------------------------------------------------------------------
// length 3..258 -> code 0..28 (symbol 257 + code), extra bits and their value
__device__ __forceinline__ void len_sym(int len, int &code, int &eb, int &ev)
{
	if (len == 258) { code = 28; eb = 0; ev = 0; return; }
	const int l = len - 3;
	if (l < 8) { code = l; eb = 0; ev = 0; return; }
	const int msb = 31 - __clz(l);
	eb = msb - 2; code = 4 * eb + 4 + ((l >> eb) & 3); ev = l & ((1 << eb) - 1);
}
// distance 1..32768 -> code 0..29
__device__ __forceinline__ void dist_sym(int dist, int &code, int &eb, int &ev)
{
	const int d = dist - 1;
	if (d < 4) { code = d; eb = 0; ev = 0; return; }
	const int msb = 31 - __clz(d);
	eb = msb - 1; code = 2 * msb + ((d >> eb) & 1); ev = d & ((1 << eb) - 1);
}
__device__ __forceinline__ int ll_extra_bits(int s) { return s < 265 || s == 285 ? 0 : (s - 261) >> 2; }
__device__ __forceinline__ int d_extra_bits(int s) { return s < 4 ? 0 : (s >> 1) - 1; }

// ---- code lengths of one alphabet, by one wavefront ----------------------------------------------------------------------------------
// freq[0..n): counts (an alphabet with fewer than two symbols in use gets its lowest unused ones with count 1 for the build, as zlib does);
// lens / codes[0..n): the result, codes bit-reversed for the LSB-first stream.  ws: BZ_HS_WORDS words of LDS.  Returns (to every lane)
// the Kraft sum of the lengths scaled to 1 << maxlen: a complete set gives exactly 1 << maxlen.
__device__ uint32_t huff_build(lds_u32 *freq, int n, int maxlen, lds_u32 *lens, lds_u32 *codes, lds_u32 *ws, int lane)
{
	lds_u32 *order = ws, *wt = ws + 288, *par = wt + 576, *dep = par + 576, *blc = dep + 576;
	int forced[2] = { -1, -1 };
	if (lane == 0) {
		int used = 0;
		for (int s = 0; s < n; ++s) used += freq[s] != 0;
		for (int s = 0, k = 0; s < n && used < 2; ++s) if (freq[s] == 0) { freq[s] = 1; forced[k++] = s; ++used; }
	}
	__builtin_amdgcn_wave_barrier();
	// rank by (count, symbol): the least frequent first
	int m = 0;
	for (int s0 = 0; s0 < n; s0 += 64) {
		const int s = s0 + lane;
		const uint32_t f = s < n ? freq[s] : 0;
		m += __popcll(__ballot(f != 0));
		if (f) {
			int rank = 0;
			for (int t = 0; t < n; ++t) { const uint32_t g = freq[t]; rank += g != 0 && (g < f || (g == f && t < s)); }
			order[rank] = (uint32_t)s;
		}
		if (s < n) { lens[s] = 0; codes[s] = 0; }
	}
	__builtin_amdgcn_wave_barrier();
	uint32_t kraft = 0;
	for (int i = lane; i < m; i += 64) wt[i] = freq[order[i]];
	if (lane < 16) blc[lane] = 0;
	__builtin_amdgcn_wave_barrier();
	const int root = 2 * m - 2;
	if (lane == 0) {
		// two-queue merge: leaves 0..m-1 in rank order, inner nodes m..2m-2 in the order they are made (their weights do not decrease);
		// the two queue heads are kept in registers
		int i = 0, j = m;
		uint32_t wi = wt[0], wj = 0;
		for (int k = m; k <= root; ++k) {
			int a, b;
			uint32_t sum;
			if (i < m && (j >= k || wi <= wj)) { a = i++; sum = wi; if (i < m) wi = wt[i]; } else { a = j++; sum = wj; if (j < k) wj = wt[j]; }
			if (i < m && (j >= k || wi <= wj)) { b = i++; sum += wi; if (i < m) wi = wt[i]; } else { b = j++; sum += wj; if (j < k) wj = wt[j]; }
			wt[k] = sum; par[a] = (uint32_t)k; par[b] = (uint32_t)k;
			if (j == k) wj = sum;                                       // the node just made is the inner queue's head
		}
	}
	__builtin_amdgcn_wave_barrier();
	// depths: every node walks up to the root on a lane of its own.  A node deeper than maxlen counts as overflow (zlib's gen_bitlen
	// clamps a node whose parent is clamped), a leaf is counted at its clamped depth
	int overflow = 0;
	for (int v = lane; v < root; v += 64) {
		int d = 0;
		for (int u = v; u != root; u = (int)par[u]) ++d;
		if (d > maxlen) { d = maxlen; ++overflow; }
		if (v < m) __hip_atomic_fetch_add(blc + d, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	}
	for (int d = 32; d; d >>= 1) overflow += __shfl_xor(overflow, d);
	__builtin_amdgcn_wave_barrier();
	if (lane == 0) {
		while (overflow > 0) {                                      // zlib's gen_bitlen: one leaf a level down, an overflowing one as its brother
			int b = maxlen - 1;
			while (blc[b] == 0) --b;
			blc[b] -= 1; blc[b + 1] += 2; blc[maxlen] -= 1;
			overflow -= 2;
		}
		uint32_t code = 0;
		for (int b = 1; b <= maxlen; ++b) { code = (code + (b > 1 ? blc[b - 1] : 0)) << 1; dep[b] = code; kraft += blc[b] << (maxlen - b); }   // dep[b]: the next code of length b
	}
	__builtin_amdgcn_wave_barrier();
	// the lengths dealt by rank: the least frequent symbols get the longest codes
	for (int idx = lane; idx < m; idx += 64) {
		uint32_t acc = 0, L = 0;
		for (int b = maxlen; b >= 1; --b) { const uint32_t c = blc[b]; if ((uint32_t)idx >= acc && (uint32_t)idx < acc + c) L = (uint32_t)b; acc += c; }
		lens[order[idx]] = L;
	}
	__builtin_amdgcn_wave_barrier();
	// canonical codes: within a length, in symbol order -- 64 symbols at a time, the earlier ones of the same length by ballot
	{
		const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
		for (int s0 = 0; s0 < n; s0 += 64) {
			const int s = s0 + lane;
			const uint32_t l = s < n ? lens[s] : 0;
			uint32_t code = 0, add = 0;
			for (int b = 1; b <= maxlen; ++b) {
				const unsigned long long mask = __ballot(l == (uint32_t)b);
				if (l == (uint32_t)b) code = dep[b] + (uint32_t)__popcll(mask & below);
				if (lane == b) add = (uint32_t)__popcll(mask);
			}
			if (l) codes[s] = __brev(code) >> (32 - l);
			__builtin_amdgcn_wave_barrier();
			if (lane >= 1 && lane <= maxlen) dep[lane] += add;
			__builtin_amdgcn_wave_barrier();
		}
	}
	if (lane == 0) for (int k = 0; k < 2; ++k) if (forced[k] >= 0) freq[forced[k]] = 0;   // the counts are the tokens' again
	__builtin_amdgcn_wave_barrier();
	return (uint32_t)__shfl((int)kraft, 0);
}

// bytes [0, n) from src to dst by T threads: single bytes up to dst's first 16-byte boundary, then 16 bytes per thread and step (the
// source read unaligned), then the rest -- the shape of k_gather_copy
__device__ __forceinline__ void wg_copy(uint8_t *dst, const uint8_t *src, int n, int tid, int T)
{
	int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
	if (head > n) head = n;
	if (tid < head) dst[tid] = src[tid];
	const int body = (n - head) >> 4;
	for (int k = tid; k < body; k += T) {
		uint4 v;
		__builtin_memcpy(&v, src + head + 16 * k, 16);
		*reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
	}
	for (int k = head + 16 * body + tid; k < n; k += T) dst[k] = src[k];
}

// md: BZ_IN words per workgroup of the grid.  slots: BZ_SLOT bytes per block (16-byte aligned).  mlen[b]: the member's length.
__global__ __launch_bounds__(BZ_T) void k_bgzf_deflate(const uint8_t *in_all, int64_t len_all, int n_blocks, uint8_t *slots, int *mlen, uint32_t *md_all, unsigned long long *n_stored,
                                                     unsigned long long *ticks)
{
	__shared__ __attribute__((aligned(16))) uint32_t R[BZ_R_WORDS];
	__shared__ uint32_t s_tok[2 * 1024];         // per window: the lanes that begin a token
	__shared__ uint32_t s_win[1024];             // per window: bits of its tokens, then their exclusive prefix
	__shared__ uint32_t s_entry[1024];           // per window: the position in it the parse enters at (64: none)
	__shared__ uint32_t s_flag[BZ_WAVES * 64];
	__shared__ uint32_t s_fll[288], s_lll[288], s_cll[288], s_fd[32], s_ld[32], s_cd[32], s_fcl[32], s_lcl[32], s_ccl[32];
	__shared__ uint32_t s_misc[8];               // 0 crc, 1 total bits, 2 stored, 3 header bits, 4 kraft ll, 5 kraft d
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t *md = md_all + (size_t)blockIdx.x * BZ_IN;
	lds_u32 *R32 = (lds_u32*)R;
	lds_u16 *J1 = (lds_u16*)R;
	const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
	// BWAHIP_BGZF_LOG: the time of every stage (100 MHz ticks of thread 0, summed over the blocks)
	unsigned long long t_prev = ticks ? wall_clock64() : 0;
	auto stage_done = [&](int k) { if (ticks && tid == 0) { const unsigned long long t = wall_clock64(); atomicAdd(ticks + k, t - t_prev); t_prev = t; } };

	for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
		const uint8_t *in = in_all + (int64_t)blk * BZ_IN;
		const int n = (int)(len_all - (int64_t)blk * BZ_IN < BZ_IN ? len_all - (int64_t)blk * BZ_IN : BZ_IN);
		const int nwin = (n + 63) >> 6;
		uint8_t *slot = slots + (size_t)blk * BZ_SLOT;

		// ---- CRC32 ----
		R[tid] = d_crc.t[tid >> 8][tid & 255];
		if (tid < 288) s_fll[tid] = 0;
		if (tid < 32) { s_fd[tid] = 0; s_fcl[tid] = 0; }
		if (tid < 8) s_misc[tid] = 0;
		__syncthreads();
		{
			uint32_t part = 0;
			const int b0 = tid * 64;
			if (b0 < n) {
				const int e0 = b0 + 64 < n ? b0 + 64 : n;
				uint32_t c = ~0u;
				int i = b0;
				for (; i + 4 <= e0; i += 4) {
					c ^= ld32(in + i);
					c = R[768 + (c & 255)] ^ R[512 + ((c >> 8) & 255)] ^ R[256 + ((c >> 16) & 255)] ^ R[c >> 24];
				}
				for (; i < e0; ++i) c = R[(c ^ in[i]) & 255] ^ (c >> 8);
				c = ~c;
				part = e0 < n ? crc_mul_dev(crc_x8n((uint32_t)(n - e0)), c) : c;
			}
			for (int d = 32; d; d >>= 1) part ^= (uint32_t)__shfl_xor((int)part, d);
			if (lane == 0) __hip_atomic_fetch_xor((lds_u32*)s_misc, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		}
		__syncthreads();
		stage_done(0);

		// ---- match search: candidates ----
		for (int k = tid; k < (1 << BZ_HASH_BITS); k += BZ_T) R[k] = 0;   // position + 1; 0: none
		__syncthreads();
		uint32_t pre[BZ_PRE];
		for (int w0 = 0; w0 < n; w0 += BZ_HWIN) {
			const int p = w0 + tid;
			const bool act = tid < BZ_HWIN, valid = act && p + 4 <= n;
			// the input words of the next BZ_PRE windows are fetched together: one memory round trip per BZ_PRE windows, not per window
			const int wi = (w0 / BZ_HWIN) % BZ_PRE;
			if (wi == 0 && act) {
#pragma unroll
				for (int k = 0; k < BZ_PRE; ++k) { const int q = p + k * BZ_HWIN; pre[k] = q + 4 <= n ? ld32(in + q) : 0; }
			}
			uint32_t word = 0;
#pragma unroll
			for (int k = 0; k < BZ_PRE; ++k) if (k == wi) word = pre[k];
			uint32_t h = 0;
			unsigned long long same = 0;
			if (act) {                                                  // whole wavefronts: tid < 256 is wavefronts 0..3
				if (valid) h = (word * 2654435761u) >> (32 - BZ_HASH_BITS);
				same = __ballot(valid);
#pragma unroll
				for (int b = 0; b < BZ_HASH_BITS; ++b) {
					const bool bit = (h >> b & 1u) != 0;
					const unsigned long long bal = __ballot(bit);
					same &= bit ? bal : ~bal;
				}
				if (!valid) same = 0;
				uint32_t cand = valid ? R[h] : 0;
				const unsigned long long lower = same & below;
				if (lower) cand = (uint32_t)(p - lane + (63 - __clzll((long long)lower))) + 1;   // the nearest lower lane with the hash: more recent than the table's
				if (p < n) md[p] = cand;
			}
			__syncthreads();
			if (valid && (same >> lane) <= 1ull) __hip_atomic_fetch_max(R32 + h, (uint32_t)p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // the highest lane of the hash in this wavefront
			__syncthreads();
		}

		stage_done(1);
		// ---- match search: verify; md[p] = distance << 9 | length, or 0 ----
		// (four positions per thread at a time: their candidates, then their first 8 bytes, are fetched together)
		for (int p0 = tid; p0 < n; p0 += BZ_T * 4) {
			uint32_t c4[4];
			uint64_t x4[4];
#pragma unroll
			for (int u = 0; u < 4; ++u) { const int p = p0 + u * BZ_T; c4[u] = p < n ? md[p] : 0; }
#pragma unroll
			for (int u = 0; u < 4; ++u) {
				const int p = p0 + u * BZ_T;
				x4[u] = 0;
				if (c4[u] && p - ((int)c4[u] - 1) <= 32768 && n - p >= 8) x4[u] = ld64(in + ((int)c4[u] - 1)) ^ ld64(in + p);
			}
#pragma unroll
			for (int u = 0; u < 4; ++u) {
				const int p = p0 + u * BZ_T;
				if (p >= n) break;
				const uint32_t cand = c4[u];
				uint32_t r = 0;
				if (cand) {
					const int q = (int)cand - 1, dist = p - q;
					const int maxlen = n - p < 258 ? n - p : 258;
					if (dist >= 1 && dist <= 32768) {
						int k = 0;
						bool go = true;
						if (maxlen >= 8) { if (x4[u]) { k = (int)(__ffsll((long long)x4[u]) - 1) >> 3; go = false; } else k = 8; }
						while (go && k + 8 <= maxlen) {
							const uint64_t x = ld64(in + q + k) ^ ld64(in + p + k);
							if (x) { k += (int)(__ffsll((long long)x) - 1) >> 3; go = false; } else k += 8;
						}
						while (go && k < maxlen && in[q + k] == in[p + k]) ++k;
						if (k >= 4) r = (uint32_t)dist << 9 | (uint32_t)k;
					}
				}
				md[p] = r;
			}
		}
		__syncthreads();
		stage_done(2);

		// ---- greedy parse: the exit of every position from its 64-position window ----
		for (int w0 = wave; w0 < nwin; w0 += BZ_WAVES * BZ_GRP) {
			uint32_t m4[BZ_GRP];
#pragma unroll
			for (int k = 0; k < BZ_GRP; ++k) { const int q = ((w0 + BZ_WAVES * k) << 6) + lane; m4[k] = q < n ? md[q] : 0; }
#pragma unroll
			for (int k = 0; k < BZ_GRP; ++k) {
			const int w = w0 + BZ_WAVES * k;
			if (w >= nwin) break;
			const int base = w << 6, p = base + lane;
			int j = lane, ex = n;
			if (p < n) {
				const int l = (int)(m4[k] & 511u);
				const int nx = p + (l ? l : 1);
				if (nx < base + 64) j = nx - base; else ex = nx;
			}
#pragma unroll
			for (int k = 0; k < 6; ++k) j = __shfl(j, j);
			ex = __shfl(ex, j);
			J1[p] = (uint16_t)ex;                                       // <= n <= 65 280
			if (lane == 0) s_entry[w] = 64;
			}
		}
		__syncthreads();
		if (tid == 0) for (int e = 0; e < n; e = J1[e]) s_entry[e >> 6] = (uint32_t)(e & 63);   // every exit lies in a later window
		__syncthreads();
		stage_done(3);

		// ---- the tokens of every window, and the symbol counts ----
		for (int w0 = wave; w0 < nwin; w0 += BZ_WAVES * BZ_GRP) {
			uint32_t m4[BZ_GRP], b4[BZ_GRP];
#pragma unroll
			for (int k = 0; k < BZ_GRP; ++k) { const int q = ((w0 + BZ_WAVES * k) << 6) + lane; m4[k] = q < n ? md[q] : 0; b4[k] = q < n ? in[q] : 0; }
#pragma unroll
			for (int k = 0; k < BZ_GRP; ++k) {
			const int w = w0 + BZ_WAVES * k;
			if (w >= nwin) break;
			const int base = w << 6, p = base + lane;
			const int e = (int)s_entry[w];
			unsigned long long mask = 0;
			uint32_t m = 0;
			if (e < 64) {
				int g = lane;
				if (p < n) {
					m = m4[k];
					const int l = (int)(m & 511u);
					const int nx = p + (l ? l : 1);
					if (nx < base + 64) g = nx - base;
				}
				bool on = lane == e;
				s_flag[wave * 64 + lane] = 0;
				__builtin_amdgcn_wave_barrier();
#pragma unroll
				for (int k = 0; k < 6; ++k) {
					if (on) s_flag[wave * 64 + g] = 1;                    // every writer writes 1
					__builtin_amdgcn_wave_barrier();
					on = on || s_flag[wave * 64 + lane] != 0;
					__builtin_amdgcn_wave_barrier();
					g = __shfl(g, g);
				}
				mask = __ballot(on && p < n);
			}
			if (lane == 0) { s_tok[2 * w] = (uint32_t)mask; s_tok[2 * w + 1] = (uint32_t)(mask >> 32); }
			if (mask >> lane & 1ull) {
				if (m) {
					int c, eb, ev, c2;
					len_sym((int)(m & 511u), c, eb, ev);
					dist_sym((int)(m >> 9), c2, eb, ev);
					__hip_atomic_fetch_add((lds_u32*)s_fll + 257 + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					__hip_atomic_fetch_add((lds_u32*)s_fd + c2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				} else __hip_atomic_fetch_add((lds_u32*)s_fll + b4[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
			}
		}
		__syncthreads();
		stage_done(4);

		// ---- the block's codes; meanwhile the other wavefronts zero the output words ----
		if (wave == 0) {
			if (lane == 0) s_fll[256] = 1;
			const uint32_t kr = huff_build((lds_u32*)s_fll, BZ_NLL, 15, (lds_u32*)s_lll, (lds_u32*)s_cll, R32 + BZ_HS0, lane);
			if (lane == 0) s_misc[4] = kr;
		} else if (wave == 1) {
			const uint32_t kr = huff_build((lds_u32*)s_fd, BZ_ND, 15, (lds_u32*)s_ld, (lds_u32*)s_cd, R32 + BZ_HS1, lane);
			if (lane == 0) s_misc[5] = kr;
		} else for (int k = tid - 128; k < BZ_OUT_WORDS; k += BZ_T - 128) R[k] = 0;
		__syncthreads();
		if (wave == 0) {
			lds_u32 *cls = R32 + BZ_CLS, *hdr = R32 + BZ_HDR;
			for (int k = lane; k < BZ_HDR_WORDS; k += 64) hdr[k] = 0;
			__builtin_amdgcn_wave_barrier();
			int ncls = 0, hlit = 0, hdist = 0;
			if (lane == 0) {
				// the lengths of both alphabets as one sequence, run-length coded (RFC 1951 3.2.7): cls[i] = symbol | extra value << 8
				hlit = BZ_NLL; while (hlit > 257 && s_lll[hlit - 1] == 0) --hlit;
				hdist = BZ_ND; while (hdist > 1 && s_ld[hdist - 1] == 0) --hdist;
				const int tot = hlit + hdist;
				auto at = [&](int i) { return i < hlit ? (int)s_lll[i] : (int)s_ld[i - hlit]; };
				for (int i = 0; i < tot;) {
					const int v = at(i);
					int r = 1;
					while (i + r < tot && at(i + r) == v) ++r;
					i += r;
					if (v == 0) {
						while (r >= 11) { const int t = r < 138 ? r : 138; cls[ncls++] = 18u | (uint32_t)(t - 11) << 8; s_fcl[18] += 1; r -= t; }
						if (r >= 3) { cls[ncls++] = 17u | (uint32_t)(r - 3) << 8; s_fcl[17] += 1; r = 0; }
						for (; r > 0; --r) { cls[ncls++] = 0; s_fcl[0] += 1; }
					} else {
						cls[ncls++] = (uint32_t)v; s_fcl[v] += 1; --r;
						while (r >= 3) { const int t = r < 6 ? r : 6; cls[ncls++] = 16u | (uint32_t)(t - 3) << 8; s_fcl[16] += 1; r -= t; }
						for (; r > 0; --r) { cls[ncls++] = (uint32_t)v; s_fcl[v] += 1; }
					}
				}
			}
			__builtin_amdgcn_wave_barrier();
			const uint32_t kr_cl = huff_build((lds_u32*)s_fcl, BZ_NCL, 7, (lds_u32*)s_lcl, (lds_u32*)s_ccl, R32 + BZ_HS0, lane);
			// the bits of all tokens from the counts: code + extra bits per symbol
			uint32_t bits = 0;
			for (int s = lane; s < BZ_NLL; s += 64) bits += s_fll[s] * (s_lll[s] + (uint32_t)(s > 256 ? ll_extra_bits(s) : 0));
			if (lane < BZ_ND) bits += s_fd[lane] * (s_ld[lane] + (uint32_t)d_extra_bits(lane));
			for (int d = 32; d; d >>= 1) bits += (uint32_t)__shfl_xor((int)bits, d);
			if (lane == 0) {
				uint32_t hb = 0;
				auto put = [&](uint32_t v, int nb) {
					const uint32_t w = hb >> 5, s = hb & 31;
					hdr[w] |= v << s;
					if (s + nb > 32) hdr[w + 1] |= v >> (32 - s);
					hb += (uint32_t)nb;
				};
				static const uint8_t cl_order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
				int hclen = 19;
				while (hclen > 4 && s_lcl[cl_order[hclen - 1]] == 0) --hclen;
				put(1, 1); put(2, 2); put((uint32_t)(hlit - 257), 5); put((uint32_t)(hdist - 1), 5); put((uint32_t)(hclen - 4), 4);
				for (int k = 0; k < hclen; ++k) put(s_lcl[cl_order[k]], 3);
				for (int k = 0; k < ncls; ++k) {
					const uint32_t s = cls[k] & 255u, x = cls[k] >> 8;
					put(s_ccl[s], (int)s_lcl[s]);
					if (s == 16) put(x, 2); else if (s == 17) put(x, 3); else if (s == 18) put(x, 7);
				}
				s_misc[3] = hb;
				const uint32_t total = hb + bits;                          // the end-of-block symbol is counted in s_fll[256]
				s_misc[1] = total;
				const bool complete = s_misc[4] == (1u << 15) && s_misc[5] == (1u << 15) && kr_cl == (1u << 7);
				s_misc[2] = !complete || (total + 7) / 8 >= 5u + (uint32_t)n;
			}
		}
		__syncthreads();
		stage_done(5);
		const bool stored = s_misc[2] != 0;
		const uint32_t crc = s_misc[0];
		int dl;                                                         // bytes of the deflate stream
		if (stored) {
			dl = 5 + n;
			if (tid == 0) {
				static const uint8_t head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
				for (int k = 0; k < 16; ++k) slot[k] = head[k];
				const int total = 18 + dl + 8;
				slot[16] = (uint8_t)(total - 1); slot[17] = (uint8_t)((total - 1) >> 8);
				uint8_t *d = slot + 18;
				d[0] = 1; d[1] = (uint8_t)n; d[2] = (uint8_t)(n >> 8); d[3] = (uint8_t)~n; d[4] = (uint8_t)(~n >> 8);
				uint8_t *t = d + dl;
				for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
				atomicAdd(n_stored, 1ull);
			}
			wg_copy(slot + 23, in, n, tid, BZ_T);
		} else {
			const uint32_t hb = s_misc[3], total_bits = s_misc[1];
			dl = (int)((total_bits + 7) / 8);
			// bits of every window's tokens
			for (int w0 = wave; w0 < nwin; w0 += BZ_WAVES * BZ_GRP) {
				uint32_t m4[BZ_GRP], b4[BZ_GRP];
#pragma unroll
				for (int k = 0; k < BZ_GRP; ++k) { const int q = ((w0 + BZ_WAVES * k) << 6) + lane; m4[k] = q < n ? md[q] : 0; b4[k] = q < n ? in[q] : 0; }
#pragma unroll
				for (int k = 0; k < BZ_GRP; ++k) {
					const int w = w0 + BZ_WAVES * k;
					if (w >= nwin) break;
					const unsigned long long mask = (unsigned long long)s_tok[2 * w] | (unsigned long long)s_tok[2 * w + 1] << 32;
					uint32_t nb = 0;
					if (mask >> lane & 1ull) {
						const uint32_t m = m4[k];
						if (m) {
							int c, eb, ev, c2, eb2;
							len_sym((int)(m & 511u), c, eb, ev);
							dist_sym((int)(m >> 9), c2, eb2, ev);
							nb = s_lll[257 + c] + (uint32_t)eb + s_ld[c2] + (uint32_t)eb2;
						} else nb = s_lll[b4[k]];
					}
					for (int d = 32; d; d >>= 1) nb += (uint32_t)__shfl_xor((int)nb, d);
					if (lane == 0) s_win[w] = nb;
				}
			}
			__syncthreads();
			if (wave == 0) {                                            // exclusive scan over the windows: 16 per lane
				uint32_t v[16], sum = 0;
#pragma unroll
				for (int k = 0; k < 16; ++k) { const int w = lane * 16 + k; v[k] = w < nwin ? s_win[w] : 0; sum += v[k]; }
				uint32_t inc = sum;
				for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += t; }
				uint32_t run = inc - sum;
#pragma unroll
				for (int k = 0; k < 16; ++k) { const int w = lane * 16 + k; if (w < nwin) s_win[w] = run; run += v[k]; }
			}
			__syncthreads();
			// the output words begin at byte 16 of the member: 16 bits of BSIZE, then the stream
			auto emit = [&](uint64_t v, uint32_t o) {
				const uint32_t w = o >> 5, s = o & 31;
				const uint64_t lo = v << s;
				const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = s ? (uint32_t)(v >> (64 - s)) : 0;
				if (w0) __hip_atomic_fetch_or(R32 + w, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				if (w1) __hip_atomic_fetch_or(R32 + w + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				if (w2) __hip_atomic_fetch_or(R32 + w + 2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			};
			for (int k = tid; k < BZ_HDR_WORDS; k += BZ_T) { const uint32_t v = R[BZ_HDR + k]; if (v) emit(v, 16u + 32u * (uint32_t)k); }
			for (int w0 = wave; w0 < nwin; w0 += BZ_WAVES * BZ_GRP) {
				uint32_t m4[BZ_GRP], b4[BZ_GRP];
#pragma unroll
				for (int k = 0; k < BZ_GRP; ++k) { const int q = ((w0 + BZ_WAVES * k) << 6) + lane; m4[k] = q < n ? md[q] : 0; b4[k] = q < n ? in[q] : 0; }
#pragma unroll
				for (int k = 0; k < BZ_GRP; ++k) {
				const int w = w0 + BZ_WAVES * k;
				if (w >= nwin) break;
				const unsigned long long mask = (unsigned long long)s_tok[2 * w] | (unsigned long long)s_tok[2 * w + 1] << 32;
				uint32_t nb = 0;
				uint64_t v = 0;
				if (mask >> lane & 1ull) {
					const uint32_t m = m4[k];
					if (m) {
						int c, eb, ev, c2, eb2, ev2;
						len_sym((int)(m & 511u), c, eb, ev);
						dist_sym((int)(m >> 9), c2, eb2, ev2);
						v = s_cll[257 + c]; nb = s_lll[257 + c];
						v |= (uint64_t)ev << nb; nb += (uint32_t)eb;
						v |= (uint64_t)s_cd[c2] << nb; nb += s_ld[c2];
						v |= (uint64_t)ev2 << nb; nb += (uint32_t)eb2;
					} else { const uint32_t b = b4[k]; v = s_cll[b]; nb = s_lll[b]; }
				}
				uint32_t inc = nb;
				for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += t; }
				if (nb) emit(v, 16u + hb + s_win[w] + inc - nb);
				}
			}
			if (tid == 0) emit(s_cll[256], 16u + total_bits - s_lll[256]);   // end of block: the last bits of the stream
			__syncthreads();
			if (tid == 0) {                                             // BSIZE in front, CRC32 and ISIZE behind the stream's last byte
				const uint32_t total = 18u + (uint32_t)dl + 8u;
				R[0] |= (total - 1) & 0xffffu;
				const uint32_t vals[2] = { crc, (uint32_t)n };
				for (int k = 0; k < 8; ++k) {
					const uint32_t byte = (vals[k >> 2] >> (8 * (k & 3))) & 255u, o = 2u + (uint32_t)dl + (uint32_t)k;
					R[o >> 2] |= byte << (8 * (o & 3));
				}
			}
			if (tid == 1) {
				static const uint8_t head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
				for (int k = 0; k < 16; ++k) slot[k] = head[k];
			}
			__syncthreads();
			const int n16 = (2 + dl + 8 + 15) >> 4;                       // 16-byte pieces from byte 16 of the slot: at most 65 312 bytes
			for (int k = tid; k < n16; k += BZ_T) *reinterpret_cast<uint4*>(slot + 16 + 16 * k) = make_uint4(R[4 * k], R[4 * k + 1], R[4 * k + 2], R[4 * k + 3]);
		}
		if (tid == 0) mlen[blk] = 18 + dl + 8;
		__syncthreads();
		stage_done(6);
		//                                                // the next block reuses every area
	}
}

// the members from their slots to their places: one workgroup per block in turn
__global__ __launch_bounds__(256) void k_bgzf_compact(const uint8_t *slots, const int64_t *moff, int n_blocks, uint8_t *out, int64_t *tot, const unsigned long long *n_stored)
{
	for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) wg_copy(out + moff[b], slots + (size_t)b * BZ_SLOT, (int)(moff[b + 1] - moff[b]), threadIdx.x, 256);
	if (blockIdx.x == 0 && threadIdx.x == 0) { tot[0] = moff[n_blocks]; tot[1] = (int64_t)*n_stored; }
}

} // namespace

int bgzf_deflate(bwahip_ctx *c, const uint8_t *d_in, int64_t len, DevBuf &out, int64_t *tot_dev, hipStream_t st)
{
	if (len < 0 || !tot_dev) return BWAHIP_EINVAL;
	const int64_t nb64 = bgzf_blocks(len);
	if (nb64 > 0x7fff0000ll / 4) return BWAHIP_ECAPACITY;
	const int nb = (int)nb64;
	if (nb == 0) { HIP_TRY(hipMemsetAsync(tot_dev, 0, 16, st)); return 0; }
	static int n_cu = 0;
	if (!n_cu) { hipDeviceProp_t pr; HIP_TRY(hipGetDeviceProperties(&pr, c->device)); n_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 64; }
	const int grid = nb < n_cu ? nb : n_cu;                         // the LDS of a workgroup leaves room for one per CU
	Bgzf &z = c->bz;
	int rc;
	if ((rc = z.slots.ensure((size_t)nb * BZ_SLOT)) || (rc = z.mlen.ensure((size_t)nb * 4)) || (rc = z.moff.ensure(((size_t)nb + 1) * 8)) ||
	    (rc = z.md.ensure((size_t)grid * BZ_IN * 4)) || (rc = z.cnt.ensure(8)) || (rc = out.ensure((size_t)len + (size_t)nb * 31 + 64))) return rc;
	static const bool log = getenv("BWAHIP_BGZF_LOG") != nullptr;
	if (log && (rc = z.cnt.ensure(8 + 8 * 8))) return rc;
	HIP_TRY(hipMemsetAsync(z.cnt.p, 0, log ? 72 : 8, st));
	hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(BZ_T), 0, st, d_in, len, nb, z.slots.as<uint8_t>(), z.mlen.as<int>(), z.md.as<uint32_t>(), z.cnt.as<unsigned long long>(),
	                   log ? z.cnt.as<unsigned long long>() + 1 : nullptr);
	if (hipGetLastError() != hipSuccess) return BWAHIP_ENODEV;
	if (log) {                                                     // diagnostic: the stages' shares, from the clock of every workgroup's first thread
		unsigned long long t[8];
		HIP_TRY(hipMemcpyAsync(t, z.cnt.as<unsigned long long>() + 1, 64, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		static const char *const names[7] = { "crc32", "candidates", "verify", "window exits", "tokens+counts", "codes", "emission" };
		unsigned long long sum = 0;
		for (int k = 0; k < 7; ++k) sum += t[k];
		fprintf(stderr, "[bwahip] bgzf: %d blocks on %d workgroups, per block:", nb, grid);
		for (int k = 0; k < 7; ++k) fprintf(stderr, " %s %.1f us (%.0f %%)", names[k], t[k] / 100.0 / nb, sum ? 100.0 * t[k] / sum : 0.0);
		fprintf(stderr, "\n");
	}
	if ((rc = launch_scan(z.mlen.as<int>(), z.moff.as<int64_t>(), nb, c->d_scan, st))) return rc;
	hipLaunchKernelGGL(k_bgzf_compact, dim3(nb < 4096 ? nb : 4096), dim3(256), 0, st, z.slots.as<uint8_t>(), z.moff.as<int64_t>(), nb, out.as<uint8_t>(), tot_dev, z.cnt.as<unsigned long long>());
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}
