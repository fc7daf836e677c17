// The coordinate-sort key of a BAM record (include/bwahip.h, "coordinate-sorted BAM"), one definition for the kernels (k_bamsort.hip)
// and for the host restatement bwahip_bam_sort_key (bam_sort_host.cpp).  Plain C++: compiles with and without hipcc.
//
//   bit 0                          reverse strand (flag 0x10): forward before reverse
//   bits 1 .. pos_bits             pos + 1 (pos -1 -> 0: first within its refID)
//   bits pos_bits + 1 .. and up    refID, with -1 (no reference) mapped to n_seqs: after every contig
//
// pos_bits = bit length of (longest contig + 1): pos + 1 ranges over 0 .. longest contig; the refID field is bit length of n_seqs wide.
// n_seqs and contig lengths are int32 (bntseq.h:41-64), so pos_bits <= 32, the refID field <= 31 and the key fits 64 bits for any index.
#pragma once
#include <stdint.h>
#include "../../include/bwahip.h"

#if defined(__HIPCC__)
#define BAMKEY_HD __host__ __device__
#else
#define BAMKEY_HD
#endif

BAMKEY_HD inline int bam_key_bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// the widths from the two numbers they depend on: the number of contigs and the length of the longest one
inline int bam_key_pos_bits_of(int64_t longest) { return bam_key_bit_length((uint64_t)(longest > 0 ? longest : 0) + 1); }
inline int bam_key_bits_of(int32_t n_seqs, int64_t longest) { return bam_key_bit_length((uint64_t)(n_seqs > 0 ? n_seqs : 0)) + bam_key_pos_bits_of(longest) + 1; }

inline int64_t bam_key_longest(const bwahip_bns_t *bns)
{
	int64_t longest = 0;
	for (int i = 0; i < bns->n_seqs; ++i) if (bns->anns[i].len > longest) longest = bns->anns[i].len;
	return longest;
}
inline int bam_key_pos_bits(const bwahip_bns_t *bns) { return bam_key_pos_bits_of(bam_key_longest(bns)); }
inline int bam_key_bits(const bwahip_bns_t *bns) { return bam_key_bits_of(bns->n_seqs, bam_key_longest(bns)); }

// a refID outside [0, n_seqs) counts as "no reference"; a pos beyond the field (no record of the product has one) saturates, so that
// the refID field above it is never touched
BAMKEY_HD inline uint64_t bam_key_pack(int32_t n_seqs, int pos_bits, int32_t refID, int32_t pos, int reverse)
{
	const uint64_t r = refID < 0 || refID >= n_seqs ? (uint64_t)(n_seqs > 0 ? n_seqs : 0) : (uint64_t)refID;
	const uint64_t pmax = pos_bits >= 64 ? ~0ull : (1ull << pos_bits) - 1;
	uint64_t p = pos < -1 ? 0 : (uint64_t)((int64_t)pos + 1);
	if (p > pmax) p = pmax;
	return r << (pos_bits + 1) | p << 1 | (reverse ? 1u : 0u);
}
