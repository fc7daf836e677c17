// What every reader and writer of BAM records shares (bai_tables.h, qc_tables.h and what builds on them, bam_dev.h): an unaligned
// little-endian word and the bin of an interval.  The checks of the 36-byte head stay spelled out in bai_parse and qc_parse: built on one
// function, k_bai.hip, k_qc.hip and k_pileup.hip compiled to other code.  Plain C++; __host__ __device__ where a HIP compiler reads it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BAM_HD __host__ __device__
#else
#define BAM_HD
#endif

BAM_HD inline uint32_t bam_ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }   // records begin at any address

// reg2bin of the specification (section 5.3) on signed values: pos = -1, end = 0 gives 4680
BAM_HD inline uint32_t bam_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}
