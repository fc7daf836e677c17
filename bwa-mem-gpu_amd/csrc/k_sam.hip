// K9 -- SAM text on the GPU.  The record lists of a read (mem_reg2sam, bwamem.c:1025-1056; mem_sam_pe's output part) and the
// decisions of every record live in rec_dev.h, shared with the BAM kernels (k_bam.hip); this file instantiates them with the text
// writer of sam_dev.h (mem_aln2sam).  One read per wavefront.  Two launches of the same code: the first computes each read's text
// length (and applies the per-record adjustments once), an exclusive scan turns lengths into offsets, the second writes -- so the
// text of read i always lands at a fixed place and the batch's SAM is one contiguous buffer in read order (no atomics:
// deterministic output).
#include "bwahip_internal.h"
#include "sam_dev.h"

namespace {
using namespace samdev;

template <bool WRITE>
__global__ __launch_bounds__(64) void k_sam_se(FinLaunch a) { records_se<WRITE, TextFmt>(a); }

template <bool WRITE>
__global__ __launch_bounds__(64, (WRITE ? 6 : 8)) void k_sam_pe(FinLaunch a)   // (occupancy over registers: size pass at 8 waves per SIMD 1.56 -> 1.30 ms, write pass at 6 with 48 B of spill 3.47 -> 3.27 ms)
{ records_pe<WRITE, TextFmt>(a); }

} // namespace

int launch_sam_pe(const FinLaunch &a_, bool write, hipStream_t st, int read_lo, int read_hi)
{
	if (read_hi < 0) read_hi = a_.n_reads;
	if (read_hi <= read_lo) return 0;
	FinLaunch a = a_;
	a.read_lo = read_lo;
	if (write) hipLaunchKernelGGL(k_sam_pe<true>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	else hipLaunchKernelGGL(k_sam_pe<false>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}

int launch_sam(const FinLaunch &a_, bool write, hipStream_t st, int read_lo, int read_hi)
{
	if (read_hi < 0) read_hi = a_.n_reads;
	if (read_hi <= read_lo) return 0;
	FinLaunch a = a_;
	a.read_lo = read_lo;
	if (write) hipLaunchKernelGGL(k_sam_se<true>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	else hipLaunchKernelGGL(k_sam_se<false>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}
