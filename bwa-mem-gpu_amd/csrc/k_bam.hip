// K9b -- BAM records on the GPU: the plan of k_sam.hip (one read per wavefront; a sizing pass, an exclusive scan, a write pass in two
// halves; the records of read i at a fixed offset, no atomics, deterministic) with the binary writer of bam_dev.h.  Which regions
// become records and what every record says is the code of rec_dev.h that the SAM kernels run.  The sizing pass adjusts the alignment
// array in place, so a batch goes through either these kernels or k_sam's, never both.
#include "bwahip_internal.h"
#include "bam_dev.h"

namespace {
using namespace samdev;

template <bool WRITE>
__global__ __launch_bounds__(64) void k_bam_se(FinLaunch a) { records_se<WRITE, BamFmt>(a); }

// occupancy as for k_sam_pe (the passes wait on scattered loads of names, qualities and the pool: more waves hide more of them)
template <bool WRITE>
__global__ __launch_bounds__(64, (WRITE ? 6 : 8)) void k_bam_pe(FinLaunch a) { records_pe<WRITE, BamFmt>(a); }

} // namespace

int launch_bam_pe(const FinLaunch &a_, bool write, hipStream_t st, int read_lo, int read_hi)
{
	if (read_hi < 0) read_hi = a_.n_reads;
	if (read_hi <= read_lo) return 0;
	FinLaunch a = a_;
	a.read_lo = read_lo;
	if (write) hipLaunchKernelGGL(k_bam_pe<true>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	else hipLaunchKernelGGL(k_bam_pe<false>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}

int launch_bam(const FinLaunch &a_, bool write, hipStream_t st, int read_lo, int read_hi)
{
	if (read_hi < 0) read_hi = a_.n_reads;
	if (read_hi <= read_lo) return 0;
	FinLaunch a = a_;
	a.read_lo = read_lo;
	if (write) hipLaunchKernelGGL(k_bam_se<true>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	else hipLaunchKernelGGL(k_bam_se<false>, dim3(read_hi - read_lo), dim3(64), 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}
