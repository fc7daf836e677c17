// K9i -- a device merger whose runs' record bytes outgrow HBM.  A spilled run keeps its keys, offsets, template indices and
// descriptors in HBM; its record bytes lie in the host-side store (spill_store.cpp) and come back one window at a time: a window is
// window_pieces consecutive pieces of the sorted stream (k_bammerge.hip).  Every run is sorted and the global order is (key, run, position),
// so the records one window needs from one run are a contiguous slice of that run.  Two kernels:
//
//   k_spill_cuts   thread = sorted ordinal.  A record of a spilled run lowers, through an integer atomicMin, the cell (window, run) of the
//                  window in which its ordinal lies to its position in the run: the cell ends as the first position the window needs.
//                  The host completes the table (a window without a record of the run takes the next window's start) and derives every
//                  window's slices from the runs' offsets.  Column n_runs of a row: the run that owns the window's first record -- that
//                  record begins in the window before (or at the cut) and belongs to both slices.
//   k_spill_addr   thread = sorted ordinal of one window.  The source address of a record of a spilled run is rebuilt for the window:
//                  the staging address of the run's slice plus the record's offset within it (base[run] + off[run][position], base = the
//                  slice's staging address minus the offset of its first record).  Resident runs keep the addresses k_src_table gave them.
//
// No LDS.  The atomics are integer minima: the table does not depend on the order in which wavefronts run.  Plain vector stores only.
#include "ctx_internal.h"

namespace {

// the last run whose first ordinal is <= g (first: n_runs + 1 entries, the last = n): not empty, because the next one's is > g
__device__ __forceinline__ int run_of(const int64_t *first, int n_runs, int64_t g)
{
	int lo = 0, hi = n_runs;
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first[mid] <= g) lo = mid; else hi = mid; }
	return lo;
}

// the first ordinal of window w: the record that holds (or begins at) the window's first byte
__device__ __forceinline__ int window_first(const int *piece_first, int window_pieces, int w) { return piece_first[(int64_t)w * window_pieces]; }

// cut: n_windows rows of n_runs + 1 cells, the first n_runs preset to 0x7f7f7f7f (above every position)
__global__ __launch_bounds__(256) void k_spill_cuts(int n, int n_runs, const int64_t *first, const uint8_t *spilled, const unsigned *idx, const int *piece_first, int window_pieces,
                                                   int n_windows, int *cut)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int64_t g = idx[i];
	const int r = run_of(first, n_runs, g);
	int lo = 0, hi = n_windows;                                    // the last window whose first ordinal is <= i (window 0's is 0)
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (window_first(piece_first, window_pieces, mid) <= i) lo = mid; else hi = mid; }
	const size_t row = (size_t)lo * ((size_t)n_runs + 1);
	if (spilled[r]) {
		const int pos = (int)(g - first[r]);
		int *cell = cut + row + r;
		if (pos < __atomic_load_n(cell, __ATOMIC_RELAXED)) atomicMin(cell, pos);   // (the relaxed read only spares atomics: the value never rises, the atomic decides)
	}
	// the owner of the first record of every window that begins with this ordinal (several, when one record is longer than a window)
	for (int w = lo; w >= 0 && window_first(piece_first, window_pieces, w) == i; --w) cut[(size_t)w * ((size_t)n_runs + 1) + n_runs] = r;
}

__global__ __launch_bounds__(256) void k_spill_addr(int rec_lo, int n_rec, int n_runs, const int64_t *first, const int64_t *const *run_off, const uint8_t *spilled, const int64_t *base,
                                                   const unsigned *idx, const uint8_t **addr)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_rec) return;
	const int64_t g = idx[rec_lo + k];
	const int r = run_of(first, n_runs, g);
	if (!spilled[r]) return;
	addr[g] = reinterpret_cast<const uint8_t*>((uintptr_t)(base[r] + run_off[r][g - first[r]]));
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }

} // namespace

int spill_window_cuts(hipStream_t st, int n, int n_runs, const int64_t *first, const uint8_t *spilled, const unsigned *idx, const int *piece_first, int window_pieces, int n_windows, int *cut)
{
	if (n <= 0 || n_runs <= 0 || n_windows <= 0 || window_pieces <= 0) return BWAHIP_EINVAL;
	const size_t cells = (size_t)n_windows * ((size_t)n_runs + 1);
	HIP_TRY(hipMemsetAsync(cut, 0x7f, cells * 4, st));
	hipLaunchKernelGGL(k_spill_cuts, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, n, n_runs, first, spilled, idx, piece_first, window_pieces, n_windows, cut);
	return launched();
}

int spill_window_addr(hipStream_t st, int rec_lo, int n_rec, int n_runs, const int64_t *first, const int64_t *const *run_off, const uint8_t *spilled, const int64_t *base,
                      const unsigned *idx, const uint8_t **addr)
{
	if (n_rec <= 0) return 0;
	hipLaunchKernelGGL(k_spill_addr, dim3((unsigned)(((int64_t)n_rec + 255) / 256)), dim3(256), 0, st, rec_lo, n_rec, n_runs, first, run_off, spilled, base, idx, addr);
	return launched();
}

// The HBM of a device merger with spilled runs: bwahip_bam_devmerge_hbm_need of the resident record bytes (and all records' metadata), and
//   staging     two buffers, each a window (window_pieces x piece_blocks x 65 280 bytes) and two straddling records of longest_record
//               bytes -- the one that begins before the window and the one that ends behind it -- or all spilled bytes if that is less;
//   pieces      the piece buffers of bwahip_bam_devmerge_hbm_need for the blocks of a piece the resident bytes alone do not give
//               (326 730 bytes per block: two inputs, two outputs, the slot, the member's length and offset);
//   cut table   16 bytes per run and window (a 4-byte cut, an 8-byte base, one more column for the owner of the window's first record),
//               counted for the most windows any piece_blocks and window_pieces give -- one per block of the whole stream -- so that the
//               need never falls as either grows; at the default shapes the table is 8 192 times smaller;
// the three with the eighth of slack the working buffers grow with.
extern "C" int64_t bwahip_bam_devmerge_spill_hbm_need(int64_t resident_raw_bytes, int64_t spilled_raw_bytes, int64_t longest_record, int64_t n_records, int64_t n_runs, int piece_blocks,
                                                      int window_pieces)
{
	if (resident_raw_bytes < 0 || spilled_raw_bytes < 0 || longest_record < 0 || n_records < 0 || n_runs < 0 || piece_blocks < 1 || piece_blocks > 4096 || window_pieces < 1 ||
	    window_pieces > 65536) return -1;
	const int64_t base = bwahip_bam_devmerge_hbm_need(resident_raw_bytes, n_records, n_runs, piece_blocks);
	if (base < 0) return -1;
	int64_t stage = (int64_t)window_pieces * piece_blocks * 65280 + 2 * longest_record;
	if (stage > spilled_raw_bytes) stage = spilled_raw_bytes;
	const int64_t total_blocks = bgzf_blocks(resident_raw_bytes + spilled_raw_bytes);
	int64_t pb_res = bgzf_blocks(resident_raw_bytes), pb_tot = total_blocks;
	if (pb_res > piece_blocks) pb_res = piece_blocks;
	if (pb_tot > piece_blocks) pb_tot = piece_blocks;
	const int64_t pieces = (pb_tot - pb_res) * (4 * 65280 + 2 * 31 + 65536 + 12);
	const int64_t table = 16 * (n_runs + 1) * total_blocks;
	const int64_t work = 2 * stage + pieces + table;
	return base + work + work / 8;
}
