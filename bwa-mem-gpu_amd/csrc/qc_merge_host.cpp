// The host merger (bam_sort_host.cpp) with the QC builder (qc_host.cpp) as its listener: the one place that knows both
#include "../../include/bwahip.h"
#include "bai_tables.h"

extern "C" int bwahip_bam_merger_set_qc(bwahip_bam_merger *m, bwahip_qc_builder *builder)
{
	if (!builder) return bam_merger_listen(m, nullptr, nullptr);
	return bam_merger_listen(m, [](void *b, const uint8_t *rec, int64_t len) { const int64_t one[2] = { 0, len }; return bwahip_qc_builder_add_records((bwahip_qc_builder*)b, rec, one, 1); }, builder);
}
