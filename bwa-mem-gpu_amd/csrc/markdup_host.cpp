// The duplicate decision of include/bwahip.h on the host: no device, no HIP.  The second judge of the device stage (k_markdup.hip) in the
// tests, and what a host merger would use.  Written from the rule, not from the device stage: ordered maps keyed by signature and by
// end word, one pass in input order each.
#include "../../include/bwahip.h"
#include <map>
#include <utility>

extern "C" uint64_t bwahip_dup_end_word(int32_t refID, int32_t u5, int reverse)
{
	return (uint64_t)(int64_t)refID << 33 | (uint64_t)((int64_t)u5 + (1ll << 31)) << 1 | (reverse ? 1u : 0u);
}

extern "C" int bwahip_markdup_decide_host(const bwahip_dup_desc_t *desc, int64_t n_tmpl, uint8_t *dup_out)
{
	if (n_tmpl < 0 || (n_tmpl && (!desc || !dup_out))) return BWAHIP_EINVAL;
	for (int64_t i = 0; i < n_tmpl; ++i) if (desc[i].kind > 2) return BWAHIP_EINVAL;
	// the template kept so far per signature / per end word: a later one replaces it only with a strictly higher score
	std::map<std::pair<uint64_t, uint64_t>, int64_t> best_pair;
	std::map<uint64_t, int64_t> best_frag;
	std::map<uint64_t, bool> pair_end;
	for (int64_t i = 0; i < n_tmpl; ++i) {
		const bwahip_dup_desc_t &d = desc[i];
		dup_out[i] = 0;
		if (d.kind == 2) {
			pair_end[d.end[0]] = pair_end[d.end[1]] = true;
			auto it = best_pair.emplace(std::make_pair(d.end[0], d.end[1]), i);
			if (!it.second && d.score > desc[it.first->second].score) it.first->second = i;
		} else if (d.kind == 1) {
			auto it = best_frag.emplace(d.end[0], i);
			if (!it.second && d.score > desc[it.first->second].score) it.first->second = i;
		}
	}
	for (int64_t i = 0; i < n_tmpl; ++i) {
		const bwahip_dup_desc_t &d = desc[i];
		if (d.kind == 2) dup_out[i] = best_pair[std::make_pair(d.end[0], d.end[1])] != i;
		else if (d.kind == 1) dup_out[i] = pair_end.count(d.end[0]) || best_frag[d.end[0]] != i;
	}
	return 0;
}
