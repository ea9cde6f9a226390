// soccer_inlists.hpp — the two-player lists the other way round (include/soccer_hip.h, "state occupancy"): for every state s'
// the entries that lead to it, which soccer_occupancy's sweep sums over.  Plain C++ with no HIP in it: soccer_pairs.hip
// builds the in-lists with it once per handle, and tests/host/inlists_host.cpp compiles it for the CPU tests.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "soccer_plan_io.hpp"

namespace soccer {

// in_offset[nS + 1] and the in-lists (InEntry, soccer_plan_io.hpp) of the out-lists offset[nS * 25 + 1] / list.
// The in-list of s' holds every out-entry whose next is s', whose done bit is clear and whose source state is not 0 (the out-lists' padding has its done bit set, so
// it goes with the rest), by ascending source key and then by position inside that key's list — the order a walk over the
// out-lists meets them in — padded to a multiple of kPlanPad with (prob 0.0, source key 0), which adds an exact +0.0 to a sum.
// Returns false, and leaves the outputs empty, if an entry's next is not a state or the padded total does not fit an int32.
inline bool build_inlists(int nS, const int32_t* offset, const PlanEntry* list, std::vector<int32_t>& in_offset,
                          std::vector<InEntry>& in_list) {
    in_offset.clear(); in_list.clear();
    if (nS < 1) return false;
    const int64_t keys = (int64_t)nS * 25;
    auto kept = [](const PlanEntry& e, int64_t key) { return e.next_done >= 0 && key >= 25; };
    std::vector<int64_t> count((size_t)nS, 0);
    for (int64_t key = 25; key < keys; ++key)
        for (int32_t e = offset[key]; e < offset[key + 1]; ++e)
            if (kept(list[e], key)) {
                if (list[e].next_done >= nS) return false;
                ++count[(size_t)list[e].next_done];
            }
    std::vector<int64_t> at((size_t)nS + 1, 0);
    for (int s = 0; s < nS; ++s) at[(size_t)s + 1] = at[(size_t)s] + (count[(size_t)s] + kPlanPad - 1) / kPlanPad * kPlanPad;
    if (at[(size_t)nS] > INT32_MAX) return false;
    in_offset.assign(at.begin(), at.end());
    in_list.assign((size_t)at[(size_t)nS], InEntry{0.0, 0, 0});
    for (int64_t key = 25; key < keys; ++key)
        for (int32_t e = offset[key]; e < offset[key + 1]; ++e)
            if (kept(list[e], key)) in_list[(size_t)at[(size_t)list[e].next_done]++] = InEntry{list[e].prob, (int32_t)key, 0};
    return true;
}

}  // namespace soccer
