// inlists_host.cpp — csrc/soccer_inlists.hpp driven on the host by a program of its own, so that it can be built with
// -fsanitize=address,undefined and run without anything preloaded (tests/test_occupancy_np.py).
//   inlists_host IN      IN holds, as decimal integers separated by white space: nS, the number of entries, the
//                        nS * 25 + 1 offsets, then per entry the bits of its probability (uint64) and next | done << 31 (int32)
// Prints nS + 1 in-offsets on one line, then one line per in-entry: the bits of its probability, its source key, its pad.
// Exit status 2 (and "refused") if the builder refuses the lists, 1 if IN cannot be read.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gym_soccer_littman94_amd/csrc/soccer_inlists.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 1;
    long long nS = 0, n = 0;
    if (std::fscanf(f, "%lld %lld", &nS, &n) != 2 || nS < 1 || nS > 65535 || n < 0 || n > (1 << 22)) { std::fclose(f); return 1; }
    std::vector<int32_t> offset((size_t)nS * 25 + 1);
    for (int32_t& o : offset) {
        long long v;
        if (std::fscanf(f, "%lld", &v) != 1 || v < 0 || v > n) { std::fclose(f); return 1; }
        o = (int32_t)v;
    }
    std::vector<soccer::PlanEntry> list((size_t)n);
    for (soccer::PlanEntry& e : list) {
        uint64_t bits; long long nd;
        if (std::fscanf(f, "%" SCNu64 " %lld", &bits, &nd) != 2) { std::fclose(f); return 1; }
        std::memcpy(&e.prob, &bits, 8);
        e.next_done = (int32_t)nd; e.reward = 0.0f;
    }
    std::fclose(f);
    std::vector<int32_t> in_offset; std::vector<soccer::InEntry> in_list;
    if (!soccer::build_inlists((int)nS, offset.data(), list.data(), in_offset, in_list)) { std::puts("refused"); return 2; }
    for (size_t i = 0; i < in_offset.size(); ++i) std::printf("%d%c", in_offset[i], i + 1 < in_offset.size() ? ' ' : '\n');
    for (const soccer::InEntry& e : in_list) {
        uint64_t bits; std::memcpy(&bits, &e.prob, 8);
        std::printf("%" PRIu64 " %d %d\n", bits, e.source_key, e.pad);
    }
    return 0;
}
