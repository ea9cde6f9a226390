// simplex_host.cpp — runs csrc/soccer_simplex.hpp's projection on the host (tests/test_simplex_host.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer).  Input file: the number of rows, then five doubles per row as the decimal
// value of their bit patterns.  Output: per row the five projected doubles, likewise.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gym_soccer_littman94_amd/csrc/soccer_simplex.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: simplex_host FILE\n"); return 1; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    long long n = 0;
    if (std::fscanf(f, "%lld", &n) != 1 || n < 0) { std::fclose(f); return 1; }
    std::vector<double> v((size_t)n * 5), out((size_t)n * 5);
    for (size_t i = 0; i < v.size(); ++i) {
        uint64_t b = 0;
        if (std::fscanf(f, "%" SCNu64, &b) != 1) { std::fclose(f); return 1; }
        std::memcpy(&v[i], &b, 8);
    }
    std::fclose(f);
    for (long long r = 0; r < n; ++r) soccer::project_simplex5(&v[(size_t)r * 5], &out[(size_t)r * 5]);
    for (long long r = 0; r < n; ++r) {
        for (int a = 0; a < 5; ++a) {
            uint64_t b = 0;
            std::memcpy(&b, &out[(size_t)r * 5 + a], 8);
            std::printf("%" PRIu64 "%c", b, a == 4 ? '\n' : ' ');
        }
    }
    return 0;
}
