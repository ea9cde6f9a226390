// soccer_league.hpp — the kick-off draw of a league opponent (include/soccer_hip.h, "learners, a league opponent for the
// population of Q-learners"): the integer thresholds of the weight vector, built once on the host, and the count that turns
// a 32-bit Philox word into a pick.  Plain C++ with no HIP in it: soccer_learners.hip builds the table with it, the kernel
// searches the table with league_pick, and tests/host/league_host.cpp compiles it for the CPU tests.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SOCCER_LEAGUE_FN __host__ __device__ __forceinline__
#else
#define SOCCER_LEAGUE_FN inline
#endif

namespace soccer {

constexpr int kLeagueMaxPolicies = 1024;

// What a weight vector is held to, as a policy row is (fixed_thresholds): every entry >= 0 and a number, the sequential
// float64 sum within 1e-8 + 1e-5 of 1.  Returns -1 if it holds, the index of the first bad entry, or K for a bad sum.
inline int league_check_weights(const double* w, int K) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        if (!(w[k] >= 0.0) || std::isinf(w[k])) return k;
        sum = sum + w[k];
    }
    return std::fabs(sum - 1.0) <= 1e-8 + 1e-5 ? -1 : K;
}

// T[k] = min(2^32, floor(c_k * 2^32)) for k < K - 1, c_k the sequential float64 sum w_0 + .. + w_k.  Never decreasing:
// the weights are >= 0, and rounding, the floor and the min keep the order.  (c * 2^32 is exact: a power of two.)
inline void league_thresholds(const double* w, int K, uint64_t* T) {
    double c = 0.0;
    for (int k = 0; k + 1 < K; ++k) {
        c = c + w[k];
        double f = std::floor(c * 4294967296.0);
        f = f < 0.0 ? 0.0 : (f > 4294967296.0 ? 4294967296.0 : f);
        T[k] = (uint64_t)f;
    }
}

// #{k < m : W >= T[k]} of a never decreasing T[m] (m = K - 1 <= 1023): the first index whose threshold exceeds W, by
// bisection — ten probes at most, where a scan by one lane would hold its wave for a thousand.
SOCCER_LEAGUE_FN int league_pick(const uint64_t* T, int m, uint32_t W) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool ge = (uint64_t)W >= T[mid];
        lo = ge ? mid + 1 : lo;
        hi = ge ? hi : mid;
    }
    return lo;
}

}  // namespace soccer
