// Host build of the league's kick-off draw (gym_soccer_littman94_amd/csrc/soccer_league.hpp) for the CPU test
// tests/test_league_np.py: the threshold builder soccer_q_population_create_league runs and the count the kernel runs.
// Test infrastructure; not part of libsoccer_hip.so.
#include <cstdint>

#include "../../gym_soccer_littman94_amd/csrc/soccer_league.hpp"

using namespace soccer;

// -1: the weights hold, else the first bad index, K: a bad sum
extern "C" int league_check_host(const double* w, int K) { return league_check_weights(w, K); }

// T[K - 1]
extern "C" void league_thresholds_host(const double* w, int K, uint64_t* T) { league_thresholds(w, K, T); }

// pick[n] of the words W[n]
extern "C" void league_pick_host(const uint64_t* T, int K, long n, const uint32_t* W, int32_t* pick) {
    for (long i = 0; i < n; ++i) pick[i] = league_pick(T, K - 1, W[i]);
}
