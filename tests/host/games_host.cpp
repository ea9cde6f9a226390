// Host build of the product's 5x5 matrix-game solver (gym_soccer_littman94_amd/csrc/soccer_games.hpp) for the CPU test
// tests/test_matrix_game_host.py and the bit-for-bit comparison with the GPU build in tests/test_gpu_minimax.py.
// Test infrastructure; not part of libsoccer_hip.so.
#include <cstdint>

#include "../../gym_soccer_littman94_amd/csrc/soccer_games.hpp"

using namespace soccer;

// n games A[n][5][5]; any output may be NULL.  saddle[g] = 1 when game g took the pure-saddle-point path.
extern "C" void games_solve_host(long n, const double* A, double* value, double* x, double* y, int32_t* saddle) {
    GameWork w;
    for (long g = 0; g < n; ++g) {
        double v = 0.0, xs[kGameN], ys[kGameN];
        const int s = solve_game5(A + g * kGameN * kGameN, &w, &v, xs, ys);
        if (value) value[g] = v;
        for (int i = 0; i < kGameN; ++i) {
            if (x) x[g * kGameN + i] = xs[i];
            if (y) y[g * kGameN + i] = ys[i];
        }
        if (saddle) saddle[g] = s;
    }
}
