// soccer_policy_rows.hpp — what the learners hold a caller's tables to before anything reaches the device: a policy row
// (every entry >= 0 and a number, the sequential float64 sum within 1e-8 + 1e-5 of 1), a fixed policy's threshold rows, and
// the bounds of a Q or V table.  Plain C++ with no HIP in it, and pure: a function reports WHERE an array fails, the caller
// in soccer_learners.hip words the message (as with league_check_weights of soccer_league.hpp);
// tests/host/policy_rows_host.cpp compiles it for the CPU tests.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace soccer {

// -1: the row [5] holds; k < 5: p[k] is negative or not a number; 5: the row does not sum to 1
inline int policy_row_check(const double* p) {
    double sum = 0.0;
    for (int k = 0; k < 5; ++k) {
        if (!(p[k] >= 0.0)) return k;
        sum = sum + p[k];
    }
    return std::fabs(sum - 1.0) <= 1e-8 + 1e-5 ? -1 : 5;
}

// the first row that does not hold; action as policy_row_check returns it
struct RowFault {
    size_t member;
    int state, action;
};

// rows first_row .. nS - 1 of `members` policies [nS][5] each (first_row 1: a checkpoint, whose row 0 is not read)
inline bool policy_rows_check(const double* policy, size_t members, int nS, int first_row, RowFault* bad) {
    for (size_t m = 0; m < members; ++m)
        for (int s = first_row; s < nS; ++s) {
            const int k = policy_row_check(policy + (m * (size_t)nS + (size_t)s) * 5);
            if (k >= 0) { *bad = RowFault{m, s, k}; return false; }
        }
    return true;
}

// a fixed mixed policy's threshold rows [nS][4], once: SoccerBatch.mixed_policy_thresholds; every row is checked, row 0 too
// (learner_thresholds(pi, 0.0, ...) of soccer_learner_kernels.hpp is this loop operation for operation: the populations of
// policy hill-climbers compute a FIXED player's row on the device from its pi row and get these bits — keep the two alike)
inline bool fixed_thresholds(const double* policy, int nS, uint16_t* rows, RowFault* bad) {
    for (int s = 0; s < nS; ++s) {
        const double* p = policy + (size_t)s * 5;
        const int k = policy_row_check(p);
        if (k >= 0) { *bad = RowFault{0, s, k}; return false; }
        double c = 0.0;
        for (int j = 0; j < 4; ++j) {
            c = c + p[j];
            double f = std::floor(c * 32768.0 + 1e-9);
            f = f < 0.0 ? 0.0 : (f > 32768.0 ? 32768.0 : f);
            rows[(size_t)s * 4 + j] = (uint16_t)f;
        }
    }
    return true;
}

constexpr size_t kInBounds = ~(size_t)0;

// `members` tables [nS][width] each, every value of rows 1 .. nS - 1 in [-1, 1] (row 0 of a member is not read):
// kInBounds, or the flat index of the first value that is not
inline size_t q_bounds_check(const double* q, size_t members, size_t nS, size_t width) {
    for (size_t m = 0; m < members; ++m)
        for (size_t i = (m * nS + 1) * width; i < (m + 1) * nS * width; ++i)
            if (!(q[i] >= -1.0 && q[i] <= 1.0)) return i;
    return kInBounds;
}

}  // namespace soccer
