// Host build of what the learners hold a caller's tables to (gym_soccer_littman94_amd/csrc/soccer_policy_rows.hpp) for the
// CPU test tests/test_policy_rows_host.py: the row check, a fixed policy's threshold rows and the Q-bounds check that
// soccer_learners.hip runs before anything reaches the device.  Test infrastructure; not part of libsoccer_hip.so.
#include <cstdint>

#include "../../gym_soccer_littman94_amd/csrc/soccer_policy_rows.hpp"

using namespace soccer;

static int report(bool ok, const RowFault& f, long* bad) {
    if (!ok) { bad[0] = (long)f.member; bad[1] = f.state; bad[2] = f.action; }
    return ok ? 1 : 0;
}

// 1: every row holds; 0: bad[3] = the first bad (member, state, action), action 5: the row's sum
extern "C" int policy_rows_check_host(const double* policy, long members, int nS, int first_row, long* bad) {
    RowFault f{};
    return report(policy_rows_check(policy, (size_t)members, nS, first_row, &f), f, bad);
}

// rows[nS][4]; 1 / 0 and bad[3] as above (member 0)
extern "C" int fixed_thresholds_host(const double* policy, int nS, uint16_t* rows, long* bad) {
    RowFault f{};
    return report(fixed_thresholds(policy, nS, rows, &f), f, bad);
}

// -1: in bounds, else the flat index of the first value of a row 1.. outside [-1, 1]
extern "C" long q_bounds_check_host(const double* q, long members, long nS, long width) {
    const size_t i = q_bounds_check(q, (size_t)members, (size_t)nS, (size_t)width);
    return i == kInBounds ? -1 : (long)i;
}
