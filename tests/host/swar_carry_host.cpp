// Host build of the steady state's CARRIED step (swar::Carry4 / step4_carry, gym_soccer_littman94_amd/csrc/soccer_swar.hpp) for
// tests/test_swar_carry_host.py: the way the rollout loop runs it — convert in, step, step, convert out — next to the
// same two steps as swar::step4<false, ...> calls, which tests/test_swar_host.py pins to the oracle.  Test infrastructure.
#include <cstdint>
#include <cstring>

#include "../../gym_soccer_littman94_amd/csrc/soccer_rules.hpp"
#include "../../gym_soccer_littman94_amd/csrc/soccer_swar.hpp"
#include "../../gym_soccer_littman94_amd/csrc/soccer_slip.hpp"

using namespace soccer;

static uint32_t ld4(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
static void st4(uint8_t* p, uint32_t v) { std::memcpy(p, &v, 4); }

// n lanes (a multiple of 4), `steps` steps in a row.  state: six byte streams of n lanes (in / out, Group form).  Per step k the
// rows act_a / act_b / words [k * n, (k + 1) * n) go in and the rows of every output come out; bad has n / 4 entries per step.
// carried != 0: carry_of, `steps` x step4_carry, group_of; else `steps` x step4<false>.
// geo: -1 byte tables where the pitch has them, 0 arithmetic forced.  sel: slip selection 1 one by one, 2 the rollout's table.
// Words as in swar_host.cpp: one per lane and step (quarter draw = the two top bits, reset draw = the two low bits).
// Returns 0, -1 / -3 when the pitch / the slip does not qualify, -4 when the slip has no bucket table.
extern "C" int swar_carry_host(int width, int height, int max_steps, int full, int geo, int sel, int carried, int steps, long n,
                               uint8_t* ra, uint8_t* ca, uint8_t* rb, uint8_t* cb, uint8_t* ps, uint8_t* tt,
                               const uint8_t* act_a, const uint8_t* act_b, const uint32_t* words, double slip_prob,
                               uint16_t* obs, uint16_t* final_obs, uint8_t* rew, uint8_t* term, uint8_t* trunc,
                               uint8_t* code, uint8_t* finished, uint8_t* bad) {
    Rules R;
    if (!R.build(width, height).empty()) return -2;
    if (!swar::fits(R.H, R.W, max_steps)) return -1;
    const swar::Consts C = swar::make_consts(R.H, R.W, R.goal_lo, R.goal_hi, max_steps, R.n_isd, R.isd, true);
    const bool slip = slip_prob != 0.0;
    const bool tables = C.small && geo != 0;
    SlipTables ST{}; swar::SlipConsts L{};
    if (slip) {
        ST = build_slip_tables(slip_prob);
        if (!ST.swar_ok) return -3;
        if (sel == 2 && !ST.lut_ok) return -4;
        for (int i = 0; i < 9; ++i) L.CB[i] = ST.CB[i];
        L.c_off = ST.c_off;
    }
    for (long i = 0; i < n; i += 4) {
        swar::Group S{ld4(ra + i), ld4(ca + i), ld4(rb + i), ld4(cb + i), ld4(ps + i), ld4(tt + i)};
        swar::Carry4 K{};
        if (carried) K = swar::carry_of(C, S);
        for (int k = 0; k < steps; ++k) {
            const long r = (long)k * n + i;
            swar::Out o{};
            const uint32_t a = ld4(act_a + r), b = ld4(act_b + r);
            const uint32_t* w = words + r;
            uint32_t s_a = 0u, s_b = 0u, k4 = 0u, c4 = 0u;
            // the carried loop hands the selection the low three bits (rollout_swar_group), the plain one canonical actions
            const uint32_t sa_in = carried ? a & 0x07070707u : swar::canon4(a), sb_in = carried ? b & 0x07070707u : swar::canon4(b);
            if (slip && sel == 2) swar::slip_select4_lut(ST.lut, ST.T, L.c_off, sa_in, sb_in, w[0], w[1], w[2], w[3], s_a, s_b, k4, c4);
            else if (slip) swar::slip_select4(L, ST.sub, sa_in, sb_in, w[0], w[1], w[2], w[3], s_a, s_b, k4, c4);
            swar::Rand4 rnd = swar::rand_words(C.isd_shift, w[0], w[1], w[2], w[3]);
            if (slip) rnd.kq = k4 << 6;
#define CALL(F, SL) do { if (carried) { if (tables) swar::step4_carry<F, SL, 1>(C, K, a, b, s_a, s_b, c4, rnd, o); \
                                        else swar::step4_carry<F, SL, 0>(C, K, a, b, s_a, s_b, c4, rnd, o); } \
                         else { if (tables) swar::step4<false, F, SL, 1>(C, S, a, b, s_a, s_b, c4, rnd, o); \
                                else swar::step4<false, F, SL, 0>(C, S, a, b, s_a, s_b, c4, rnd, o); } } while (0)
            if (slip) { if (full) CALL(true, true); else CALL(false, true); }
            else { if (full) CALL(true, false); else CALL(false, false); }
#undef CALL
            obs[r] = (uint16_t)o.obs_lo; obs[r + 1] = (uint16_t)(o.obs_lo >> 16); obs[r + 2] = (uint16_t)o.obs_hi; obs[r + 3] = (uint16_t)(o.obs_hi >> 16);
            if (full) {
                final_obs[r] = (uint16_t)o.fin_lo; final_obs[r + 1] = (uint16_t)(o.fin_lo >> 16);
                final_obs[r + 2] = (uint16_t)o.fin_hi; final_obs[r + 3] = (uint16_t)(o.fin_hi >> 16);
                st4(code + r, o.code);
            }
            st4(rew + r, o.rew); st4(term + r, o.term); st4(trunc + r, o.trunc);
            st4(finished + r, (o.finished >> 7) & 0x01010101u);
            bad[r >> 2] = o.bad_action != 0u;
        }
        if (carried) S = swar::group_of(C, K);
        st4(ra + i, S.ra); st4(ca + i, S.ca); st4(rb + i, S.rb); st4(cb + i, S.cb); st4(ps + i, S.ps); st4(tt + i, S.tt);
    }
    return 0;
}
