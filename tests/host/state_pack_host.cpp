// Host build of the packed resident state (swar::pack3 / swar::unpack3 of gym_soccer_littman94_amd/csrc/soccer_swar.hpp) for the
// CPU test tests/test_state_pack_host.py: the code the kernels run, compiled for the host.  Test infrastructure; not part of
// libsoccer_hip.so.
#include <cstdint>
#include <cstring>
#include <string>

#include "../../gym_soccer_littman94_amd/csrc/soccer_rules.hpp"
#include "../../gym_soccer_littman94_amd/csrc/soccer_swar.hpp"

using namespace soccer;

static uint32_t ld4(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

static bool same(const swar::Group& x, const swar::Group& y) {
    return x.ra == y.ra && x.ca == y.ca && x.rb == y.rb && x.cb == y.cb && x.ps == y.ps && x.tt == y.tt;
}

// Every (row_a, col_a, row_b, col_b, poss, need, t) with rows < 8, columns < 16, t <= 250, in every byte position of the dword,
// the other three bytes holding `bg` (a lane of its own: all fields 0, or all at their maximum): the packed bytes of the
// position are poss << 7 | row << 4 | col, need << 7 | row << 4 | col, t; unpack3(pack3(x)) == x; and the three neighbours come
// back as they went in, in the packed dwords and in the unpacked ones.  Returns the number of failures; first[0..6] = the first
// failing (ra, ca, rb, cb, ps, t, position).
extern "C" long state_pack_roundtrip(int32_t* first) {
    long bad = 0;
    for (int bgv = 0; bgv < 2; ++bgv) {
        const uint32_t g_r = bgv ? 7u : 0u, g_c = bgv ? 15u : 0u, g_p = bgv ? 3u : 0u, g_t = bgv ? 250u : 0u;
        for (int pos = 0; pos < 4; ++pos) {
            const uint32_t sh = 8u * (uint32_t)pos, keep = ~(0xffu << sh);
            auto put = [&](uint32_t bg, uint32_t v) { return ((bg * 0x01010101u) & keep) | (v << sh); };
            for (uint32_t ra = 0; ra < 8; ++ra) for (uint32_t ca = 0; ca < 16; ++ca) for (uint32_t rb = 0; rb < 8; ++rb)
            for (uint32_t cb = 0; cb < 16; ++cb) for (uint32_t ps = 0; ps < 4; ++ps) for (uint32_t t = 0; t <= 250; ++t) {
                const swar::Group x{put(g_r, ra), put(g_c, ca), put(g_r, rb), put(g_c, cb), put(g_p, ps), put(g_t, t)};
                uint32_t a, b, tt;
                swar::pack3(x, a, b, tt);
                swar::Group y;
                swar::unpack3(a, b, tt, y);
                const uint32_t ea = put((g_p & 1u) << 7 | g_r << 4 | g_c, (ps & 1u) << 7 | ra << 4 | ca);
                const uint32_t eb = put((g_p >> 1) << 7 | g_r << 4 | g_c, (ps >> 1) << 7 | rb << 4 | cb);
                if (!same(x, y) || a != ea || b != eb || tt != x.tt) {
                    if (!bad) { first[0] = (int32_t)ra; first[1] = (int32_t)ca; first[2] = (int32_t)rb; first[3] = (int32_t)cb; first[4] = (int32_t)ps; first[5] = (int32_t)t; first[6] = pos; }
                    ++bad;
                }
            }
        }
    }
    return bad;
}

// One step of n lanes (a multiple of 4) taken twice: on the six dwords of a swar::Group as loaded from the six streams, and
// through the packed state — pack3 of the same six dwords is what the handle holds, the kernel's unpack3 / step4 / pack3 runs on
// it, and unpack3 of what it stores is the next state.  Every field of swar::Out and the next state must agree.  words as in
// swar_step_host (tests/host/swar_host.cpp): quarter draw = the word's two top bits, reset draw = its two low bits.
// Returns the number of groups that differ (first_group = the first of them), -1 when the pitch does not fit the byte
// arithmetic, -5 when it does not pack.  The next state of the packed walk is written back to the six streams, the results of
// the packed walk to obs / rew / term / trunc (so the caller can also hold them against the oracle).
extern "C" long state_pack_step(int width, int height, int max_steps, int autoreset, int general, int full, int force_geo0, long n,
                                uint8_t* ra, uint8_t* ca, uint8_t* rb, uint8_t* cb, uint8_t* ps, uint8_t* tt,
                                const uint8_t* act_a, const uint8_t* act_b, const uint32_t* words,
                                uint16_t* obs, uint8_t* rew, uint8_t* term, uint8_t* trunc, long* first_group) {
    Rules R;
    if (!R.build(width, height).empty()) return -2;
    if (!swar::fits(R.H, R.W, max_steps)) return -1;
    if (!swar::packs(R.H, R.W)) return -5;
    const swar::Consts C = swar::make_consts(R.H, R.W, R.goal_lo, R.goal_hi, max_steps, R.n_isd, R.isd, autoreset != 0);
    long bad = 0;
    for (long i = 0; i < n; i += 4) {
        const swar::Group S0{ld4(ra + i), ld4(ca + i), ld4(rb + i), ld4(cb + i), ld4(ps + i), ld4(tt + i)};
        const uint32_t a = ld4(act_a + i), b = ld4(act_b + i);
        const uint32_t* w = words + i;
        const swar::Rand4 rnd = swar::rand_words(C.isd_shift, w[0], w[1], w[2], w[3]);
        auto step = [&](swar::Group& S, swar::Out& o) {
#define CALL(G, F) do { if (C.small && !force_geo0) swar::step4<G, F, false, 1>(C, S, a, b, 0u, 0u, 0u, rnd, o); \
                        else swar::step4<G, F, false, 0>(C, S, a, b, 0u, 0u, 0u, rnd, o); } while (0)
            if (general) { if (full) CALL(true, true); else CALL(true, false); }
            else { if (full) CALL(false, true); else CALL(false, false); }
#undef CALL
        };
        swar::Group G = S0; swar::Out og{};
        step(G, og);
        uint32_t pa, pb, pt;
        swar::pack3(S0, pa, pb, pt);                            // what the handle holds
        swar::Group P; swar::Out op{};
        swar::unpack3(pa, pb, pt, P);
        step(P, op);
        swar::pack3(P, pa, pb, pt);                             // what the kernel stores
        swar::Group N;
        swar::unpack3(pa, pb, pt, N);
        bool ok = same(G, N) && og.obs_lo == op.obs_lo && og.obs_hi == op.obs_hi && og.rew == op.rew && og.term == op.term &&
                  og.trunc == op.trunc && og.finished == op.finished && og.frozen == op.frozen && og.bad_action == op.bad_action;
        if (full) ok = ok && og.fin_lo == op.fin_lo && og.fin_hi == op.fin_hi && og.code == op.code;
        if (!ok) { if (!bad) *first_group = i >> 2; ++bad; }
        std::memcpy(ra + i, &N.ra, 4); std::memcpy(ca + i, &N.ca, 4); std::memcpy(rb + i, &N.rb, 4); std::memcpy(cb + i, &N.cb, 4);
        std::memcpy(ps + i, &N.ps, 4); std::memcpy(tt + i, &N.tt, 4);
        obs[i] = (uint16_t)op.obs_lo; obs[i + 1] = (uint16_t)(op.obs_lo >> 16); obs[i + 2] = (uint16_t)op.obs_hi; obs[i + 3] = (uint16_t)(op.obs_hi >> 16);
        std::memcpy(rew + i, &op.rew, 4); std::memcpy(term + i, &op.term, 4); std::memcpy(trunc + i, &op.trunc, 4);
    }
    return bad;
}
