// soccer_hip.hip — C-ABI implementation of libsoccer_hip.so (see include/soccer_hip.h): the handle's life cycle,
// reset, state access, staging, the one-environment calls, statistics, timers and graph capture.  batched_step* is in
// soccer_step.hip, batched_rollout* in soccer_rollout.hip, the planners in soccer_planners.hip, soccer_comm_* in
// soccer_comm.hip; soccer_handle.hpp is what they share.
//
// Host side: validates arguments the way the reference's asserts do, builds the rule tables
// (soccer_rules.hpp), owns the resident SoA state, and enqueues the kernels of soccer_*_kernels.hpp
// on the handle's HIP stream.  There is no CPU execution path in this library: every batched_* call
// is a kernel launch, and a missing/failed device is an error, not a fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "soccer_dispatch.hpp"
#include "soccer_handle.hpp"
#include "soccer_env_kernels.hpp"
#include "soccer_slip.hpp"

static thread_local std::string g_err;       // the one error slot of calls without a handle, for every unit (through fail)

int fail(soccer_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (h) h->err = buf; else g_err = buf;
    return code;
}

// ------------------------------------------------------------------------------------------------
extern "C" int soccer_abi_version(void) { return SOCCER_ABI_VERSION; }

extern "C" int soccer_device_count(int* count) {
    if (!count) return fail(nullptr, SOCCER_E_INVALID, "count is NULL");
    HIP_TRY(nullptr, hipGetDeviceCount(count));
    return SOCCER_OK;
}

extern "C" const char* soccer_last_error(const soccer_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

// nothing is freed before the stream has drained; a handle whose creation failed early has no stream and no events
soccer_handle::~soccer_handle() {
    (void)hipSetDevice(cfg.device);
    (void)hipStreamSynchronize(stream);
    comm_release(this);
    learners_release(this);
    gradient_players_release(this);
    bufs.clear(); plan_bufs.clear(); mm_bufs.clear(); br_bufs.clear();      // here, not as members after this body: the stream is still alive
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

static void set_key(soccer_handle* h, uint64_t seed) {
    h->cfg.seed = seed;
    h->P.key0 = static_cast<uint32_t>(seed);
    h->P.key1 = static_cast<uint32_t>(seed >> 32);
}

extern "C" int soccer_create(const soccer_config* cfg, soccer_handle** out) {
    if (!cfg || !out) return fail(nullptr, SOCCER_E_INVALID, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->n_lanes < 1) return fail(nullptr, SOCCER_E_INVALID, "n_lanes must be >= 1");
    if (!(cfg->slip_prob >= 0.0 && cfg->slip_prob <= 1.0))
        return fail(nullptr, SOCCER_E_INVALID, "slip_prob must be in [0, 1]");
    if (cfg->max_steps < 1 || cfg->max_steps > 250)
        return fail(nullptr, SOCCER_E_INVALID, "max_steps must be in 1..250 (timestep is a uint8)");
    const uint32_t e = cfg->envs_per_thread;
    if (!(e == 0 || e == 1 || e == 4 || e == 8))
        return fail(nullptr, SOCCER_E_INVALID, "envs_per_thread must be 0, 1, 4 or 8");
    std::unique_ptr<soccer_handle> owner(new soccer_handle());      // every failing exit below destroys the handle
    soccer_handle* h = owner.get();
    h->cfg = *cfg;
    const std::string msg = h->rules.build(cfg->width, cfg->height);
    if (!msg.empty()) return fail(nullptr, SOCCER_E_INVALID, "%s", msg.c_str());
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev < 1)
        return fail(nullptr, SOCCER_E_HIP, "no HIP device available (%s); libsoccer_hip has no CPU path",
                    de == hipSuccess ? "device count is 0" : hipGetErrorString(de));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, SOCCER_E_INVALID, "device %d out of range (0..%d)", cfg->device, ndev - 1);
    HIP_TRY(nullptr, hipSetDevice(cfg->device));
    if (cfg->flags & SOCCER_F_NULL_STREAM) { h->stream = nullptr; h->own_stream = false; }
    else if (cfg->stream) { h->stream = static_cast<hipStream_t>(cfg->stream); h->own_stream = false; }
    else { HIP_TRY(nullptr, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    HIP_TRY(nullptr, hipEventCreate(&h->ev0));
    HIP_TRY(nullptr, hipEventCreate(&h->ev1));

    const Rules& R = h->rules;
    KernelParams& P = h->P;
    const size_t n = cfg->n_lanes;
    const size_t padded = (n + 255) & ~size_t(255);
    h->state_stride = padded;
    h->mapped = (cfg->flags & SOCCER_F_HOST_MAPPED) != 0;
    if (h->mapped && n > 4096) return fail(nullptr, SOCCER_E_INVALID, "SOCCER_F_HOST_MAPPED is for small handles (n_lanes <= 4096)");
    // three packed streams (swar::pack3) where rows fit three bits and columns four; host-mapped handles keep the six that
    // soccer_host_view hands out, and SOCCER_STATE_LAYOUT=wide forces them (tests and A/B runs of the other layout)
    const char* lay = std::getenv("SOCCER_STATE_LAYOUT");
    const bool packed = swar::packs(R.H, R.W) && !h->mapped && !(lay && std::strcmp(lay, "wide") == 0);
    h->state_streams = packed ? 3 : 6;
    const size_t state_bytes = (size_t)h->state_streams * padded;
    if (int rc = h->mapped ? h->bufs.alloc_pinned(nullptr, state_bytes, OwnedBufs::kPinnedMapped, &h->d_state)
                           : h->bufs.alloc(nullptr, state_bytes, &h->d_state)) return rc;
    P.state = h->d_state; P.state_stride = padded; P.state_layout = packed ? kStatePacked : kStateWide;
    // every lane starts needing a reset (:140), parked on the first ISD state so the tuple is valid
    {
        uint8_t init[6] = {(uint8_t)R.isd[0][0], (uint8_t)R.isd[0][1], (uint8_t)R.isd[0][2], (uint8_t)R.isd[0][3], (uint8_t)(2 | R.isd[0][4]), 0};
        if (packed) {
            uint32_t a, b, t;
            swar::pack3(swar::Group{init[0], init[1], init[2], init[3], init[4], init[5]}, a, b, t);
            init[0] = (uint8_t)a; init[1] = (uint8_t)b; init[2] = (uint8_t)t;
        }
        for (int k = 0; k < h->state_streams; ++k) {
            if (h->mapped) std::memset(h->d_state + k * padded, init[k], padded);
            else HIP_TRY(nullptr, hipMemsetAsync(h->d_state + k * padded, init[k], padded, h->stream));
        }
    }

    if (int rc = h->bufs.alloc(nullptr, R.next_cell.size(), &h->d_nc)) return rc;
    if (int rc = h->bufs.alloc(nullptr, sizeof(R.isd_words) / sizeof(uint32_t), &h->d_isd)) return rc;
    HIP_TRY(nullptr, hipMemcpy(h->d_isd, R.isd_words, sizeof(R.isd_words), hipMemcpyHostToDevice));
    HIP_TRY(nullptr, hipMemcpy(h->d_nc, R.next_cell.data(), R.next_cell.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = h->bufs.alloc(nullptr, 256 / sizeof(unsigned long long), &h->d_tick)) return rc;
    HIP_TRY(nullptr, hipMemset(h->d_tick, 0, 256));
    // one private histogram slot per wave of the largest grid that counts episodes: the capped grids (rollout, per-lane
    // step) stay below kHistSlots waves; the byte-parallel step launches one wave per 256 lanes, uncapped
    while (h->hist_slots < (n + 255) / 256) h->hist_slots <<= 1;
    if (int rc = h->bufs.alloc(nullptr, h->hist_slots * kHistStride, &h->d_hist)) return rc;
    HIP_TRY(nullptr, hipMemset(h->d_hist, 0, sizeof(unsigned long long) * h->hist_slots * kHistStride));
    if (int rc = h->bufs.alloc_pinned(nullptr, kMappedBytes / sizeof(unsigned int), OwnedBufs::kPinnedMapped, &h->misuse_host)) return rc;
    std::memset(h->misuse_host, 0, kMappedBytes);
    HIP_TRY(nullptr, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_misuse), h->misuse_host, 0));

    P.next_cell = h->d_nc; P.isd = h->d_isd;
    P.hist = h->d_hist; P.hist_mask = (uint32_t)(h->hist_slots - 1); P.misuse = h->d_misuse;
    P.lane_offset = cfg->lane_offset;
    P.first = 0; P.n = n; P.W = R.W; P.HW = R.H * R.W; P.HW5 = 5 * R.H * R.W;
    P.nc_len = static_cast<int32_t>(R.next_cell.size());
    P.max_steps = cfg->max_steps;
    P.autoreset = (cfg->flags & SOCCER_F_AUTORESET) ? 1u : 0u;
    P.step_stats = (cfg->flags & SOCCER_F_STEP_STATS) ? 1u : 0u;
    P.isd_shift = R.n_isd == 4 ? 0u : 1u;
    // slip-combination weights, the nominal float64 thresholds of the slip fast path and their integer form
    // (soccer_slip.hpp: host-only, shared with the CPU test of the byte-parallel slip step)
    {
        const SlipTables ST = build_slip_tables(cfg->slip_prob);
        for (int i = 0; i < 4; ++i) P.w[i] = ST.w[i];
        for (int i = 0; i < 9; ++i) { P.B[i] = ST.B[i]; P.CB[i] = ST.CB[i]; }
        P.nb = ST.nb; P.act_pack = ST.act_pack; P.slip_int = ST.slip_int;
        static_assert(sizeof(swar::Quad) == sizeof(uint4), "threshold rows are 16 bytes");
        if (int rc = h->bufs.alloc(nullptr, sizeof(ST.sub) / sizeof(uint4), &h->d_sub)) return rc;
        HIP_TRY(nullptr, hipMemcpy(h->d_sub, ST.sub, sizeof(ST.sub), hipMemcpyHostToDevice));
        P.sub = h->d_sub;
        h->slip_swar_ok = ST.swar_ok;
        static_assert(kSlipBuckets == 16384 && kSlipThresholds == 40, "table layout shared with the kernels");
        if (ST.lut_ok) {
            std::vector<uint32_t> img(kSlipLdsWords, 0xFFFFFFFFu);
            std::memcpy(img.data(), ST.lut, kSlipBuckets);
            std::memcpy(img.data() + kSlipBuckets / 4, ST.T, sizeof(ST.T));
            if (int rc = h->bufs.alloc(nullptr, img.size(), &h->d_slip_lut)) return rc;
            HIP_TRY(nullptr, hipMemcpy(h->d_slip_lut, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        if (ST.lut_step_ok && !std::getenv("SOCCER_STEP_SLIP_ONE_BY_ONE")) {      // (the variable: tests and A/B runs of the other form)
            std::vector<uint32_t> img(kSlipStepLdsWords, 0xFFFFFFFFu);
            std::memcpy(img.data(), ST.lut_step, kSlipStepBuckets);
            std::memcpy(img.data() + kSlipStepBuckets / 4, ST.T, sizeof(ST.T));
            if (int rc = h->bufs.alloc(nullptr, img.size(), &h->d_slip_step_lut)) return rc;
            HIP_TRY(nullptr, hipMemcpy(h->d_slip_step_lut, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        {
            const SlipF64 F = make_slip_f64(ST);
            if (int rc = h->bufs.alloc(nullptr, 1, &h->d_slip_f64)) return rc;
            HIP_TRY(nullptr, hipMemcpy(h->d_slip_f64, &F, sizeof F, hipMemcpyHostToDevice));
        }
        h->slip_c = swar::SlipConsts{};
        for (int i = 0; i < 9; ++i) h->slip_c.CB[i] = ST.CB[i];
        h->slip_c.c_off = ST.c_off;
    }
    set_key(h, cfg->seed);
    h->swar_ok = swar::fits(R.H, R.W, cfg->max_steps);
    if (h->swar_ok) h->swar_c = swar::make_consts(R.H, R.W, R.goal_lo, R.goal_hi, cfg->max_steps, R.n_isd, R.isd, P.autoreset != 0u);
    h->slip = cfg->slip_prob != 0.0;
    if (const char* e2 = std::getenv("SOCCER_ROLLOUT")) h->rollout_pref = std::atoi(e2);
    if (const char* e4 = std::getenv("SOCCER_GRAPH_FUSE")) h->graph_fuse = std::atoi(e4) != 0;   // (A/B runs, tests: a launch per captured step)
    if (const char* e3 = std::getenv("SOCCER_SWAR_LAUNCH_LANES")) {
        const unsigned long long v = std::strtoull(e3, nullptr, 10) & ~3ull;
        if (v >= 4ull && v <= kSwarLaunchLanes) h->swar_launch_lanes = v;
    }
    h->E = e ? static_cast<int>(e) : 4;

    // Observation table (uint16 index < 65535 bounds it to a few hundred KB): global for the step kernel,
    // staged into LDS by the rollout / reset kernels when it fits next to the move/bounds table.
    const size_t nc_bytes = (R.next_cell.size() + kIsdWords) * sizeof(uint32_t);
    const size_t lut_bytes = R.lut.size() * sizeof(uint16_t);
    if (nc_bytes > 150 * 1024)
        return fail(nullptr, SOCCER_E_INVALID, "pitch too large: the move/bounds table (%zu bytes) must fit the 160 KB LDS", nc_bytes);
    if (int rc = h->bufs.alloc(nullptr, R.lut.size(), &h->d_lut)) return rc;
    HIP_TRY(nullptr, hipMemcpy(h->d_lut, R.lut.data(), lut_bytes, hipMemcpyHostToDevice));
    P.lut = h->d_lut; P.lut_len = static_cast<int32_t>(R.lut.size());
    h->lut_lds = nc_bytes + lut_bytes <= 150 * 1024;
    h->smem_bytes = nc_bytes + (h->lut_lds ? lut_bytes : 0);
    if (h->smem_bytes > 48 * 1024) {
        const size_t b = h->smem_bytes;
        hipError_t se = rollout_raise_smem_limit(h, b);
        if (se == hipSuccess)
            se = with_shape(h, [&](auto slip, auto lds) {
                return hipFuncSetAttribute(reinterpret_cast<const void*>(&reset_kernel<decltype(lds)::value, decltype(slip)::value>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
            });
        HIP_TRY(nullptr, se);
    }
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, cfg->device));
    { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device) == hipSuccess && khz > 0) h->wall_clock_khz = khz; }
    h->grid_cap = prop.multiProcessorCount * 8;
    h->n_cu = prop.multiProcessorCount;
    if (prop.sharedMemPerBlockOptin > 0) h->lds_limit = prop.sharedMemPerBlockOptin;
    else if (prop.sharedMemPerBlock > 0) h->lds_limit = prop.sharedMemPerBlock;
    HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
    HIP_TRY(nullptr, hipDeviceSynchronize());      // the hipMemset / hipMemcpy calls above went to the null stream, which a non-blocking stream does not wait for
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_destroy(soccer_handle* h) {
    delete h;
    return SOCCER_OK;
}

extern "C" int soccer_sync(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_sync during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_seed(soccer_handle* h, uint64_t seed) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_seed during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    set_key(h, seed);
    h->tick = 0;
    HIP_TRY(h, hipMemsetAsync(h->d_tick, 0, 256, h->stream));
    return SOCCER_OK;
}

extern "C" uint64_t soccer_tick(const soccer_handle* h) { return h ? h->tick : 0; }

// checkpoint / resume: (state streams, seed, tick) fully determine every later result
extern "C" int soccer_set_tick(soccer_handle* h, uint64_t tick) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_set_tick during graph capture");
    if (tick >> 63) return fail(h, SOCCER_E_INVALID, "tick must be below 2^63");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    unsigned long long slots[32] = {0};
    slots[0] = tick; slots[16] = tick;
    HIP_TRY(h, hipMemcpy(h->d_tick, slots, sizeof slots, hipMemcpyHostToDevice));
    h->tick = tick;
    return SOCCER_OK;
}
extern "C" uint64_t soccer_get_seed(const soccer_handle* h) { return h ? h->cfg.seed : 0; }

// ------------------------------------------------------------------------------------------------
extern "C" int batched_reset(soccer_handle* h, const uint8_t* mask, const double* u_reset, uint16_t* obs) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!aligned(u_reset, 8) || !aligned(obs, 2))
        return fail(h, SOCCER_E_INVALID, "batched_reset: u_reset must be 8-byte and obs 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = flush_pending(h)) return rc;       // captured steps before this call come first
    KernelParams P = h->P;
    bind_tick(h, P, 1);
    ResetIO io{mask, u_reset, obs};
    // the byte-parallel kernel over the 4-aligned part (Philox draws, dword-aligned streams); whatever is left — a ragged
    // tail, or everything — through the per-lane kernel on the same tick
    const ResetPlan R = plan_reset(handle_facts(h), ResetCall{mask != nullptr, u_reset != nullptr, aligned(mask, 4) && aligned(obs, 8)});
    const unsigned long long n4 = R.n4;
    if (n4) {
        ResetSwar RS{h->swar_c, P.state, P.state_stride, P.state_layout, n4, P.lane_offset, P.tick_in, P.tick_out, P.key0, P.key1, mask, obs};
        const dim3 g(static_cast<unsigned>(((n4 >> 2) + kBlock - 1) / kBlock)), b(kBlock);
        with_flag(R.masked, [&](auto masked) { with_flag(R.slip, [&](auto slip) {
            hipLaunchKernelGGL((reset_kernel_swar<decltype(masked)::value, decltype(slip)::value>), g, b, 0, h->stream, RS);
        }); });
        note_kernel(h);
    }
    if (n4 < P.n) {
        KernelParams Q = P;
        Q.first = n4; Q.n = P.n - n4;
        if (n4) Q.tick_out = nullptr;           // the main launch publishes the tick
        const dim3 g(grid_for(h, Q.n)), b(kBlock);
        with_flag(R.lut_lds, [&](auto lds) { with_flag(R.slip, [&](auto slip) {
            hipLaunchKernelGGL((reset_kernel<decltype(lds)::value, decltype(slip)::value>), g, b, h->smem_bytes, h->stream, Q, io);
        }); });
        note_kernel(h);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// the handle's state as six host streams of stride state_stride, whatever its layout (`img` holds 6 * state_stride bytes): one
// copy, then the packed streams are taken apart in place (a lane's three bytes are read before any of its six is written)
static int fetch_state(soccer_handle* h, std::vector<uint8_t>& img) {
    const size_t n = h->P.n, S = h->state_stride, bytes = (size_t)h->state_streams * S;
    if (h->mapped) std::memcpy(img.data(), h->d_state, bytes);
    else HIP_TRY(h, hipMemcpy(img.data(), h->d_state, bytes, hipMemcpyDeviceToHost));
    if (h->state_streams == 3) {
        for (size_t i = 0; i < n; ++i) {
            swar::Group G;
            swar::unpack3(img[i], img[S + i], img[2 * S + i], G);
            img[5 * S + i] = (uint8_t)G.tt; img[4 * S + i] = (uint8_t)G.ps; img[3 * S + i] = (uint8_t)G.cb;
            img[2 * S + i] = (uint8_t)G.rb; img[S + i] = (uint8_t)G.ca; img[i] = (uint8_t)G.ra;
        }
    }
    return SOCCER_OK;
}

extern "C" int soccer_state_streams(const soccer_handle* h) { return h ? h->state_streams : 0; }

extern "C" int soccer_set_state(soccer_handle* h, const int8_t* row_a, const int8_t* col_a, const int8_t* row_b,
                                const int8_t* col_b, const uint8_t* poss, const uint8_t* t,
                                const uint8_t* needs_reset) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_set_state during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t n = h->P.n, S = h->state_stride;
    const Rules& R = h->rules;
    // current device copy of whatever is not supplied, so the resulting tuple can be validated
    std::vector<uint8_t> img(6 * S);
    if (int rc = fetch_state(h, img)) return rc;
    int8_t* ra = reinterpret_cast<int8_t*>(img.data());
    int8_t* ca = ra + S; int8_t* rb = ra + 2 * S; int8_t* cb = ra + 3 * S;
    uint8_t* ps = img.data() + 4 * S; uint8_t* tt = img.data() + 5 * S;
    for (size_t i = 0; i < n; ++i) {
        if (row_a) ra[i] = row_a[i];
        if (col_a) ca[i] = col_a[i];
        if (row_b) rb[i] = row_b[i];
        if (col_b) cb[i] = col_b[i];
        uint8_t p = ps[i] & 1, nr = (ps[i] >> 1) & 1;
        if (poss) { if (poss[i] > 1) return fail(h, SOCCER_E_INVALID, "lane %zu: possession must be 0 or 1", i); p = poss[i]; }
        if (needs_reset) nr = needs_reset[i] ? 1 : 0;
        ps[i] = static_cast<uint8_t>(p | (nr << 1));
        if (t) { if (t[i] > h->cfg.max_steps) return fail(h, SOCCER_E_INVALID, "lane %zu: timestep %d > max_steps", i, (int)t[i]); tt[i] = t[i]; }
        const bool in_range = ra[i] >= 0 && ra[i] < R.H && rb[i] >= 0 && rb[i] < R.H &&
                              ca[i] >= 0 && ca[i] < R.W && cb[i] >= 0 && cb[i] < R.W;
        // the reference raises KeyError when stepping from a tuple it has no table entry for
        if (!in_range || R.kind[R.flat(ra[i], ca[i], rb[i], cb[i], p)] == 0)
            return fail(h, SOCCER_E_INVALID, "lane %zu: state (%d, %d, %d, %d, %d) is not a reachable state tuple",
                        i, (int)ra[i], (int)ca[i], (int)rb[i], (int)cb[i], (int)p);
    }
    if (h->state_streams == 3) {                    // validated above: rows < H <= 8, columns < W <= 16
        for (size_t i = 0; i < n; ++i) {
            uint32_t a, b, t_;
            swar::pack3(swar::Group{(uint8_t)ra[i], (uint8_t)ca[i], (uint8_t)rb[i], (uint8_t)cb[i], ps[i], tt[i]}, a, b, t_);
            img[i] = (uint8_t)a; img[S + i] = (uint8_t)b; img[2 * S + i] = (uint8_t)t_;
        }
    }
    const size_t bytes = (size_t)h->state_streams * S;
    if (h->mapped) std::memcpy(h->d_state, img.data(), bytes);
    else HIP_TRY(h, hipMemcpy(h->d_state, img.data(), bytes, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

extern "C" int soccer_host_view(soccer_handle* h, uint8_t** state, uint64_t* stride) {
    if (!h || !state || !stride) return fail(h, SOCCER_E_INVALID, "handle/state/stride is NULL");
    if (!h->mapped) return fail(h, SOCCER_E_STATE, "soccer_host_view needs a SOCCER_F_HOST_MAPPED handle");
    *state = h->d_state; *stride = h->state_stride;
    return SOCCER_OK;
}

extern "C" int soccer_get_state(soccer_handle* h, int8_t* row_a, int8_t* col_a, int8_t* row_b, int8_t* col_b,
                                uint8_t* poss, uint8_t* t, uint8_t* needs_reset) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_get_state during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t n = h->P.n, S = h->state_stride;
    std::vector<uint8_t> img(6 * S);
    if (int rc = fetch_state(h, img)) return rc;
    if (row_a) std::memcpy(row_a, img.data(), n);
    if (col_a) std::memcpy(col_a, img.data() + S, n);
    if (row_b) std::memcpy(row_b, img.data() + 2 * S, n);
    if (col_b) std::memcpy(col_b, img.data() + 3 * S, n);
    if (t) std::memcpy(t, img.data() + 5 * S, n);
    const uint8_t* ps = img.data() + 4 * S;
    for (size_t i = 0; i < n; ++i) {
        if (poss) poss[i] = ps[i] & 1;
        if (needs_reset) needs_reset[i] = (ps[i] >> 1) & 1;
    }
    return SOCCER_OK;
}

// ---- host-pointer entry points: stage through one pinned block, one copy each way ---------------
namespace {
struct StageLayout {
    size_t act_a, act_b, mask, u_step, u_reset;            // inputs (the action streams first: they always travel)
    size_t obs, final_obs, reward, term, trunc, code;      // outputs
    size_t out_begin, total;
};
StageLayout stage_layout(size_t n) {
    auto up = [](size_t x) { return (x + 63) & ~size_t(63); };
    StageLayout L{};
    size_t o = 0;
    L.act_a = o; o = up(o + n);
    L.act_b = o; o = up(o + n);
    L.mask = o; o = up(o + n);
    L.u_step = o; o = up(o + 8 * n);
    L.u_reset = o; o = up(o + 8 * n);
    L.out_begin = o;
    L.obs = o; o = up(o + 2 * n);
    L.final_obs = o; o = up(o + 2 * n);
    L.reward = o; o = up(o + n);
    L.term = o; o = up(o + n);
    L.trunc = o; o = up(o + n);
    L.code = o; o = up(o + n);
    L.total = o;
    return L;
}
int ensure_stage(soccer_handle* h, const StageLayout& L) {
    if (h->stage_bytes >= L.total) return SOCCER_OK;
    // both halves or neither.  Mapped: the kernel reads inputs from / writes outputs to the pinned block in place
    uint8_t* host = nullptr; uint8_t* dev = nullptr;
    if (int rc = h->bufs.alloc_pinned(h, L.total, h->mapped ? OwnedBufs::kPinnedMapped : OwnedBufs::kPinned, &host)) return rc;
    if (h->mapped) dev = host;
    else if (int rc = h->bufs.alloc(h, L.total, &dev)) { h->bufs.release(host); return rc; }
    h->stage_host = host; h->stage_dev = dev; h->stage_bytes = L.total;
    return SOCCER_OK;
}
}  // namespace

extern "C" int soccer_staging(soccer_handle* h, soccer_staging_view* v) {
    if (!h || !v) return fail(h, SOCCER_E_INVALID, "handle/view is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const StageLayout L = stage_layout(h->P.n);
    if (int rc = ensure_stage(h, L)) return rc;
    uint8_t* H = h->stage_host;
    v->act_a = reinterpret_cast<int8_t*>(H + L.act_a); v->act_b = reinterpret_cast<int8_t*>(H + L.act_b);
    v->mask = H + L.mask;
    v->u_step = reinterpret_cast<double*>(H + L.u_step); v->u_reset = reinterpret_cast<double*>(H + L.u_reset);
    v->obs = reinterpret_cast<uint16_t*>(H + L.obs); v->final_obs = reinterpret_cast<uint16_t*>(H + L.final_obs);
    v->reward = reinterpret_cast<int8_t*>(H + L.reward); v->terminated = H + L.term; v->truncated = H + L.trunc;
    v->prob_code = H + L.code;
    return SOCCER_OK;
}

// every action byte of a host array must be 0..4 (the reference indexes ACTION_STRING with it: IndexError, :393)
static long first_bad_action(const int8_t* a, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {                    // eight bytes at a time: any bit above 2 set, or 5..7
        uint64_t v; std::memcpy(&v, a + i, 8);
        if ((v & 0xF8F8F8F8F8F8F8F8ull) | (((v & 0x0707070707070707ull) + 0x0303030303030303ull) & 0x0808080808080808ull)) break;
    }
    for (; i < n; ++i) if (a[i] < 0 || a[i] > 4) return (long)i;
    return -1;
}

extern "C" int batched_step_staged(soccer_handle* h, uint32_t use) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "batched_step_staged during graph capture");
    const bool has_a = use & SOCCER_STAGE_ACT_A, has_b = use & SOCCER_STAGE_ACT_B;
    if ((!has_a && !h->P.policy_a) || (!has_b && !h->P.policy_b))
        return fail(h, SOCCER_E_INVALID, "batched_step: an action stream is required for every player without a fixed policy");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = h->P.n;
    const StageLayout L = stage_layout(n);
    if (int rc = ensure_stage(h, L)) return rc;
    uint8_t* H = h->stage_host; uint8_t* D = h->stage_dev;
    for (int pl = 0; pl < 2; ++pl) {
        if (!(pl ? has_b : has_a)) continue;
        const long bad = first_bad_action(reinterpret_cast<const int8_t*>(H + (pl ? L.act_b : L.act_a)), n);
        if (bad >= 0) return fail(h, SOCCER_E_INVALID, "batched_step: action of player_%c in lane %ld is %d; actions must be in 0..4",
                                  pl ? 'b' : 'a', bad, (int)reinterpret_cast<const int8_t*>(H + (pl ? L.act_b : L.act_a))[bad]);
    }
    if (!h->mapped) {           // only what this call uses crosses the bus
        if (has_a && has_b) HIP_TRY(h, hipMemcpyAsync(D + L.act_a, H + L.act_a, L.act_b + n - L.act_a, hipMemcpyHostToDevice, h->stream));
        else if (has_a) HIP_TRY(h, hipMemcpyAsync(D + L.act_a, H + L.act_a, n, hipMemcpyHostToDevice, h->stream));
        else if (has_b) HIP_TRY(h, hipMemcpyAsync(D + L.act_b, H + L.act_b, n, hipMemcpyHostToDevice, h->stream));
        if (use & SOCCER_STAGE_U_STEP) HIP_TRY(h, hipMemcpyAsync(D + L.u_step, H + L.u_step, 8 * n, hipMemcpyHostToDevice, h->stream));
        if (use & SOCCER_STAGE_U_RESET) HIP_TRY(h, hipMemcpyAsync(D + L.u_reset, H + L.u_reset, 8 * n, hipMemcpyHostToDevice, h->stream));
    }
    soccer_step_args d{};
    d.act_a = has_a ? reinterpret_cast<const int8_t*>(D + L.act_a) : nullptr;
    d.act_b = has_b ? reinterpret_cast<const int8_t*>(D + L.act_b) : nullptr;
    d.u_step = (use & SOCCER_STAGE_U_STEP) ? reinterpret_cast<const double*>(D + L.u_step) : nullptr;
    d.u_reset = (use & SOCCER_STAGE_U_RESET) ? reinterpret_cast<const double*>(D + L.u_reset) : nullptr;
    d.obs = reinterpret_cast<uint16_t*>(D + L.obs); d.final_obs = reinterpret_cast<uint16_t*>(D + L.final_obs);
    d.reward = reinterpret_cast<int8_t*>(D + L.reward); d.terminated = D + L.term; d.truncated = D + L.trunc;
    d.prob_code = D + L.code;
    if (int rc = batched_step_ex(h, &d)) return rc;
    if (!h->mapped) HIP_TRY(h, hipMemcpyAsync(H + L.out_begin, D + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int batched_reset_staged(soccer_handle* h, uint32_t use) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "batched_reset_staged during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = h->P.n;
    const StageLayout L = stage_layout(n);
    if (int rc = ensure_stage(h, L)) return rc;
    uint8_t* H = h->stage_host; uint8_t* D = h->stage_dev;
    if (!h->mapped) {
        if (use & SOCCER_STAGE_MASK) HIP_TRY(h, hipMemcpyAsync(D + L.mask, H + L.mask, n, hipMemcpyHostToDevice, h->stream));
        if (use & SOCCER_STAGE_U_RESET) HIP_TRY(h, hipMemcpyAsync(D + L.u_reset, H + L.u_reset, 8 * n, hipMemcpyHostToDevice, h->stream));
    }
    if (int rc = batched_reset(h, (use & SOCCER_STAGE_MASK) ? D + L.mask : nullptr,
                               (use & SOCCER_STAGE_U_RESET) ? reinterpret_cast<const double*>(D + L.u_reset) : nullptr,
                               reinterpret_cast<uint16_t*>(D + L.obs))) return rc;
    if (!h->mapped) HIP_TRY(h, hipMemcpyAsync(H + L.obs, D + L.obs, 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// one environment, one call: inputs by value, result polled from a mapped record (see scalar_kernel)
static int scalar_call(soccer_handle* h, const char* what, uint32_t op, soccer_scalar_io* io) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!io) return fail(h, SOCCER_E_INVALID, "%s: io is NULL", what);
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (h->P.n != 1) return fail(h, SOCCER_E_INVALID, "%s needs a handle with n_lanes == 1", what);
    const Rules& R = h->rules;
    ScalarIO k{};
    k.op = op; k.u_step = io->u_step; k.u_reset = io->u_reset;
    if (op == 0u) {
        if (io->needs_reset) return fail(h, SOCCER_E_INVALID, "Please reset the environment before taking a step");   // :376
        const int ra = io->row_a, ca = io->col_a, rb = io->row_b, cb = io->col_b;
        if (ra < 0 || ra >= R.H || rb < 0 || rb >= R.H || ca < 0 || ca >= R.W || cb < 0 || cb >= R.W || io->poss > 1)
            return fail(h, SOCCER_E_INVALID, "%s: tuple (%d, %d, %d, %d, %d) is outside the pitch", what, ra, ca, rb, cb, (int)io->poss);
        if (R.kind[((((size_t)ra * R.W + ca) * R.H + rb) * R.W + cb) * 2 + io->poss] == 0)
            return fail(h, SOCCER_E_INVALID, "%s: tuple (%d, %d, %d, %d, %d) is unreachable", what, ra, ca, rb, cb, (int)io->poss);
        if ((int)io->t > h->cfg.max_steps) return fail(h, SOCCER_E_INVALID, "%s: t = %d exceeds max_steps", what, (int)io->t);
        if ((!h->P.policy_a && (io->act_a < 0 || io->act_a > 4)) || (!h->P.policy_b && (io->act_b < 0 || io->act_b > 4)))
            return fail(h, SOCCER_E_INVALID, "%s: actions must be in 0..4", what);
        k.pos = (uint32_t)ra | ((uint32_t)ca << 8) | ((uint32_t)rb << 16) | ((uint32_t)cb << 24);
        k.misc = (uint32_t)io->poss | ((uint32_t)io->t << 8) | ((uint32_t)(uint8_t)io->act_a << 16) | ((uint32_t)(uint8_t)io->act_b << 24);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->rec_host) {
        uint4* rec = nullptr;
        if (int rc = h->bufs.alloc_pinned(h, 64 / sizeof(uint4), OwnedBufs::kPinnedMapped, &rec)) return rc;
        std::memset(rec, 0, 64);
        const hipError_t e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->rec_dev), rec, 0);
        if (e != hipSuccess) { h->bufs.release(rec); return fail(h, SOCCER_E_HIP, "%s: no device address for the result record: %s", what, hipGetErrorString(e)); }
        h->rec_host = rec;
    }
    k.seq = ++h->rec_seq ? h->rec_seq : ++h->rec_seq;                    // never 0
    k.record = h->rec_dev;
    KernelParams P = h->P;
    bind_tick(h, P, 1);
    with_flag(h->slip, [&](auto slip) { hipLaunchKernelGGL(scalar_kernel<decltype(slip)::value>, dim3(1), dim3(64), 0, h->stream, P, k); });
    HIP_TRY(h, hipGetLastError());
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(h->rec_host);
    const auto t_start = std::chrono::steady_clock::now();
    // complete record: word 0 == seq and the top byte of word 3 == seq's low byte (both ends of the one store)
    // ... and the check byte in word 3 is the byte-sum of words 1 and 2, so a record of which only some dwords have
    // landed is never accepted (soccer_hip.h, soccer_step_scalar)
    auto byte_sum = [](uint32_t a, uint32_t b) { uint32_t s_ = 0; for (int q = 0; q < 4; ++q) s_ += ((a >> (8 * q)) & 0xffu) + ((b >> (8 * q)) & 0xffu); return s_ & 0xffu; };
    auto landed = [&]() {
        const uint32_t f0 = flag[0], f1 = flag[1], f2 = flag[2], f3 = flag[3];
        return f0 == k.seq && (f3 >> 24) == (k.seq & 0xffu) && ((f3 >> 16) & 0xffu) == byte_sum(f1, f2);
    };
    for (uint32_t spins = 0; !landed(); ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xfffffu) == 0xfffffu) {                            // every few ms: has the stream died?
            const hipError_t e = hipStreamQuery(h->stream);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(h, SOCCER_E_HIP, "%s: %s", what, hipGetErrorString(e));
            if (e == hipSuccess && !landed()) return fail(h, SOCCER_E_HIP, "%s: the kernel finished without publishing its record", what);
            if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(30))
                return fail(h, SOCCER_E_HIP, "%s: no result after 30 s (is another stream hogging the device?)", what);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const volatile uint32_t* r = flag;
    const uint32_t res = r[1], npos = r[2], nm = r[3];
    io->obs = (uint16_t)(res & 0xffffu); io->reward = (int8_t)((res >> 16) & 0xffu);
    io->terminated = (res >> 24) & 1u; io->truncated = (res >> 25) & 1u; io->prob_code = (uint8_t)(res >> 26);
    io->row_a = (int8_t)(npos & 0xffu); io->col_a = (int8_t)((npos >> 8) & 0xffu);
    io->row_b = (int8_t)((npos >> 16) & 0xffu); io->col_b = (int8_t)(npos >> 24);
    io->poss = nm & 1u; io->needs_reset = (nm >> 1) & 1u; io->t = (uint8_t)((nm >> 8) & 0xffu);
    return SOCCER_OK;
}

extern "C" int soccer_step_scalar(soccer_handle* h, soccer_scalar_io* io) { return scalar_call(h, "soccer_step_scalar", 0u, io); }
extern "C" int soccer_reset_scalar(soccer_handle* h, soccer_scalar_io* io) { return scalar_call(h, "soccer_reset_scalar", 1u, io); }

// host arrays in, host arrays out: copies through the staging block around the *_staged calls
extern "C" int batched_step_host(soccer_handle* h, const soccer_step_args* a) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!a) return fail(h, SOCCER_E_INVALID, "batched_step: arguments are NULL");
    if (a->last_return || a->reward_a_f32 || a->reward_b_f32 || a->finished)
        return fail(h, SOCCER_E_INVALID, "batched_step_host: last_return / reward_*_f32 / finished are device-only");
    soccer_staging_view v{};
    if (int rc = soccer_staging(h, &v)) return rc;
    const size_t n = h->P.n;
    uint32_t use = 0;
    if (a->act_a) { std::memcpy(v.act_a, a->act_a, n); use |= SOCCER_STAGE_ACT_A; }
    if (a->act_b) { std::memcpy(v.act_b, a->act_b, n); use |= SOCCER_STAGE_ACT_B; }
    if (a->u_step) { std::memcpy(v.u_step, a->u_step, 8 * n); use |= SOCCER_STAGE_U_STEP; }
    if (a->u_reset) { std::memcpy(v.u_reset, a->u_reset, 8 * n); use |= SOCCER_STAGE_U_RESET; }
    if (int rc = batched_step_staged(h, use)) return rc;
    if (a->obs) std::memcpy(a->obs, v.obs, 2 * n);
    if (a->final_obs) std::memcpy(a->final_obs, v.final_obs, 2 * n);
    if (a->reward) std::memcpy(a->reward, v.reward, n);
    if (a->terminated) std::memcpy(a->terminated, v.terminated, n);
    if (a->truncated) std::memcpy(a->truncated, v.truncated, n);
    if (a->prob_code) std::memcpy(a->prob_code, v.prob_code, n);
    return SOCCER_OK;
}

extern "C" int batched_reset_host(soccer_handle* h, const uint8_t* mask, const double* u_reset, uint16_t* obs) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    soccer_staging_view v{};
    if (int rc = soccer_staging(h, &v)) return rc;
    const size_t n = h->P.n;
    uint32_t use = 0;
    if (mask) { std::memcpy(v.mask, mask, n); use |= SOCCER_STAGE_MASK; }
    if (u_reset) { std::memcpy(v.u_reset, u_reset, 8 * n); use |= SOCCER_STAGE_U_RESET; }
    if (int rc = batched_reset_staged(h, use)) return rc;
    if (obs) std::memcpy(obs, v.obs, 2 * n);
    return SOCCER_OK;
}


// single-agent mode: one side follows a fixed policy looked up by the current observation index
// (reference :54-56, :187-188).  policy_host NULL clears it.
extern "C" int soccer_set_policy(soccer_handle* h, int32_t player, const int8_t* policy_host, int32_t n_states) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_set_policy during graph capture");
    if (player != 0 && player != 1) return fail(h, SOCCER_E_INVALID, "player must be 0 (player_a) or 1 (player_b)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int8_t** slot = player == 0 ? &h->P.policy_a : &h->P.policy_b;
    h->plan_bufs.clear();
    if (!policy_host) { *slot = nullptr; return SOCCER_OK; }
    if (n_states != h->rules.nS) return fail(h, SOCCER_E_INVALID, "policy must have one action per observation index (%d)", h->rules.nS);
    if ((player == 0 ? h->P.policy_b : h->P.policy_a) != nullptr)
        return fail(h, SOCCER_E_INVALID, "Both players cannot have a policy. At least one must be None.");   // :38
    for (int i = 0; i < n_states; ++i)
        if (policy_host[i] < 0 || policy_host[i] > 4) return fail(h, SOCCER_E_INVALID, "policy[%d] = %d is not an action", i, (int)policy_host[i]);
    if (!h->d_policy[player]) if (int rc = h->bufs.alloc(h, (size_t)h->rules.nS, &h->d_policy[player])) return rc;
    HIP_TRY(h, hipMemcpy(h->d_policy[player], policy_host, (size_t)n_states, hipMemcpyHostToDevice));
    *slot = h->d_policy[player];
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int soccer_dims(const soccer_handle* h, int32_t* n_states, int32_t* lut_len, int32_t* n_isd,
                           int32_t* internal_width) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (n_states) *n_states = h->rules.nS;
    if (lut_len) *lut_len = static_cast<int32_t>(h->rules.lut.size());
    if (n_isd) *n_isd = h->rules.n_isd;
    if (internal_width) *internal_width = h->rules.W;
    return SOCCER_OK;
}

extern "C" int soccer_get_tables(const soccer_handle* h, uint16_t* lut, int8_t* goal_value, int8_t* isd_states) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    const Rules& R = h->rules;
    if (lut) std::memcpy(lut, R.lut.data(), R.lut.size() * sizeof(uint16_t));
    if (goal_value) std::memcpy(goal_value, R.goal_value.data(), R.goal_value.size());
    if (isd_states) for (int i = 0; i < R.n_isd; ++i) for (int k = 0; k < 5; ++k) isd_states[i * 5 + k] = R.isd[i][k];
    return SOCCER_OK;
}

extern "C" int soccer_prob_table(const soccer_handle* h, double prob[12]) {
    if (!h || !prob) return fail(nullptr, SOCCER_E_INVALID, "handle/prob is NULL");
    static const double nsp[3] = {1.0, 0.5, 0.25};
    for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) prob[c * 3 + k] = h->P.w[c] * nsp[k];   // :241
    return SOCCER_OK;
}

extern "C" int soccer_get_stats(soccer_handle* h, uint64_t hist[3], uint64_t* misuse) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_get_stats during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (hist) {
        std::vector<unsigned long long> shards(h->hist_slots * kHistStride);
        HIP_TRY(h, hipMemcpy(shards.data(), h->d_hist, shards.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        hist[0] = hist[1] = hist[2] = 0;
        for (size_t s = 0; s < h->hist_slots; ++s) for (int b = 0; b < 3; ++b) hist[b] += shards[s * kHistStride + b];
    }
    if (misuse) {                                   // the stream is idle: no copy needed
        const volatile unsigned int* m = h->misuse_host;
        *misuse = (m[0] ? 1u : 0u) | (m[1] ? 2u : 0u) | (m[2] ? 4u : 0u);
    }
    return SOCCER_OK;
}

extern "C" uint32_t soccer_peek_misuse(const soccer_handle* h) {
    if (!h || !h->misuse_host) return 0u;
    const volatile unsigned int* m = h->misuse_host;
    return (m[0] ? SOCCER_MISUSE_FROZEN : 0u) | (m[1] ? SOCCER_MISUSE_ACTION : 0u) | (m[2] ? SOCCER_MISUSE_OBSERVATION : 0u);
}

extern "C" int soccer_reset_stats(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = flush_pending(h)) return rc;
    HIP_TRY(h, hipMemsetAsync(h->d_hist, 0, sizeof(unsigned long long) * h->hist_slots * kHistStride, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_misuse, 0, 64, h->stream));
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int soccer_malloc(soccer_handle* h, size_t bytes, void** dptr) {
    if (!h || !dptr) return fail(h, SOCCER_E_INVALID, "handle/dptr is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMalloc(dptr, bytes ? bytes : 1));
    return SOCCER_OK;
}
extern "C" int soccer_free(soccer_handle* h, void* dptr) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (dptr) HIP_TRY(h, hipFree(dptr));
    return SOCCER_OK;
}
extern "C" int soccer_memcpy_h2d(soccer_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_memcpy_h2d during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}
extern "C" int soccer_memcpy_d2h(soccer_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_memcpy_d2h during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}
extern "C" int soccer_memset(soccer_handle* h, void* dst, int value, size_t bytes) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = flush_pending(h)) return rc;
    HIP_TRY(h, hipMemsetAsync(dst, value, bytes, h->stream));
    return SOCCER_OK;
}

// Inside a graph capture an event record becomes a node that carries no timestamp (hipEventElapsedTime refuses such
// events), so a captured timer_start / timer_mark is a one-thread kernel that stores the device's constant-rate wall clock
// into the handle's host-mapped block instead; soccer_timer_read converts the difference.
__global__ void stamp_kernel(unsigned long long* slot) {
    if (threadIdx.x == 0) *slot = wall_clock64();
}

static volatile unsigned long long* stamp_host(soccer_handle* h) {
    return reinterpret_cast<volatile unsigned long long*>(reinterpret_cast<uint8_t*>(h->misuse_host) + 64);
}
static unsigned long long* stamp_dev(soccer_handle* h) {
    return reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(h->d_misuse) + 64);
}

extern "C" int soccer_stamp(soccer_handle* h, int32_t slot) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (slot < 0 || slot >= SOCCER_STAMP_SLOTS) return fail(h, SOCCER_E_INVALID, "stamp slot %d out of range (0..%d)", slot, SOCCER_STAMP_SLOTS - 1);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = flush_pending(h)) return rc;       // (a captured soccer_timer_start / _mark comes through here too)
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, h->stream, stamp_dev(h) + kStampStride * slot);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_stamps_clear(soccer_handle* h, int32_t first, int32_t count) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (first < 0 || count < 0 || first + count > SOCCER_STAMP_SLOTS) return fail(h, SOCCER_E_INVALID, "stamp range out of bounds");
    for (int32_t i = 0; i < count; ++i) stamp_host(h)[kStampStride * (first + i)] = 0ull;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    return SOCCER_OK;
}

extern "C" int soccer_stamps_read(soccer_handle* h, int32_t first, int32_t count, uint64_t* ticks, int32_t* khz) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (first < 0 || count < 0 || first + count > SOCCER_STAMP_SLOTS || (count && !ticks)) return fail(h, SOCCER_E_INVALID, "stamp range out of bounds");
    for (int32_t i = 0; i < count; ++i) ticks[i] = stamp_host(h)[kStampStride * (first + i)];
    if (khz) *khz = h->wall_clock_khz;
    return SOCCER_OK;
}

extern "C" int soccer_timer_start(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    h->timer_stamped = h->capturing;
    if (h->capturing) { h->capture_stamped = true; return soccer_stamp(h, 0); }
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    return SOCCER_OK;
}
extern "C" int soccer_timer_mark(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->capturing) {
        if (!h->capture_stamped) return fail(h, SOCCER_E_STATE, "soccer_timer_mark in a capture needs soccer_timer_start in the same capture");
        return soccer_stamp(h, 1);
    }
    h->timer_stamped = false;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    return SOCCER_OK;
}
extern "C" int soccer_timer_read(soccer_handle* h, float* elapsed_ms) {
    if (!h || !elapsed_ms) return fail(h, SOCCER_E_INVALID, "handle/elapsed_ms is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_timer_read during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->timer_stamped) {                 // the stamps of the last replay of a graph that captured start / mark
        volatile unsigned long long* st = stamp_host(h);
        if (h->stamp_poll) {
            // The closing stamp's kernel writes it to host-mapped memory and clock values only grow: watching that word
            // change from what it held when the (single) replay was enqueued costs no runtime call at all — the host
            // sees the end of the region ~1 us after the device reaches it — and the host never WRITES the stamp lines.  (The runtime's own completion signal of the replay arrives ~13 us after the last
            // kernel on an MI355X — the write-back of the dirty L2 lines and the signal path, tools/labs/sync_cost.py — whether
            // one waits for it in hipStreamSynchronize, in hipDeviceSynchronize or by polling an event recorded behind
            // the replay; a host that only needs the device time does not have to.)
            const auto t_start = std::chrono::steady_clock::now();
            for (uint32_t spins = 0; st[kStampStride] == h->stamp_prev; ++spins) {
                __builtin_ia32_pause();
                if ((spins & 0xfffffu) == 0xfffffu) {                    // every few ms: has the stream died?
                    const hipError_t e = hipStreamQuery(h->stream);
                    if (e != hipSuccess && e != hipErrorNotReady) return fail(h, SOCCER_E_HIP, "soccer_timer_read: %s", hipGetErrorString(e));
                    if (e == hipSuccess && st[kStampStride] == h->stamp_prev) return fail(h, SOCCER_E_STATE, "soccer_timer_read: the stream is idle but the closing stamp was never written");
                    if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(60))
                        return fail(h, SOCCER_E_HIP, "soccer_timer_read: no closing stamp after 60 s");
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        } else {
            for (uint32_t spins = 0;; ++spins) {
                const hipError_t q = hipStreamQuery(h->stream);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) return fail(h, SOCCER_E_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
                if (spins > 2000u) { (void)hipGetLastError(); HIP_TRY(h, hipStreamSynchronize(h->stream)); break; }
                __builtin_ia32_pause();
            }
            (void)hipGetLastError();
        }
        *elapsed_ms = (float)((double)(st[kStampStride] - st[0]) / (double)h->wall_clock_khz);
        return SOCCER_OK;
    }
    // poll instead of blocking: a blocked waiter is woken tens of microseconds after the event completes, which is
    // as long as the whole timed region of a short run
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(h->ev1);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(h, SOCCER_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        if (spins > 2000u) { (void)hipGetLastError(); HIP_TRY(h, hipEventSynchronize(h->ev1)); break; }   // long waits: block
        __builtin_ia32_pause();
    }
    (void)hipGetLastError();
    HIP_TRY(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return SOCCER_OK;
}
extern "C" int soccer_timer_stop(soccer_handle* h, float* elapsed_ms) {
    if (int rc = soccer_timer_mark(h)) return rc;
    return soccer_timer_read(h, elapsed_ms);
}

// ------------------------------------------------------------------------------------------------
__global__ void move_tick_kernel(unsigned long long* dst, const unsigned long long* src) {
    if (threadIdx.x == 0) *dst = *src;
}

extern "C" int soccer_graph_begin(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "graph capture already in progress");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    h->capturing = true; h->capture_ticks = 0; h->capture_calls = 0; h->capture_stamped = false;
    h->capture_start_slot = h->tick_slot;
    h->run = PendingRun{}; h->capture_kernels = 0; h->capture_steps_fused = 0; h->capture_fused_launches = 0;
    return SOCCER_OK;
}

extern "C" int soccer_graph_end(soccer_handle* h, soccer_graph** out) {
    if (!h || !out) return fail(h, SOCCER_E_INVALID, "handle/out is NULL");
    if (!h->capturing) return fail(h, SOCCER_E_STATE, "no graph capture in progress");
    if (const int rc = flush_pending(h)) {
        // the last run could not be recorded: the capture is abandoned (the error text is the launch's)
        const std::string why = h->err;
        hipGraph_t dead = nullptr;
        h->capturing = false; h->tick_slot = h->capture_start_slot;
        (void)hipStreamEndCapture(h->stream, &dead);
        if (dead) (void)hipGraphDestroy(dead);
        (void)hipGetLastError();
        h->err = why;
        return rc;
    }
    if (h->capture_calls % 2 != 0) {
        // An odd number of launches leaves the tick in the other slot, and the nodes' slot pointers are baked in: one more node
        // (a one-thread kernel, ~1.5 us per replay; an even count needs none) moves it back to where a replay starts reading.
        hipLaunchKernelGGL(move_tick_kernel, dim3(1), dim3(64), 0, h->stream,
                           h->d_tick + (h->capture_start_slot ? 16 : 0), h->d_tick + (h->tick_slot ? 16 : 0));
        h->tick_slot = h->capture_start_slot;
    }
    h->capturing = false;
    hipGraph_t graph = nullptr;
    HIP_TRY(h, hipStreamEndCapture(h->stream, &graph));
    soccer_graph* g = new soccer_graph();
    g->kernel_nodes = h->capture_kernels; g->steps_fused = h->capture_steps_fused; g->fused_launches = h->capture_fused_launches;
    g->graph = graph; g->ticks = h->capture_ticks; g->start_slot = h->capture_start_slot; g->stamped = h->capture_stamped;
    hipError_t e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(graph); delete g;
        return fail(h, SOCCER_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    // move the executable graph to the device now, so that the first soccer_graph_launch does not pay for it
    // (best effort: a runtime without hipGraphUpload support just uploads on first launch)
    (void)hipGraphUpload(g->exec, h->stream);
    (void)hipGetLastError();
    *out = g;
    return SOCCER_OK;
}

extern "C" int soccer_graph_launch(soccer_handle* h, soccer_graph* g, int32_t replays) {
    if (!h || !g) return fail(h, SOCCER_E_INVALID, "handle/graph is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_graph_launch during graph capture");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (replays > 0 && h->tick_slot != g->start_slot) {
        // launches issued since the capture left the tick in the other slot: move it across
        HIP_TRY(h, hipMemcpyAsync(h->d_tick + (g->start_slot ? 16 : 0), h->d_tick + (h->tick_slot ? 16 : 0),
                                  sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
        h->tick_slot = g->start_slot;
    }
    // one replay: remember what the closing stamp holds, so that soccer_timer_read can watch it change (several replays
    // would each write it)
    // (only with the stream idle: a replay still in flight would write the slot AFTER it was sampled, and soccer_timer_read would
    // return on that earlier replay's stamp; otherwise — and for graphs without timer nodes — soccer_timer_read waits for the stream)
    h->stamp_poll = replays == 1 && g->stamped && hipStreamQuery(h->stream) == hipSuccess;
    (void)hipGetLastError();
    h->timer_stamped = g->stamped;          // soccer_timer_read after this launch: the graph's stamps, or the eager events
    if (h->stamp_poll) h->stamp_prev = stamp_host(h)[kStampStride];
    for (int32_t r = 0; r < replays; ++r) HIP_TRY(h, hipGraphLaunch(g->exec, h->stream));
    h->tick += g->ticks * (uint64_t)(replays > 0 ? replays : 0);
    return SOCCER_OK;
}

extern "C" int soccer_graph_info(const soccer_graph* g, int32_t* kernel_nodes, int64_t* steps_fused, int32_t* fused_launches) {
    if (!g) return fail(nullptr, SOCCER_E_INVALID, "graph is NULL");
    if (kernel_nodes) *kernel_nodes = g->kernel_nodes;
    if (steps_fused) *steps_fused = g->steps_fused;
    if (fused_launches) *fused_launches = g->fused_launches;
    return SOCCER_OK;
}

extern "C" int soccer_graph_destroy(soccer_handle* h, soccer_graph* g) {
    if (!g) return SOCCER_OK;
    if (h) { (void)hipSetDevice(h->cfg.device); (void)hipStreamSynchronize(h->stream); }
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// episode returns from [T][n] result trajectories (trajectory_returns_kernel)
extern "C" int soccer_trajectory_returns(soccer_handle* h, int32_t n_steps, const int8_t* reward, const uint8_t* terminated,
                                         const uint8_t* truncated, int64_t stride, int8_t* last_return,
                                         int32_t* episode_count, uint64_t hist[3]) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_trajectory_returns during graph capture");
    if (n_steps < 1 || !reward || !terminated || !truncated)
        return fail(h, SOCCER_E_INVALID, "soccer_trajectory_returns: n_steps >= 1 and the reward / terminated / truncated trajectories are required");
    if (stride < (int64_t)h->P.n) return fail(h, SOCCER_E_INVALID, "soccer_trajectory_returns: stride must be >= n_lanes");
    if (!aligned(episode_count, 4)) return fail(h, SOCCER_E_INVALID, "soccer_trajectory_returns: episode_count must be 4-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t slots = (size_t)h->grid_cap * 2;       // one u64[4] per workgroup of the (at most two) launches
    if (!h->d_traj_hist) if (int rc = h->bufs.alloc(h, slots * 4, &h->d_traj_hist)) return rc;
    const unsigned long long n = h->P.n;
    const bool vec = stride % 4 == 0 && aligned(reward, 4) && aligned(terminated, 4) && aligned(truncated, 4) &&
                     aligned(last_return, 4) && aligned(episode_count, 16);
    const unsigned long long n4 = vec ? (n & ~3ull) : 0ull;
    TrajIO io{reward, terminated, truncated, (long long)stride, n_steps, n4, last_return, episode_count, h->d_traj_hist, 0u};
    uint32_t used = 0;
    if (n4) { used = (uint32_t)grid_for(h, n4 >> 2); hipLaunchKernelGGL(trajectory_returns_kernel<true>, dim3(used), dim3(kBlock), 0, h->stream, io); }
    if (n4 < n) {               // ragged tail, or everything when a stream is not dword-aligned: a lane per thread
        TrajIO t = io;
        t.reward += n4; t.terminated += n4; t.truncated += n4; t.n = n - n4; t.slot0 = used;
        t.last_return = off(last_return, n4); t.episode_count = off(episode_count, n4);
        const uint32_t g2 = (uint32_t)grid_for(h, t.n);
        hipLaunchKernelGGL(trajectory_returns_kernel<false>, dim3(g2), dim3(kBlock), 0, h->stream, t);
        used += g2;
    }
    HIP_TRY(h, hipGetLastError());
    if (hist) {
        std::vector<unsigned long long> part((size_t)used * 4);
        HIP_TRY(h, hipMemcpyAsync(part.data(), h->d_traj_hist, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        hist[0] = hist[1] = hist[2] = 0;
        for (uint32_t b = 0; b < used; ++b) for (int k = 0; k < 3; ++k) hist[k] += part[(size_t)b * 4 + k];
    }
    return SOCCER_OK;
}

