// floor_lab.hip — what bounds a single-step launch at 2^20 lanes?  Same grid (1024 x 256 threads, 4 lanes per thread), same
// streams and non-temporal dword accesses as step_kernel_swar, graph-replayed like bench.py:
//   empty      nothing                                    -> launch + dependent-kernel boundary
//   copy       8 loads, 10 stores, one xor per dword      -> + the 19 B/lane round trip
//   copy+rng   + the Philox block of the thread's 4 lanes -> + the vector work that no rule needs
//   copy13     5 loads, 7 stores (three state streams)    -> the round trip once the state is packed into 13 B/lane
// and what kernel-argument fetches on a wave's critical path cost (k_copy13a: the 13 B copy with step_kernel_swar's argument
// shape — seven leading scalars, preloaded into SGPRs, then a struct that makes the block 424 bytes with the hidden arguments):
//   copy13a        every other argument requested in one batch at wave start           -> the plain row
//   + first        a word of the non-preloaded part (offset 0xb8) added into the loads' address: one scalar-memory round
//                  trip between wave start and the first data load
//   + 2 serial     two argument loads, each waited for, between the last arithmetic and the stores (offsets 0xc0, 0x130)
//   + both
// Build (the library's preload flag, or the leading scalars are fetched like everything else and no row is plain):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-kernarg-preload-count=14 -Igym_soccer_littman94_amd/csrc \
//         -o build/floor_lab tools/labs/floor_lab.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "soccer_kernels.hpp"
using namespace soccer;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1);} } while (0)

struct Args { uint8_t* state; unsigned long long stride; const int8_t* aa; const int8_t* ab; uint16_t* obs; int8_t* rew; uint8_t* te; uint8_t* tr; unsigned long long tick; };

__global__ __launch_bounds__(256) void k_empty(const Args A) {}

template <bool RNG, int NS = 6>
__global__ __launch_bounds__(256) void k_copy(const Args A) {
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) << 2;
    const uint8_t* sp = A.state + i0;
    uint32_t s[6];
#pragma unroll
    for (int k = NS; k < 6; ++k) s[k] = 0x01010101u * (uint32_t)k;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(sp + k * A.stride));
    const uint32_t a = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(A.aa + i0));
    const uint32_t b = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(A.ab + i0));
    uint32_t x = a ^ b;
    if (RNG) { const Philox4 p = philox4x32_10((uint32_t)(i0 >> 2), 0u, (uint32_t)A.tick, 0u, 1u, 2u); x ^= p.w[0] ^ p.w[1] ^ p.w[2] ^ p.w[3]; }
    x &= 0x01010101u;
    uint8_t* sw = A.state + i0;
#pragma unroll
    for (int k = 0; k < NS; ++k) __builtin_nontemporal_store(s[k] ^ (k == NS - 1 ? x : 0u), reinterpret_cast<uint32_t*>(sw + k * A.stride));
    __builtin_nontemporal_store((unsigned long long)s[0] | ((unsigned long long)s[1] << 32), reinterpret_cast<unsigned long long*>(A.obs + i0));
    __builtin_nontemporal_store(s[2] ^ x, reinterpret_cast<uint32_t*>(A.rew + i0));
    __builtin_nontemporal_store(s[3], reinterpret_cast<uint32_t*>(A.te + i0));
    __builtin_nontemporal_store(s[4], reinterpret_cast<uint32_t*>(A.tr + i0));
}

// The part of the argument block behind the 56 bytes of leading scalars, fields at the offsets step_kernel_swar's had when the
// waits were found (before its SwarParams was reordered): `first` at 0xb8, tick_out / misuse at 0xc0, the result pointers at 0x130.
struct Big {
    uint32_t pad0[32];
    unsigned long long first;
    unsigned long long* tick_out; unsigned int* misuse;
    uint32_t pad1[24];
    uint16_t* obs; int8_t* rew; uint8_t* te; uint8_t* tr;
    uint32_t pad2[16];
};
static_assert(sizeof(Big) == 400 - 56 && offsetof(Big, first) == 0xb8 - 56 && offsetof(Big, tick_out) == 0xc0 - 56 && offsetof(Big, obs) == 0x130 - 56,
              "400 bytes of explicit arguments (424 with the hidden ones behind them), the fields where the product kernel had them");

// MODE bit 0: `first` (always 0) enters the loads' address; bit 1: the stores' pointers are fetched by two serial scalar loads
// behind the arithmetic (written out, with their waits: the compiler would batch them at the top of this one-block kernel).
template <int MODE>
__global__ __launch_bounds__(256) void k_copy13a(uint8_t* state, unsigned long long stride, const int8_t* aa, const int8_t* ab,
                                                 const unsigned long long* tick_in, unsigned long long n, unsigned long long tick_val,
                                                 const Big B) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (((unsigned long long)g << 2) >= n) return;
    uint32_t i0 = g << 2;
    if (MODE & 1) i0 += (uint32_t)B.first;
    uint32_t s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(state + k * stride + i0));
    const uint32_t a = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(aa + i0));
    const uint32_t b = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ab + i0));
    uint32_t x = (a ^ b) & 0x01010101u;
    // (global pointers: one rebuilt from the loaded words would otherwise be a generic one, and its store a flat store)
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    gbyte* obs = (gbyte*)B.obs; gbyte* rew = (gbyte*)B.rew; gbyte* te = (gbyte*)B.te; gbyte* tr = (gbyte*)B.tr;
    if (MODE & 2) {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u8 __attribute__((ext_vector_type(8)));
        u4 lo; u8 hi;
        // (tied to x and to the state words: behind the wait for the state and the arithmetic, ahead of the stores)
        asm volatile("s_load_dwordx4 %[lo], %[ka], 0xc0\n\ts_waitcnt lgkmcnt(0)\n\ts_load_dwordx8 %[hi], %[ka], 0x130\n\ts_waitcnt lgkmcnt(0)"
                     : [lo] "=&s"(lo), [hi] "=&s"(hi), "+v"(x), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]) : [ka] "s"(__builtin_amdgcn_kernarg_segment_ptr()));
        auto ptr = [](uint32_t l, uint32_t h) { return (unsigned long long)l | ((unsigned long long)h << 32); };
        obs = (gbyte*)ptr(hi[0], hi[1]); rew = (gbyte*)ptr(hi[2], hi[3]); te = (gbyte*)ptr(hi[4], hi[5]); tr = (gbyte*)ptr(hi[6], hi[7]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(s[k] ^ (k == 2 ? x : 0u), reinterpret_cast<uint32_t*>(state + k * stride + i0));
    __builtin_nontemporal_store((unsigned long long)s[0] | ((unsigned long long)s[1] << 32), (__attribute__((address_space(1))) unsigned long long*)(obs + 2 * i0));
    __builtin_nontemporal_store(s[2] ^ x, (__attribute__((address_space(1))) uint32_t*)(rew + i0));
    __builtin_nontemporal_store(0x03030303u, (__attribute__((address_space(1))) uint32_t*)(te + i0));
    __builtin_nontemporal_store(0x04040404u, (__attribute__((address_space(1))) uint32_t*)(tr + i0));
}

int main() {
    const size_t N = 1 << 20; const int K = 200, ROUNDS = 7, T = 64;
    uint8_t* st_; int8_t* act; uint16_t* obs; int8_t* rew; uint8_t* te; uint8_t* tr;
    CK(hipMalloc(&st_, 6 * N)); CK(hipMemset(st_, 1, 6 * N));
    CK(hipMalloc(&act, (size_t)T * 2 * N)); CK(hipMemset(act, 2, (size_t)T * 2 * N));
    CK(hipMalloc(&obs, (size_t)T * N * 2)); CK(hipMalloc(&rew, (size_t)T * N)); CK(hipMalloc(&te, (size_t)T * N)); CK(hipMalloc(&tr, (size_t)T * N));
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto args = [&](int k) { const size_t r = (size_t)(k % T); return Args{st_, N, act + r * 2 * N, act + r * 2 * N + N, obs + r * N, rew + r * N, te + r * N, tr + r * N, (unsigned long long)k}; };
    const char* names[8] = {"empty", "copy (19 B/lane, nt dwords)", "copy + Philox block", "copy (13 B/lane, 3 state streams)",
                            "copy13a (424 B block, preloaded)", "copy13a + first in the address", "copy13a + 2 serial loads at stores", "copy13a + both"};
    for (int v = 0; v < 8; ++v) {
        hipGraph_t g; hipGraphExec_t ge;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < K; ++k) {
            const Args a = args(k);
            if (v == 0) hipLaunchKernelGGL(k_empty, dim3(1024), dim3(256), 0, s, a);
            else if (v == 1) hipLaunchKernelGGL(k_copy<false>, dim3(1024), dim3(256), 0, s, a);
            else if (v == 2) hipLaunchKernelGGL(k_copy<true>, dim3(1024), dim3(256), 0, s, a);
            else if (v == 3) hipLaunchKernelGGL((k_copy<false, 3>), dim3(1024), dim3(256), 0, s, a);
            else {
                Big B{}; B.first = 0ull; B.obs = a.obs; B.rew = a.rew; B.te = a.te; B.tr = a.tr;
#define COPY13A(M) hipLaunchKernelGGL(k_copy13a<M>, dim3(1024), dim3(256), 0, s, a.state, a.stride, a.aa, a.ab, (const unsigned long long*)nullptr, (unsigned long long)N, a.tick, B)
                if (v == 4) COPY13A(0); else if (v == 5) COPY13A(1); else if (v == 6) COPY13A(2); else COPY13A(3);
#undef COPY13A
            }
        }
        CK(hipStreamEndCapture(s, &g)); CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        CK(hipGraphLaunch(ge, s)); CK(hipStreamSynchronize(s));
        std::vector<float> ms;
        for (int r = 0; r < ROUNDS; ++r) {
            CK(hipEventRecord(e0, s)); CK(hipGraphLaunch(ge, s)); CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1)); ms.push_back(t * 1e3f / K);
        }
        std::sort(ms.begin(), ms.end());
        printf("%-34s median %.2f  min %.2f us per launch (graph of %d, N = 2^20)\n", names[v], ms[ms.size() / 2], ms[0], K);
        CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    }
    return 0;
}
