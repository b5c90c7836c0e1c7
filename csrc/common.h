// Shared helpers for the shallowspeed_amd HIP/CDNA4 (gfx950) kernels.
//
// Targets MI355X only: wave64, 4 SIMD-32/CU, MFMA bf16 matrix cores,
// 160 KiB LDS/CU.  No CUDA-compat paths, no other archs.
//
// Device side: vector and address-space types, counted waits, the XCD
// block remap, wave reductions.  Host side: the grid-size, environment
// and bool-dispatch helpers the launchers share.  A new kernel file
// takes these from here; launcher prototypes live in launchers.h.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdlib>
#include <type_traits>

#define WAVE 64

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// operand types of global_load_lds (HBM -> LDS DMA) and of the LDS
// transpose read
typedef __attribute__((address_space(1))) const unsigned int* gptr_t;
typedef __attribute__((address_space(3))) unsigned int* lptr_t;
typedef __attribute__((address_space(3))) bf16x4v* lds_v4p;

// counted waits and the bare barrier of the hand-scheduled kernels
#define SS_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n))
#define SS_LGKM(n) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n))
#define SS_BAR() __builtin_amdgcn_s_barrier()

__device__ __forceinline__ float bf2f(__bf16 v) { return (float)v; }
__device__ __forceinline__ __bf16 f2bf(float v) { return (__bf16)v; }

// XCD-aware bijective block remap (8 XCDs, each with its own L2): the
// dispatcher places hardware block hw on XCD hw % 8; the returned work
// id gives each XCD one CONTIGUOUS run of the nwg work ids, so blocks
// that a kernel decodes as neighbours share one L2.  The decode of the
// work id into tile origins is the kernel's own.
__device__ __forceinline__ int xcd_remap(int hw, int nwg) {
    const int xcd = hw % 8, q8 = nwg / 8, r8 = nwg % 8;
    return (xcd < r8 ? xcd * (q8 + 1)
                     : r8 * (q8 + 1) + (xcd - r8) * q8) + hw / 8;
}

// 64-lane xor-butterfly reductions: every lane ends with the result
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------- host

// ceil-div
constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// grid of the 8-wide grid-stride elementwise kernels (256 threads)
inline int ew_grid(long n) {
    long blocks = (n / 8 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;  // grid-stride the rest (G11)
    return (int)blocks;
}

// Integer environment variable, atoi-parsed.  Launchers read each SS_*
// variable ONCE: `static const int v = env_int("SS_X", dflt);`.
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, ...): the
// run-time flags become template arguments inside a generic lambda, one
// instantiation per combination.
template <class F>
inline void with_bools(F&& f) {
    f();
}
template <class F, class... Rest>
inline void with_bools(F&& f, bool b, Rest... rest) {
    if (b)
        with_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else
        with_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
