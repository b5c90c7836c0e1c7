// LayerNorm + GELU kernels (gfx950, MI355X) — modern-MLP extensions
// beyond the reference's ReLU/Softmax module set.
//
// LayerNorm: wave-per-row, f32 statistics, bf16 I/O.
//   fwd: y = (x - µ) * rstd * γ + β ; saves µ, rstd per row.
//       Two-pass statistics: µ = Σx / C, then var = Σ(x - µ)² / C;
//       rows of up to 1024 elements are held in registers between passes.
//   bwd (input grad): dx = rstd * (g - mean(g) - x̂ * mean(g * x̂)),
//       g = dy * γ, x̂ = (x - µ) * rstd  — wave-per-row.
//   bwd (param grads): dγ[c] += Σ_rows dy * x̂ ; dβ[c] += Σ_rows dy —
//       column reduction, coalesced row-major walk + f32 atomics.
// GELU (tanh approximation): elementwise, bf16 I/O vectorized.
//   bwd needs the PRE-activation z (stashed by the layer).

#include "common.h"
#include "launchers.h"

// --------------------------------------------------------------- layernorm

// Statistics in two passes, as the CPU path defines them: mu = sum x / C,
// then var = sum (x - mu)^2 / C, non-negative by construction.  (A
// one-pass E[x^2] - mu^2 cancels to an absolute error of C ulps of mu^2:
// on a constant or large-mean row that is as large as var + eps, or
// negative, and rsqrt returns NaN.)
// R > 0: the row fits R elements per lane (C <= 64 R) and is read ONCE
// into registers for all three passes; R = 0: any C, each pass re-reads
// the row (in cache).  Lane-strided in both, so a lane adds the same
// values in the same order either way.
template <int R>
__global__ __launch_bounds__(256) void ln_fwd_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ gamma,
    const __bf16* __restrict__ beta, __bf16* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd, int B, int C,
    float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const __bf16* xr = x + (long)row * C;
    __bf16* yr = y + (long)row * C;
    float v[R > 0 ? R : 1];
    float s = 0.f, s2 = 0.f;
    if constexpr (R > 0) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + 64 * k;
            v[k] = c < C ? bf2f(xr[c]) : 0.f;
            s += v[k];
        }
    } else {
        for (int c = lane; c < C; c += 64) s += bf2f(xr[c]);
    }
    const float mu = wave_sum(s) / C;
    if constexpr (R > 0) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float d = lane + 64 * k < C ? v[k] - mu : 0.f;
            s2 += d * d;
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            const float d = bf2f(xr[c]) - mu;
            s2 += d * d;
        }
    }
    const float var = wave_sum(s2) / C;
    const float rs = rsqrtf(var + eps);
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
    if constexpr (R > 0) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int c = lane + 64 * k;
            if (c < C)
                yr[c] = f2bf((v[k] - mu) * rs * bf2f(gamma[c]) +
                             bf2f(beta[c]));
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            const float xh = (bf2f(xr[c]) - mu) * rs;
            yr[c] = f2bf(xh * bf2f(gamma[c]) + bf2f(beta[c]));
        }
    }
}

__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
    const __bf16* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, __bf16* __restrict__ dx, int B, int C) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const __bf16* dyr = dy + (long)row * C;
    const __bf16* xr = x + (long)row * C;
    const float mu = mean[row], rs = rstd[row];
    float sg = 0.f, sgx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float g = bf2f(dyr[c]) * bf2f(gamma[c]);
        const float xh = (bf2f(xr[c]) - mu) * rs;
        sg += g;
        sgx += g * xh;
    }
    sg = wave_sum(sg) / C;
    sgx = wave_sum(sgx) / C;
    __bf16* dxr = dx + (long)row * C;
    for (int c = lane; c < C; c += 64) {
        const float g = bf2f(dyr[c]) * bf2f(gamma[c]);
        const float xh = (bf2f(xr[c]) - mu) * rs;
        dxr[c] = f2bf(rs * (g - sg - xh * sgx));
    }
}

__global__ __launch_bounds__(256) void ln_bwd_dparam_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int C,
    int rows_per_block) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(B, r0 + rows_per_block);
    if (col >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float d = bf2f(dy[(long)r * C + col]);
        const float xh = (bf2f(x[(long)r * C + col]) - mean[r]) * rstd[r];
        sg += d * xh;
        sb += d;
    }
    atomicAdd(&dgamma[col], sg);
    atomicAdd(&dbeta[col], sb);
}

// ------------------------------------------------------------------ gelu

__device__ __forceinline__ float gelu_f(float z) {
    // tanh approximation
    const float c = 0.7978845608028654f;  // sqrt(2/pi)
    const float u = c * (z + 0.044715f * z * z * z);
    return 0.5f * z * (1.f + tanhf(u));
}

__device__ __forceinline__ float gelu_grad_f(float z) {
    const float c = 0.7978845608028654f;
    const float u = c * (z + 0.044715f * z * z * z);
    const float t = tanhf(u);
    const float du = c * (1.f + 3.f * 0.044715f * z * z);
    return 0.5f * (1.f + t) + 0.5f * z * (1.f - t * t) * du;
}

__global__ __launch_bounds__(256) void gelu_fwd_kernel(
    const __bf16* __restrict__ z, __bf16* __restrict__ y, long n) {
    long i = (long)(blockIdx.x * 256 + threadIdx.x) * 8;
    const long stride = (long)gridDim.x * 256 * 8;
    for (; i + 8 <= n; i += stride) {
        bf16x8 v = *(const bf16x8*)(z + i);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(gelu_f(bf2f(v[j])));
        *(bf16x8*)(y + i) = o;
    }
    if (i < n)
        for (; i < n; ++i) y[i] = f2bf(gelu_f(bf2f(z[i])));
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ z,
    __bf16* __restrict__ dz, long n) {
    long i = (long)(blockIdx.x * 256 + threadIdx.x) * 8;
    const long stride = (long)gridDim.x * 256 * 8;
    for (; i + 8 <= n; i += stride) {
        bf16x8 g = *(const bf16x8*)(dy + i);
        bf16x8 v = *(const bf16x8*)(z + i);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = f2bf(bf2f(g[j]) * gelu_grad_f(bf2f(v[j])));
        *(bf16x8*)(dz + i) = o;
    }
    if (i < n)
        for (; i < n; ++i) dz[i] = f2bf(bf2f(dy[i]) * gelu_grad_f(bf2f(z[i])));
}

// ---------------------------------------------------------------- launchers

void ss_ln_fwd(const void* x, const void* gamma, const void* beta, void* y,
               void* mean, void* rstd, int B, int C, float eps,
               hipStream_t st) {
    // rows of up to 256 / 1024 elements stay in 4 / 16 registers a lane
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(cdiv(B, 4)), dim3(256), 0, st,
                           (const __bf16*)x, (const __bf16*)gamma,
                           (const __bf16*)beta, (__bf16*)y, (float*)mean,
                           (float*)rstd, B, C, eps);
    };
    if (C <= 256) launch(ln_fwd_kernel<4>);
    else if (C <= 1024) launch(ln_fwd_kernel<16>);
    else launch(ln_fwd_kernel<0>);
}

void ss_ln_bwd_dx(const void* dy, const void* x, const void* gamma,
                  const void* mean, const void* rstd, void* dx, int B, int C,
                  hipStream_t st) {
    hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st,
                       (const __bf16*)dy, (const __bf16*)x,
                       (const __bf16*)gamma, (const float*)mean,
                       (const float*)rstd, (__bf16*)dx, B, C);
}

void ss_ln_bwd_dparam(const void* dy, const void* x, const void* mean,
                      const void* rstd, void* dgamma, void* dbeta, int B,
                      int C, hipStream_t st) {
    int col_tiles = cdiv(C, 256);
    int splits = cdiv(512, col_tiles);
    if (splits > cdiv(B, 64)) splits = cdiv(B, 64);
    if (splits < 1) splits = 1;
    dim3 grid(col_tiles, splits);
    hipLaunchKernelGGL(ln_bwd_dparam_kernel, grid, dim3(256), 0, st,
                       (const __bf16*)dy, (const __bf16*)x,
                       (const float*)mean, (const float*)rstd, (float*)dgamma,
                       (float*)dbeta, B, C, cdiv(B, splits));
}

void ss_gelu_fwd(const void* z, void* y, long n, hipStream_t st) {
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st,
                       (const __bf16*)z, (__bf16*)y, n);
}

void ss_gelu_bwd(const void* dy, const void* z, void* dz, long n,
                 hipStream_t st) {
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st,
                       (const __bf16*)dy, (const __bf16*)z, (__bf16*)dz, n);
}
