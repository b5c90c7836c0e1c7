// The stage arm of the backward chain (gfx950 / MI355X): the ReLU-layer
// data gradients of a pipeline stage that has no classifier head, as
// ONE kernel entered from the received gradient dout [M][256] in memory
// in place of the head.  The kernel's text, its bits and its launch
// contract (minus C; dout 16-B aligned) are bwd_chain.hip's: see there
// and bwd_chain_kernel.h.

#include "chain_dev.h"

// This arm's scaled products stay one v_mul_f32 each: the factor goes
// through an empty asm statement, which keeps the compiler from pairing
// two of them into a packed f32 multiply (new kernels here are built
// without packed f32 arithmetic; the headed kernel keeps the
// instructions it has).
__device__ __forceinline__ float chain_unpaired(float f) {
    asm volatile("" : "+v"(f));
    return f;
}
#define BWD_CHAIN_KERNEL bwd_chain_stage_kernel
#define BWD_CHAIN_HEAD 0
#define BWD_CHAIN_SCALE(f) (chain_unpaired(f) * (dz_scale + ...))
#include "bwd_chain_kernel.h"

// The stage arm.  Same arguments and overrides.  The shipped rows follow
// the forward chain's rule, 32 where 64-row tiles would cover at most
// half of the 256 CUs: measured at M = 4096 (12.1 against 13.8 us, three
// layers) and M = 16384 (64 rows: 18.6 against 23.0 us;
// scripts/microbench_stage_chain.py, docs/KERNELS.md).  The scaled form
// is built for the eight-wave arms without w_lds, the ones that ship.
bool ss_bwd_chain_stage(const void* dout, const void* const* h,
                        const void* const* wt, void* const* dz, int nlayers,
                        void* dx, int M, int H, int rows, int waves,
                        int w_lds, float dz_scale, hipStream_t st) {
    if (M < 1 || H != 256 || nlayers < 1 || nlayers > SS_BWD_CHAIN_MAX ||
        !aligned16(dout))
        return false;
    BwdChainLayers L = {};
    if (!bwd_chain_layers(L, h, wt, dz, nlayers, dx)) return false;
    bwd_chain_env(rows, waves, w_lds);
    if (!rows) rows = cdiv(M, 64) <= 128 ? 32 : 64;
    if (!waves) waves = 8;
    if (dz_scale != 1.f) {
        if (waves != 8 || w_lds != 0) return false;
        if (rows == 32)
            bwd_chain_launch<32, 8>(dout, L, nlayers, dx, M, st,
                                          dz_scale);
        else if (rows == 64)
            bwd_chain_launch<64, 8>(dout, L, nlayers, dx, M, st,
                                          dz_scale);
        else
            return false;
        return true;
    }
    if (w_lds == 1) {
        if (rows != 64 || waves != 8) return false;
        bwd_chain_launch<64, 8, true>(dout, L, nlayers, dx, M, st);
        return true;
    }
    return with_chain_arm(rows, waves, [&](auto r, auto nw) {
        bwd_chain_launch<r.value, nw.value>(dout, L, nlayers, dx, M, st);
    });
}
