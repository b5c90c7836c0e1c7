// What the wide chain kernels share (fwd_chain_wide.hip,
// bwd_chain_wide.hip; H = 128 and 512): the register budget their K loops
// are sized by, the (rows, waves) arms built per width and the shipped
// choice among them.  The device pieces are chain_dev.h's macros as they
// stand; each kernel defines the geometry names they read.
#pragma once

#include "chain_dev.h"
#include "launchers.h"

// Registers per lane that a block of NW waves leaves each of its waves
// when it has a CU to itself: the 512 of a SIMD over its NW / 4 waves.
constexpr int wide_reg_budget(int NW) { return NW <= 8 ? 256 : 2048 / NW; }

// The (rows, waves) arms built for width H, the serving kernel's pairs.
// Calls f(integral_constant<H>, <rows>, <waves>) and returns true; false,
// with f not called, for any other pair.
template <int H, class F>
inline bool with_chain_wide_arm(int rows, int waves, F&& f) {
    using std::integral_constant;
    auto arm = [&](auto r, auto nw) {
        if (rows != r.value || waves != nw.value) return false;
        f(integral_constant<int, H>{}, r, nw);
        return true;
    };
    using I32 = integral_constant<int, 32>;
    using I64 = integral_constant<int, 64>;
    static_assert(H == 128 || H == 512, "widths of the wide chain kernels");
    if constexpr (H == 128)
        return arm(I32{}, integral_constant<int, 4>{}) ||
               arm(I64{}, integral_constant<int, 4>{});
    else
        return arm(I32{}, integral_constant<int, 8>{}) ||
               arm(I64{}, integral_constant<int, 8>{}) ||
               arm(I64{}, integral_constant<int, 16>{});
}

// rows / waves == 0 -> the shipped arm of (H, M); a pair with one zero is
// left as it is and matches no arm.  Measured at M = 1024 and 16384, both
// kernels (profiles/r20_chain_wide.md): (32, 4) at 128 for every M; at
// 512 (32, 8) where 64-row tiles would cover at most half of the 256 CUs
// (M <= 8192), above that (64, 16).
inline void chain_wide_shipped(int H, int M, int& rows, int& waves) {
    if (rows || waves) return;
    const bool few = cdiv(M, 64) <= 128;
    rows = H == 128 || few ? 32 : 64;
    waves = H == 128 ? 4 : few ? 8 : 16;
}
