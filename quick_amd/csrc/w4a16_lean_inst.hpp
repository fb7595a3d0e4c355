// Lean small-M kernels: the per-build launcher template (group mode, RMSNorm prologue and token-count flavours of one (waves, tiles per wave,
// channel tiles) build).  Explicitly instantiated in w4a16_lean_a/b/c.hip so that the builds compile in parallel; w4a16_lean.hip dispatches.
#pragma once
#include <algorithm>

#include "w4a16_args.hpp"
#include "w4a16_lean.hpp"
#include "w4a16_lean_host.hpp"

namespace quick_amd {

template <int WAVES, int TMAX, int NTW, int GM, int ABL, bool LN, int MR, int NSETS = 1>
static bool lean_go(const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  const unsigned lds = lean_lds_need(a.M, a.K, WAVES, NTW, a.ln_w != nullptr, NSETS > 1);
  LeanRest rest{};
  rest.Y = a.Y; rest.bias = a.bias; rest.residual = a.residual; rest.silu_mul = a.silu_mul; rest.ln_eps = a.ln_eps; rest.span = a.span; rest.dbg = a.dbg;
  launch_kernel<w4a16_lean_kernel<WAVES, TMAX, NTW, GM, ABL, LN, MR, NSETS>>(L, dim3(grid_x, grid_y), dim3(WAVES * 64), lds, 160 * 1024, a.X, a.QW, a.S, a.ln_w, a.K, a.N, a.M,
                                                                            (unsigned)(a.K / a.G), grid_x, (unsigned)a.tpg, rest);
  return true;
}

// token-count flavour: 1 token / up to 4 tokens with the unit sums as scalars (while TMAX * 4 * 2 of them fit the SGPRs), else the matrix-core sums
template <int WAVES, int TMAX, int NTW, int GM, int ABL, bool LN>
static bool lean_go_m(const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  // fewer workgroups than channel blocks: persistent (two register sets, the next block's requests in flight under this block's tiles);
  // builds with up to four tiles per wave, G = 128, no phase stamps
  if (grid_x < (a.N >> 4) / NTW) {
    // eight waves (sixteen would need more registers than a 1024-thread workgroup may have), up to four tiles per wave, G = 128, no stamps;
    // two register sets (four were measured slower, 16 x 4096 x 22016 14.4 -> 14.8 us: with one workgroup per CU the block time is the waves'
    // own dependency chains, not the depth of the requests in flight)
    if constexpr (WAVES == 8 && TMAX <= 4 && GM == 0 && ABL != 64) {
      constexpr int NS = 2;
      if (a.M == 1) return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 1, NS>(a, grid_x, grid_y, L);
      if (a.M <= 4) return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 4, NS>(a, grid_x, grid_y, L);
      return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 16, NS>(a, grid_x, grid_y, L);
    }
    return false;
  }
  if (a.M == 1) return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 1>(a, grid_x, grid_y, L);
  if constexpr (TMAX <= 8) {
    if (a.M <= 4) return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 4>(a, grid_x, grid_y, L);
  }
  return lean_go<WAVES, TMAX, NTW, GM, ABL, LN, 16>(a, grid_x, grid_y, L);
}

template <int WAVES, int TMAX, int NTW, int ABL>
bool lean_build(const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  if constexpr (ABL == 0) {
    if (a.ln_w != nullptr) {
      if (a.G == 128) return lean_go_m<WAVES, TMAX, NTW, 0, ABL, true>(a, grid_x, grid_y, L);
      return lean_go_m<WAVES, TMAX, NTW, 1, ABL, true>(a, grid_x, grid_y, L);
    }
    if (a.G == 128) return lean_go_m<WAVES, TMAX, NTW, 0, ABL, false>(a, grid_x, grid_y, L);
    return lean_go_m<WAVES, TMAX, NTW, 1, ABL, false>(a, grid_x, grid_y, L);
  } else {  // span / phase stamps: G = 128, the stamps of the RMSNorm prologue on the 8 x 4 builds only
    if (a.G != 128) return false;
    if (a.ln_w != nullptr) {
      if constexpr (ABL == 64 && WAVES == 8 && TMAX == 4) return lean_go_m<WAVES, TMAX, NTW, 0, ABL, true>(a, grid_x, grid_y, L);
      return false;
    }
    return lean_go_m<WAVES, TMAX, NTW, 0, ABL, false>(a, grid_x, grid_y, L);
  }
}

#ifdef QUICK_AMD_TOOLS
#define QA_LEAN_INSTANTIATE(W, T, C)                                                                                    \
  template bool lean_build<W, T, C, 0>(const GemmArgs&, int, int, const Launch&);                                       \
  template bool lean_build<W, T, C, 32>(const GemmArgs&, int, int, const Launch&);                                      \
  template bool lean_build<W, T, C, 64>(const GemmArgs&, int, int, const Launch&);
#else
#define QA_LEAN_INSTANTIATE(W, T, C)                                                                                    \
  template bool lean_build<W, T, C, 0>(const GemmArgs&, int, int, const Launch&);                                       \
  template bool lean_build<W, T, C, 32>(const GemmArgs&, int, int, const Launch&);
#endif

}  // namespace quick_amd
