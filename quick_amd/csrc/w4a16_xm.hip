// Mid-token kernels (w4a16_xm.hpp): instantiations and launcher.  Its own translation unit.
#include "w4a16_common.hpp"

#include "w4a16_args.hpp"
#include "w4a16_xm.hpp"
#include "w4a16_xm_host.hpp"

namespace quick_amd {

unsigned xm_lds_need(int mb, int pr) { return xm_lds_bytes(mb, pr); }

template <int MB, int PR, int ABL>
static bool xm_go(const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  XmRest rest{a.bias, a.residual, a.Y, a.span, a.dbg, a.silu_mul};
  const int tpg_log2 = 31 - __builtin_clz((unsigned)a.tpg);
  launch_kernel<w4a16_xm_kernel<MB, PR, ABL>>(L, dim3(grid_x, grid_y), dim3(512), xm_lds_bytes(MB, PR), 160 * 1024, a.X, a.QW, a.S, a.M, a.K, a.N, tpg_log2, grid_x, rest);
  return true;
}

template <int ABL>
static bool xm_go_t(int mb, int pr, const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  switch (mb * 10 + pr) {
    case 11: return xm_go<1, 1, ABL>(a, grid_x, grid_y, L);
    case 12: return xm_go<1, 2, ABL>(a, grid_x, grid_y, L);
    case 13: return xm_go<1, 3, ABL>(a, grid_x, grid_y, L);
    case 21: return xm_go<2, 1, ABL>(a, grid_x, grid_y, L);
    case 22: return xm_go<2, 2, ABL>(a, grid_x, grid_y, L);
    case 23: return xm_go<2, 3, ABL>(a, grid_x, grid_y, L);
    default: return false;
  }
}

bool xm_launch(int mb, int pr, int abl, const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  if (a.G % 128 != 0 || (a.tpg & (a.tpg - 1)) != 0 || a.ln_w != nullptr) return false;
  switch (abl) {
    case 0: return xm_go_t<0>(mb, pr, a, grid_x, grid_y, L);
    case 32: return xm_go_t<32>(mb, pr, a, grid_x, grid_y, L);
#ifdef QUICK_AMD_TOOLS
    case 64: return xm_go_t<64>(mb, pr, a, grid_x, grid_y, L);
#endif
    default: return false;
  }
}

}  // namespace quick_amd
