// W4A16 GEMM for MI355X (gfx950), the wide family: launchers of the four-wave wide and LDS-ring kernels.  The kernels themselves are in
// w4a16_wide.hpp, which the exchange-K and four-wave units (w4a16_xk.hip, w4a16_xw.hip) share.
#include "w4a16_common.hpp"

#include "w4a16_args.hpp"
#include "w4a16_launch.hpp"
#include "w4a16_plan.hpp"
#include "w4a16_wide.hpp"

namespace quick_amd {

template <int MB, int PAIRS, int GM, int NBUF, int ABL, int WK>
static bool ring_go(const Plan& p, const GemmArgs& a, const Launch& L) {
  constexpr unsigned lds = NBUF * (MB * 8192 + PAIRS * 8192 + WK * PAIRS * 1024);
  launch_kernel<w4a16_ring_kernel<MB, PAIRS, GM, NBUF, ABL, WK>>(L, dim3(p.ntiles, p.ksplit), dim3(256 * WK), lds, (int)lds, a);
  return true;
}

template <int MB, int PAIRS, int NBUF, int WK = 1>
static bool launch_ring(const Plan& p, const GemmArgs& a, const Launch& L) {
#ifdef QUICK_AMD_TOOLS
  if constexpr ((MB == 2 && PAIRS == 1 && NBUF == 4 && WK == 2) || (MB == 4 && PAIRS == 1 && NBUF == 3 && WK == 2))
    if (p.ablate == 16 && a.G == 128)  // phase stamps into the workspace (tools/wide_phases.py), nothing else changes
      return ring_go<MB, PAIRS, 0, NBUF, 64, WK>(p, a, L);
  if constexpr (MB == 2 && PAIRS == 1 && NBUF == 6 && WK == 1)
    if (p.ablate && a.G == 128) {  // timing experiments (results are wrong on purpose)
      switch (p.ablate) {
        case 1: return ring_go<MB, PAIRS, 0, NBUF, 1, WK>(p, a, L);
        case 5: return ring_go<MB, PAIRS, 0, NBUF, 5, WK>(p, a, L);
        case 9: return ring_go<MB, PAIRS, 0, NBUF, 9, WK>(p, a, L);
        case 18: return ring_go<MB, PAIRS, 0, NBUF, 18, WK>(p, a, L);
        default: return ring_go<MB, PAIRS, 0, NBUF, 2, WK>(p, a, L);
      }
    }
  if constexpr (MB == 2 && PAIRS == 1 && WK == 2)
    if (p.ablate && a.G == 128) {
      if (p.ablate == 1) return ring_go<MB, PAIRS, 0, NBUF, 1, WK>(p, a, L);
      return ring_go<MB, PAIRS, 0, NBUF, 2, WK>(p, a, L);
    }
#endif
  if (a.span) {
    if constexpr (MB == 2 && PAIRS == 1 && ((NBUF == 6 && WK == 1) || (NBUF == 4 && WK == 2))) {
      if (group_mode(a.G) == 0) return ring_go<MB, PAIRS, 0, NBUF, 32, WK>(p, a, L);   // ABL bit 32 = span stamps, nothing else
    }
    return false;
  }
  if (group_mode(a.G) == 0) return ring_go<MB, PAIRS, 0, NBUF, 0, WK>(p, a, L);
  return ring_go<MB, PAIRS, 1, NBUF, 0, WK>(p, a, L);
}

template <int MB, int PAIRS, int GM, int ABL = 0>
static bool wide_go(const Plan& p, const GemmArgs& a, const Launch& L) {
  constexpr unsigned lds = 2 * MB * 32 * 256;
  launch_kernel<w4a16_wide_kernel<MB, PAIRS, GM, ABL>>(L, dim3(p.ntiles, p.ksplit), dim3(256), lds, (int)lds, a);
  return true;
}

template <int MB, int PAIRS>
static bool launch_wide(const Plan& p, const GemmArgs& a, const Launch& L) {
  if constexpr (MB <= 4 && MB * PAIRS <= 4) {
    if (p.wide_nbuf >= 3 && p.waves == 8) {  // eight waves (two per SIMD), the k16 steps split by parity
      constexpr int NMAX8 = wide_ring_nbuf(MB, PAIRS, 2);
      if (p.wide_nbuf == 3) return launch_ring<MB, PAIRS, 3, 2>(p, a, L);
      if (NMAX8 >= 4 && p.wide_nbuf == 4) return launch_ring<MB, PAIRS, (NMAX8 >= 4 ? 4 : 3), 2>(p, a, L);
      return launch_ring<MB, PAIRS, NMAX8, 2>(p, a, L);
    }
  }
  if constexpr (MB <= 4) {
    if (p.wide_nbuf >= 3) {
      constexpr int NMAX = wide_ring_nbuf(MB, PAIRS);
      if (p.wide_nbuf == 3) return launch_ring<MB, PAIRS, 3>(p, a, L);
      if (NMAX >= 4 && p.wide_nbuf == 4) return launch_ring<MB, PAIRS, (NMAX >= 4 ? 4 : 3)>(p, a, L);
      return launch_ring<MB, PAIRS, NMAX>(p, a, L);
    }
  }
  if (a.span) return false;  // no wide kernel without the ring carries span stamps
#ifdef QUICK_AMD_TOOLS
  if constexpr ((MB == 2 && PAIRS == 1) || (MB == 8 && PAIRS == 2) || (MB == 4 && PAIRS == 2))
    if (p.ablate && a.G == 128) {  // timing experiments (results are wrong on purpose)
      if (p.ablate == 1) return wide_go<MB, PAIRS, 0, 1>(p, a, L);
      if (p.ablate == 16) return wide_go<MB, PAIRS, 0, 64>(p, a, L);  // phase stamps into the workspace, nothing else changes
      return wide_go<MB, PAIRS, 0, 2>(p, a, L);
    }
#endif
  if (group_mode(a.G) == 0) return wide_go<MB, PAIRS, 0>(p, a, L);
  return wide_go<MB, PAIRS, 1>(p, a, L);
}

bool wide_launch(const Plan& p, const GemmArgs& a, const Launch& L) {
  switch (p.wide_mb * 10 + p.wide_pairs) {
    case 21: return launch_wide<2, 1>(p, a, L);
    case 22: return launch_wide<2, 2>(p, a, L);
    case 41: return launch_wide<4, 1>(p, a, L);
    case 42: return launch_wide<4, 2>(p, a, L);
    case 81: return launch_wide<8, 1>(p, a, L);
#ifdef QUICK_AMD_TOOLS
    default: return launch_wide<8, 2>(p, a, L);   // r02's hipcc-scheduled 256 x 256 tile (92 bytes of scratch): the A/B partner of the generated loop, tools builds only
#else
    default: return false;   // (... which the product library does not carry: it runs the generated loop, w4a16_xw.hpp, or 128 x 256 tiles)
#endif
  }
}

}  // namespace quick_amd
