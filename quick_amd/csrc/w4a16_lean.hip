// Lean small-M kernels (w4a16_lean.hpp): the launcher.  The kernels themselves are instantiated in w4a16_lean_a/b/c.hip.
#include "w4a16_common.hpp"

#include <algorithm>

#include "w4a16_args.hpp"
#include "w4a16_lean.hpp"
#include "w4a16_lean_host.hpp"

namespace quick_amd {

template <int WAVES, int TMAX, int NTW, int ABL>
bool lean_build(const GemmArgs& a, int grid_x, int grid_y, const Launch& L);

unsigned lean_lds_need(int M, int K, int waves, int ntw, bool ln, bool persist) { return lean_lds_bytes(std::min(M, 16), K, waves, ntw, ln, persist); }

template <int ABL>
static bool lean_go_w(int waves, int tmax, int ntw, const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  switch (waves * 1000 + tmax * 10 + ntw) {
#define QA_LEAN_CASE(W, T, C) \
  case W * 1000 + T * 10 + C: return lean_build<W, T, C, ABL>(a, grid_x, grid_y, L)
    QA_LEAN_CASE(8, 4, 1);
    QA_LEAN_CASE(8, 4, 2);
    QA_LEAN_CASE(8, 8, 1);
    QA_LEAN_CASE(8, 12, 1);
    QA_LEAN_CASE(16, 4, 1);
    QA_LEAN_CASE(16, 4, 2);
    QA_LEAN_CASE(16, 8, 1);
#undef QA_LEAN_CASE
    default: return false;
  }
}

bool lean_launch(int waves, int tmax, int ntw, int abl, const GemmArgs& a, int grid_x, int grid_y, const Launch& L) {
  if (a.G % 128 != 0 || (a.K >> 7) < waves || ((a.K >> 7) + waves - 1) / waves > tmax || (a.N >> 4) % ntw != 0) return false;
  switch (abl) {
    case 0: return lean_go_w<0>(waves, tmax, ntw, a, grid_x, grid_y, L);
    case 32: return lean_go_w<32>(waves, tmax, ntw, a, grid_x, grid_y, L);
#ifdef QUICK_AMD_TOOLS
    case 64: return lean_go_w<64>(waves, tmax, ntw, a, grid_x, grid_y, L);
#endif
    default: return false;
  }
}

}  // namespace quick_amd
