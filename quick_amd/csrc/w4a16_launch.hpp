// Host-side launch path of the W4A16 GEMM: where a launch goes (Launch), the one way a GEMM kernel is started (launch_kernel) and the
// launchers of the skinny, tiled and wide families (w4a16_skinny.hip, w4a16_tiled.hip, w4a16_wide.hip) for the dispatcher (w4a16_gemm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "w4a16_args.hpp"

namespace quick_amd {

struct Plan;

// Where the main kernel goes: the stream, plus an optional event pair bound to that one dispatch
// so that a profiler-free caller can read the kernel's own duration.
struct Launch {
  hipStream_t st;
  hipEvent_t start, stop;
  unsigned long long* span = nullptr;  // device [2]: in-kernel span of this launch (see span_stamp)
  unsigned flags = 0;                  // extended-launch flags (experiment builds only)
};

// Raises KFN's dynamic-LDS limit to `lds_limit` once per device (lds_limit_once; the static word is this instantiation's own, one per
// kernel) and starts it on L's stream, bound to L's event pair.  Every GEMM kernel of the library starts here.
template <auto KFN, typename... Args>
inline void launch_kernel(const Launch& L, dim3 grid, dim3 block, unsigned lds, int lds_limit, Args... args) {
  static std::atomic<unsigned long long> attr_set{0};
  (void)lds_limit_once(attr_set, (const void*)KFN, lds_limit);
  hipExtLaunchKernelGGL(KFN, grid, block, lds, L.st, L.start, L.stop, L.flags, args...);
}

// ... for the kernels whose arguments are the leading scalars + XwRest (w4a16_args.hpp) and whose LDS limit is what they ask for
template <auto KFN>
inline bool launch_kernel_xw(const Launch& L, dim3 grid, dim3 block, unsigned lds, const GemmArgs& a) {
  const XwRest rest{a.bias, a.residual, a.Y, a.slabs, a.counters, a.dbg, a.span, a.silu_mul, a.G};
  launch_kernel<KFN>(L, grid, block, lds, (int)lds, a.X, a.QW, a.S, a.M, a.K, a.N, a.tpg, a.ksplit, a.kt_per_split, a.xcd_gm, rest);
  return true;
}

// The launchers of the three hipcc-scheduled families.  Each picks the instantiation the plan names and starts it; false: no build for
// this request (span stamps asked of a kernel without them, the tools-only 256 x 256 wide tile in a product build) and NOTHING was launched.
bool skinny_launch(const Plan& p, const GemmArgs& a, const Launch& L);
bool tiled_launch(const Plan& p, const GemmArgs& a, const Launch& L);
bool wide_launch(const Plan& p, const GemmArgs& a, const Launch& L);

}  // namespace quick_amd
