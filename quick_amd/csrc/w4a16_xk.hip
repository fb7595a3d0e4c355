// Exchange-K kernels: instantiations and launcher (see w4a16_xk.hpp).  Its own translation unit so that the library builds in parallel.
#include "w4a16_common.hpp"

#include "w4a16_args.hpp"
#include "w4a16_wide.hpp"
#include "w4a16_xk.hpp"
#include "w4a16_xk_host.hpp"

namespace quick_amd {

static_assert(kXkZoneBytesHost == kXkZoneBytes, "exchange zone size");

XkConfig xk_default_config(int mb, int s) { return XkConfig{mb, s, 5, 4, 0}; }

template <int MB, int NBUF, int WD, int S, int ABL = 0, int KQ = 2>
static bool xk_go(const GemmArgs& a, int workgroups, const Launch& L) {
  constexpr unsigned lds = NBUF * MB * 8192 * (KQ / 2);
  const dim3 grid(workgroups), block(KQ == 4 ? 1024 : ((ABL & 4096) ? 768 : 512));
  const int gm = a.G == 128 ? 0 : (a.G % 128 == 0 ? 1 : -1);
  if (gm < 0) return false;
  if (gm == 0) return launch_kernel_xw<w4a16_xk_kernel<MB, 0, NBUF, WD, S, ABL, KQ>>(L, grid, block, lds, a);
  if constexpr (ABL == 0) return launch_kernel_xw<w4a16_xk_kernel<MB, 1, NBUF, WD, S, ABL, KQ>>(L, grid, block, lds, a);
  return false;  // timing experiments: G = 128 only
}

template <int MB, int S, int ABL = 0>
static bool xl_go(const GemmArgs& a, int workgroups, const Launch& L) {
  constexpr unsigned lds = (MB == 2 ? 4 : 3) * MB * 8192 + 5 * (8192 + 512);
  const dim3 grid(workgroups), block(768);
  const int gm = a.G == 128 ? 0 : (a.G % 128 == 0 ? 1 : -1);
  if (gm < 0) return false;
  if (gm == 0) return launch_kernel_xw<w4a16_xl_kernel<MB, 0, S, ABL>>(L, grid, block, lds, a);
  if constexpr (ABL == 0) return launch_kernel_xw<w4a16_xl_kernel<MB, 1, S, ABL>>(L, grid, block, lds, a);
  return false;
}

template <int MB, int ABL = 0>
static bool xl_go_s(int s, const GemmArgs& a, int workgroups, const Launch& L) {
  switch (s) {
    case 1: return xl_go<MB, 1, ABL>(a, workgroups, L);
    case 2: return xl_go<MB, 2, ABL>(a, workgroups, L);
    case 4: return xl_go<MB, 4, ABL>(a, workgroups, L);
    case 8: return xl_go<MB, 8, ABL>(a, workgroups, L);
    default: return false;
  }
}

template <int MB, int NBUF, int WD, int ABL = 0>
static bool xk_go_s(int s, const GemmArgs& a, int workgroups, const Launch& L) {
  switch (s) {
    case 1: return xk_go<MB, NBUF, WD, 1, ABL>(a, workgroups, L);
    case 2: return xk_go<MB, NBUF, WD, 2, ABL>(a, workgroups, L);
    case 4: return xk_go<MB, NBUF, WD, 4, ABL>(a, workgroups, L);
    case 8: return xk_go<MB, NBUF, WD, 8, ABL>(a, workgroups, L);
    default: return false;
  }
}

bool xk_launch(const XkConfig& c, const GemmArgs& a, int workgroups, const Launch& L) {
  if (c.loader) {  // twelve waves: four loaders + eight compute waves (an experiment the product library does not carry)
#ifdef QUICK_AMD_TOOLS
    if (c.abl == 0) return c.mb == 4 ? xl_go_s<4>(c.s, a, workgroups, L) : (c.mb == 2 ? xl_go_s<2>(c.s, a, workgroups, L) : false);
    if (c.abl == 32) {
      if (c.mb == 2 && c.s == 1) return xl_go<2, 1, 32>(a, workgroups, L);
      if (c.mb == 4 && c.s == 2) return xl_go<4, 2, 32>(a, workgroups, L);
      if (c.mb == 4 && c.s == 1) return xl_go<4, 1, 32>(a, workgroups, L);
      return false;
    }
    if (c.abl == 64) {
      if (c.mb == 2 && c.s == 1) return xl_go<2, 1, 64>(a, workgroups, L);
      if (c.mb == 4 && c.s == 2) return xl_go<4, 2, 64>(a, workgroups, L);
      if (c.mb == 4 && c.s == 4) return xl_go<4, 4, 64>(a, workgroups, L);
      if (c.mb == 2 && c.s == 8) return xl_go<2, 8, 64>(a, workgroups, L);
    }
#endif
    return false;
  }
  if (c.kq == 4) {  // sixteen waves, four per SIMD (an experiment the product library does not carry: level with eight waves)
#ifdef QUICK_AMD_TOOLS
    if (c.mb != 2 || c.s != 1 || c.nbuf != 5 || c.wd != 4) return false;
    if (c.abl == 0) return xk_go<2, 5, 4, 1, 0, 4>(a, workgroups, L);
    if (c.abl == 32) return xk_go<2, 5, 4, 1, 32, 4>(a, workgroups, L);
    if (c.abl == 64) return xk_go<2, 5, 4, 1, 64, 4>(a, workgroups, L);
    if (c.abl == 262208) return xk_go<2, 5, 4, 1, 262208, 4>(a, workgroups, L);  // the two halves in step (no skew)
#endif
    return false;
  }
  const int key = c.mb * 100 + c.nbuf * 10 + c.wd;
#ifdef QUICK_AMD_TOOLS
  if (c.abl) {  // timing experiments (tools builds): phase stamps, and the launch without the cross-CU exchange (wrong results)
    if (key == 454 && c.s == 2) switch (c.abl) {   // (all with phase stamps: tools/xk_phases.py reads the K loop's own time)
      case 64: return xk_go<4, 5, 4, 2, 64>(a, workgroups, L);
      case 65: return xk_go<4, 5, 4, 2, 65>(a, workgroups, L);    // loads only
      case 66: return xk_go<4, 5, 4, 2, 66>(a, workgroups, L);    // no loads
      case 82: return xk_go<4, 5, 4, 2, 82>(a, workgroups, L);    // no loads, no B-fragment reads
      case 74: return xk_go<4, 5, 4, 2, 74>(a, workgroups, L);    // no loads, no dequantisation
      case 90: return xk_go<4, 5, 4, 2, 90>(a, workgroups, L);    // MFMAs + barrier
      case 98: return xk_go<4, 5, 4, 2, 98>(a, workgroups, L);    // no loads, no barrier
      case 122: return xk_go<4, 5, 4, 2, 122>(a, workgroups, L);  // MFMAs only
      case 68: return xk_go<4, 5, 4, 2, 68>(a, workgroups, L);    // no cross-CU exchange
      case 192: return xk_go<4, 5, 4, 2, 192>(a, workgroups, L);  // no counted wait at the end of a stage
      case 320: return xk_go<4, 5, 4, 2, 320>(a, workgroups, L);  // no x pieces in the K loop
      case 576: return xk_go<4, 5, 4, 2, 576>(a, workgroups, L);  // no weight loads in the K loop
      case 1088: return xk_go<4, 5, 4, 2, 1088>(a, workgroups, L);  // one x piece with every unit
      case 4160: return xk_go<4, 5, 4, 2, 4160>(a, workgroups, L);  // four loader waves issue the x pieces
      case 4672: return xk_go<4, 5, 4, 2, 4672>(a, workgroups, L);  // ... and the compute waves issue no weight loads either
      case 8256: return xk_go<4, 5, 4, 2, 8256>(a, workgroups, L);  // + clocks spent in the counted wait / at the barrier
      case 8258: return xk_go<4, 5, 4, 2, 8258>(a, workgroups, L);  // ... without loads
      case 16720: return xk_go<4, 5, 4, 2, 16720>(a, workgroups, L);  // weight loads only, always the same (cached) stage, no B-fragment reads
      case 80: return xk_go<4, 5, 4, 2, 80>(a, workgroups, L);      // loads, no B-fragment reads
      case 72: return xk_go<4, 5, 4, 2, 72>(a, workgroups, L);      // loads, no dequantisation
      case 88: return xk_go<4, 5, 4, 2, 88>(a, workgroups, L);      // loads, MFMAs, barrier
      case 336: return xk_go<4, 5, 4, 2, 336>(a, workgroups, L);    // weight loads only, no B-fragment reads
      default: return false;
    }
    if (key == 254 && c.s == 1 && c.abl == 65536) return xk_go<2, 5, 4, 1, 65536>(a, workgroups, L);  // staggered issue
    if (key == 254 && c.s == 1 && c.abl == 65600) return xk_go<2, 5, 4, 1, 65600>(a, workgroups, L);
    if (key == 454 && c.s == 2 && c.abl == 65536) return xk_go<4, 5, 4, 2, 65536>(a, workgroups, L);
    if (key == 454 && c.s == 2 && c.abl == 65600) return xk_go<4, 5, 4, 2, 65600>(a, workgroups, L);
    if (key == 254 && c.s == 1 && c.abl == 131072) return xk_go<2, 5, 4, 1, 131072>(a, workgroups, L);  // <= 128 registers: two workgroups per CU
    if (key == 254 && c.s == 1 && c.abl == 131136) return xk_go<2, 5, 4, 1, 131136>(a, workgroups, L);
    if (key == 244 && c.s == 1 && c.abl == 131072) return xk_go<2, 4, 4, 1, 131072>(a, workgroups, L);
    if (key == 244 && c.s == 1 && c.abl == 131136) return xk_go<2, 4, 4, 1, 131136>(a, workgroups, L);
    if (key == 244 && c.s == 1 && c.abl == 64) return xk_go<2, 4, 4, 1, 64>(a, workgroups, L);
    if (key == 254 && c.s == 1 && c.abl == 524352) return xk_go<2, 5, 4, 1, 524352>(a, workgroups, L);    // a barrier behind every second stage only
    if (key == 254 && c.s == 1 && c.abl == 1572928) return xk_go<2, 5, 4, 1, 1572928>(a, workgroups, L);  // ... every fourth
    if (key == 454 && c.s == 2 && c.abl == 524352) return xk_go<4, 5, 4, 2, 524352>(a, workgroups, L);
    if (key == 254 && c.s == 1 && c.abl == 32768) return xk_go<2, 5, 4, 1, 32768>(a, workgroups, L);  // write-through y stores
    if (key == 254 && c.s == 1 && c.abl == 64) return xk_go<2, 5, 4, 1, 64>(a, workgroups, L);
    if (key == 454 && c.s == 4 && c.abl == 64) return xk_go<4, 5, 4, 4, 64>(a, workgroups, L);
    if (key == 254 && c.s == 8 && c.abl == 64) return xk_go<2, 5, 4, 8, 64>(a, workgroups, L);
    return false;
  }
  // ring / queue geometries that only the tuning sweeps ask for
  if (key == 444) return xk_go_s<4, 4, 4>(c.s, a, workgroups, L);
  if (key == 445) return xk_go_s<4, 4, 5>(c.s, a, workgroups, L);
  if (key == 455) return xk_go_s<4, 5, 5>(c.s, a, workgroups, L);
  if (key == 456) return xk_go_s<4, 5, 6>(c.s, a, workgroups, L);
  if (key == 244) return xk_go_s<2, 4, 4>(c.s, a, workgroups, L);
#else
  if (c.abl && c.abl != 32) return false;
#endif
  if (c.abl == 32) {  // in-kernel span stamps (quick_w4a16_gemm_span, bench.py): the shapes of the BASELINE sweep and their neighbours
    if (key == 254 && c.s == 1) return xk_go<2, 5, 4, 1, 32>(a, workgroups, L);
    if (key == 254 && c.s == 2) return xk_go<2, 5, 4, 2, 32>(a, workgroups, L);
    if (key == 254 && c.s == 4) return xk_go<2, 5, 4, 4, 32>(a, workgroups, L);
    if (key == 454 && c.s == 1) return xk_go<4, 5, 4, 1, 32>(a, workgroups, L);
    if (key == 454 && c.s == 2) return xk_go<4, 5, 4, 2, 32>(a, workgroups, L);
    return false;
  }
  if (key == 454) return xk_go_s<4, 5, 4>(c.s, a, workgroups, L);
  if (key == 254) return xk_go_s<2, 5, 4>(c.s, a, workgroups, L);
  return false;
}

}  // namespace quick_amd
