// Host-side interface of the GEMM planner (w4a16_plan.hip): what a W4A16 launch runs -- family, tile, K split, workspace -- for a shape
// and a kernel id.  Used by the families' launchers (w4a16_skinny.hip, w4a16_tiled.hip, w4a16_wide.hip) and the dispatcher and entry points in w4a16_gemm.hip.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/quick_amd.h"
#include "w4a16_xk_host.hpp"

namespace quick_amd {

constexpr size_t kLdsPerCu = 160 * 1024;  // gfx950

// The fields of a kernel id (include/quick_amd.h, "kernel id"); what a field means depends on the family, 0 = the planner's choice
struct KernelId {
  int family;        // bits 0-3: QUICK_KERNEL_*
  int mt;            // bits 4-7: channel tiles (SKINNY, LEAN) / token tiles (TILED, WIDE, XK, XW) per workgroup; XM: channel pairs per workgroup
  int n8, waves;     // bits 8-11, and x 4: waves per workgroup (SKINNY, TILED, LEAN); WIDE: pairs per wave; XK / XW: K slices
  int xm_tile;       // bits 8-9: XM 32- (1) / 64-token (2) tiles
  bool b12;          // bit 12: SKINNY no LDS copy of x; WIDE no ring; XK loader waves; XW 128-channel tiles
  bool b13;          // bit 13: XK sixteen waves; TILED retired
  bool plain_order;  // bit 14: no XCD-aware tile order
  bool b15;          // bit 15: TILED 2 x 4 wave grid; WIDE eight waves
  int ablate;        // bits 16-20: timing experiments (QUICK_AMD_TOOLS builds)
  bool flip;         // bit 21: SKINNY flips the persistence default
  int slots;         // bits 22-24: SKINNY / LEAN persistent slots per CU; WIDE ring slots; XK x ring slots
  int poll_log2;     // bits 22-26: XW log2 of the exchange poll limit
  bool exact;        // bit 25: SKINNY exact dequantisation
  bool force_table;  // bit 26: SKINNY the table deferred-zero path
  int xk_wd;         // bits 26-28: XK weight queue depth
  bool force_big;    // bit 27: TILED 128 x 256 four-wave tiles
  bool no_frag;      // bit 28: SKINNY no fragment deferred-zero path
  bool force256;     // bit 29: TILED 256-channel tiles
  bool forbid256;    // bit 30: TILED no 256-channel tiles
  bool high;         // any bit from 12 up
  int xw_stagger;    // bits 27-28: XW staggered K ranges of the two-slice 128 x 128 launch, d = 1..3 (0 = today's launch)
};
inline KernelId decode_kernel_id(int k) {
  return {k & 15, (k >> 4) & 15, (k >> 8) & 15, ((k >> 8) & 15) * 4, (k >> 8) & 3, ((k >> 12) & 1) != 0, ((k >> 13) & 1) != 0, ((k >> 14) & 1) != 0,
          ((k >> 15) & 1) != 0, (k >> 16) & 31, ((k >> 21) & 1) != 0, (k >> 22) & 7, (k >> 22) & 31, ((k >> 25) & 1) != 0, ((k >> 26) & 1) != 0,
          (k >> 26) & 7, ((k >> 27) & 1) != 0, ((k >> 28) & 1) != 0, ((k >> 29) & 1) != 0, ((k >> 30) & 1) != 0, (k >> 12) != 0, (k >> 27) & 3};
}

struct Plan {
  int kernel;  // QUICK_KERNEL_SKINNY / QUICK_KERNEL_TILED / QUICK_KERNEL_WIDE
  int wide_mb, wide_pairs;  // wide: token tiles of 32 per workgroup, 32-channel pairs per wave
  int wide_nbuf;            // wide: LDS ring slots (>= 3: w4a16_ring_kernel, everything by LDS-DMA; 0: w4a16_wide_kernel)
  int mt;      // skinny: channel tiles (of 16) per workgroup, NTW; tiled: token tiles per workgroup, BMT
  int waves;   // skinny: waves per workgroup
  bool xlds;   // skinny: x through an LDS copy
  int grid_x;  // skinny: workgroups along the channel blocks; fewer than the blocks = persistent workgroups
  bool dz;     // skinny: deferred-zero compute; with xlds the table flavour (NTW = 1), without the fragment flavour
  int ksplit;  // K slices across workgroups, reduced in-kernel by the last arriver
  int ntiles;  // output tiles (one arrival counter each)
  size_t slab_floats;  // fp32 elements of one partial tile
  int kt_per_split;
  int ablate;  // kernel bits 16-20: ablation variant of the tiled kernel (timing experiments only)
  int xcd_gm;  // tiled: rows of the XCD grid over the tile grid (0 = plain order)
  bool wn2;    // tiled: 2 x 4 wave grid (kernel bit 15)
  int tch;     // tiled: channels per workgroup tile, 128 or 256
  int xk_nbuf, xk_wd;  // exchange-K: x ring slots, weight queue depth (wide_mb = token tiles of 32, ksplit = slices that exchange)
  bool xk_loader;      // exchange-K: the twelve-wave flavour (four loader waves; kernel bit 12)
  int xk_kq;           // exchange-K: K groups of waves per workgroup, 2 (eight waves) or 4 (sixteen; kernel bit 13)
  int xw_stagger;      // XW, 128 x 128 tiles with two slices: stagger d of the slices' K ranges in 128-k stages (w4a16_xw.hpp), 0 = none
  int poll_log2;       // XW: log2 of the ticks (10 ns) a wave waits for a partner slice before it gives its block up (0 = the kernel's default)
  int lean_tmax;       // LEAN: the most k tiles a wave may own (the build's register ring), 0 = no build for this shape
  int frag8_t;         // SKINNY, mt == 8: k tiles per wave of the straight-line eight-tile fragment kernel (w4a16_frag8_kernel), 0 = not that kernel
  double est_us, est_xw_us;  // launch-time model: the r02 / r03 candidates' minimum, the four-wave kernels' minimum (0 = not evaluated)
};

// The plan of a launch; silu: the launch carries SiLU * mul, with_ln: an RMSNorm prologue (AUTO keeps to the kernels that have one)
Plan plan_for(int M, int K, int N, int G, int kernel, int grid_split_k, bool silu, bool with_ln);
// workspace bytes a launch needs, with or without SiLU * mul
size_t plan_workspace_bytes(int M, int K, int N, int G, int kernel, int grid_split_k);
// the plan's kernel carries an RMSNorm prologue
bool plan_takes_rmsnorm(const Plan& p);
// the text of quick_w4a16_plan_describe (valid shapes, text_bytes > 0)
void plan_describe(int M, int K, int N, int G, int kernel, int grid_split_k, char* text, size_t text_bytes);

// workspace: [64 KiB of arrival counters, one per output tile][exchange zone][ntiles * ksplit fp32 slabs]
// The counter region has a FIXED size: the slabs are not handed back zeroed, so a region that grew with the tile count
// would lay the counters of one launch over the stale partial sums of an earlier, smaller one.
constexpr int kMaxSplitTiles = 16384;
inline size_t counters_bytes(const Plan&) { return (size_t)kMaxSplitTiles * 4; }
// ... and behind the counters a FIXED 16 MiB "exchange zone": the mailboxes of the exchange-K kernels (w4a16_xk.hpp), all-zero
// between launches (every consumer zeroes what it has read); the slabs of the last-arriver kernels start behind it and never
// touch it.  Layout: [64 KiB counters][16 MiB exchange zone][ntiles * ksplit fp32 slabs].
inline size_t slabs_offset(const Plan& p) { return counters_bytes(p) + kXkZoneBytesHost; }
inline size_t workspace_need(const Plan& p) {
  if (p.ksplit <= 1) return 0;
  if (p.kernel == QUICK_KERNEL_XK || p.kernel == QUICK_KERNEL_XW) return slabs_offset(p);
  return slabs_offset(p) + (size_t)p.ntiles * p.ksplit * p.slab_floats * sizeof(float);
}

// SiLU * mul in an exchange-K launch needs every wave to finish whole 32-token blocks (w4a16_xk.hpp, the way out)
inline bool xk_takes_silu(const Plan& p) { return (p.wide_mb / 2 * 16) % (16 * p.ksplit) == 0; }

// ring slots that fit the 160 KiB of LDS for a (MB, PAIRS) tile at one (scale, zero) word per pair and stage (G % 128 == 0);
// wk = waves along K (1: four waves, 2: eight)
constexpr int wide_ring_nbuf(int mb, int pairs, int wk = 1) {
  const int slot = mb * 8192 + pairs * 8192 + wk * pairs * 1024;
  const int n = (160 * 1024) / slot;
  return n > 6 ? 6 : n;
}

// LDS of one skinny workgroup: reduction buffer(s), the x copy, the deferred-zero table
inline size_t skinny_lds_bytes(int M, int G, int ntw, int waves, int kt_per_split, bool persistent, bool xlds, bool dz) {
  size_t b = (size_t)(persistent ? 2 : 1) * waves * ntw * 1024;
  if (xlds) b += (size_t)std::min(M, 16) * (kt_per_split * 256 + 16);
  if (dz) b += (size_t)kt_per_split * (G >= 128 ? 1 : (G == 64 ? 2 : 4)) * 128;
  return b;
}

inline int group_mode(int G) { return G == 128 ? 0 : (G % 128 == 0 ? 1 : (G == 64 ? 2 : (G == 32 ? 3 : 4))); }

}  // namespace quick_amd
