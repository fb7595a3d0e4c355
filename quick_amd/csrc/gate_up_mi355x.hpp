// What one lane of gate_up_mi355x (repack.hip) does, as a function of its workgroup and thread index, so that a host program can walk the
// same indices over heap buffers of the exact sizes (tools/gate_up_host_check.py; a plain C++ compiler gets __host__, __device__ and
// __forceinline__ defined away by that program).  Pure data movement: 16-byte pieces in, 16-byte pieces out.
#pragma once
#include <cstddef>
#include <cstdint>

namespace quick_amd {

typedef uint32_t gate_up_piece __attribute__((ext_vector_type(4)));     // = u32x4 (w4a16_common.hpp)

// Workgroups [0, wblocks): weights, [wblocks, wblocks + sblocks): scale words, the rest: the plain zero-point copy.  Sizes in pieces:
// fused qweight K * I / 16, fused scales NG * I / 2, fused qzeros NG * I / 8; a projection holds half of each.  K % 128 == 0, I % 64 == 0.
template <bool kSplit>
__host__ __device__ __forceinline__ void gate_up_mi355x_lane(gate_up_piece* __restrict__ gate_qw, gate_up_piece* __restrict__ gate_sc, gate_up_piece* __restrict__ gate_qz,
                                          gate_up_piece* __restrict__ up_qw, gate_up_piece* __restrict__ up_sc, gate_up_piece* __restrict__ up_qz,
                                          gate_up_piece* __restrict__ fused_qw, gate_up_piece* __restrict__ fused_sc,
                                          gate_up_piece* __restrict__ fused_qz, int K, int I, int NG, unsigned wblocks, unsigned sblocks,
                                          unsigned block, unsigned thread) {
  if (block < wblocks + sblocks) {
    const bool weights = block < wblocks;
    // weights: a run of 8 pieces = (tile, k tile, quarter, gate | up); scale words: a run of 2 pieces = (tile, group, gate | up)
    const int per_run = weights ? 8 : 2, inner = weights ? 4 * (K >> 7) : NG;
    const size_t p = (size_t)(block - (weights ? 0u : wblocks)) * 256 + thread;
    const size_t total = weights ? (size_t)K * I / 16 : (size_t)NG * I / 2;
    if (p >= total) return;
    const int i = (int)(p % per_run);
    const size_t run = p / per_run;
    const bool is_up = run & 1;
    const size_t row = run >> 1;                       // T * inner + (kt * 4 + q | g), T = the fused channel tile
    const size_t T = row / inner, r = row % inner;
    const size_t part = ((((T >> 1) * inner + r) << 1) + (T & 1)) * per_run + i;
    gate_up_piece* fused = weights ? fused_qw : fused_sc;
    gate_up_piece* proj = weights ? (is_up ? up_qw : gate_qw) : (is_up ? up_sc : gate_sc);
    if (kSplit) proj[part] = fused[p];
    else fused[p] = proj[part];
    return;
  }
  // zero points: I / 16 lanes per group row, each owning two fused pieces (of I / 8 a row) and one piece of each projection (of I / 16)
  const size_t idx = (size_t)(block - wblocks - sblocks) * 256 + thread;
  const int lanes = I >> 4;
  if (idx >= (size_t)NG * lanes) return;
  const size_t g = idx / lanes;
  const int j = (int)(idx % lanes);
  const size_t f = g * (size_t)(I >> 3) + 2 * j, s = g * (size_t)lanes + j;
  const gate_up_piece zero = {0u, 0u, 0u, 0u};
  if (j >= (I >> 5)) {                                 // the half of every row that holds no channels
    if (kSplit) gate_qz[s] = zero, up_qz[s] = zero;
    else fused_qz[f] = zero, fused_qz[f + 1] = zero;
  } else if (kSplit) {
    const gate_up_piece a = fused_qz[f], b = fused_qz[f + 1];
    gate_qz[s] = gate_up_piece{a[0], a[2], b[0], b[2]};
    up_qz[s] = gate_up_piece{a[1], a[3], b[1], b[3]};
  } else {
    const gate_up_piece a = gate_qz[s], b = up_qz[s];
    fused_qz[f] = gate_up_piece{a[0], b[0], a[1], b[1]};
    fused_qz[f + 1] = gate_up_piece{a[2], b[2], a[3], b[3]};
  }
}

}  // namespace quick_amd
