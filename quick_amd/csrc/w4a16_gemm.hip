// W4A16 GEMM for MI355X (gfx950): y[M,N] = x[M,K] @ fp16((w - z) * s).
//
// Replaces the five __global__ kernels + host dispatcher of the reference
// (csrc/gemm_cuda_quick.cu:1199-1517) with a design made for CDNA4:
//   * weights are the MFMA *A* operand (rows = output channels), activations the *B* operand, so
//     the accumulator fragment of a lane is 4 consecutive output channels of one token -> 8-byte
//     row-major stores with no transpose;
//   * the offline interleave ("mi355x order") makes one 16-byte global load per lane
//     deliver the A fragments of 4 consecutive k-steps of v_mfma_f32_16x16x32_f16: dequantised
//     weights go HBM -> VGPR -> matrix core, never through LDS (the QUICK idea, re-derived for the
//     64-lane MFMA operand order instead of mma.sync/ldmatrix);
//   * activations: skinny kernel (M <= 64) -- one 16-channel tile per workgroup, K split over the
//     workgroup's waves, x either broadcast from an LDS copy (tiny M) or loaded as fragments straight
//     from L2; tiled kernel (large M) -- 64 x 128 workgroup tile, x staged in LDS *in fragment order*
//     by global_load_lds, 8 waves = 4 along N x 2 along K.
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "w4a16_args.hpp"
#include "w4a16_wide.hpp"
#include "w4a16_xk_host.hpp"
#include "w4a16_xw_host.hpp"
#include "w4a16_lean_host.hpp"
#include "w4a16_xm_host.hpp"
#include "w4a16_plan.hpp"
namespace quick_amd {

// ------------------------------------------------------------------------------------------------
// skinny kernel: one workgroup owns 16 tokens x (NTW*16) channels for the whole K; its waves split K (and
// blockIdx.z splits it further when the grid would not fill the chip).
// ------------------------------------------------------------------------------------------------
// Every wave walks its k-tiles in chunks of U.  A chunk is LOADED (weights 16 B/lane/tile straight from HBM, raw
// group constants, and -- unless x sits in LDS -- the B fragments from L2, once per k-step for all NTW channel
// tiles) one chunk ahead of being COMPUTED, into the other of two register sets; the sched_barriers keep hipcc
// from sinking the loads next to their uses, which would serialise one HBM round trip per tile.
// NTW trades workgroup count against x traffic: token blocks re-read the weights (L2 hits), channel blocks re-read
// x, so NTW ~ number of token blocks keeps both at N/16 workgroups' worth.
//
// XLDS: the workgroup first copies x[rows, kbegin:kend] into LDS with coalesced 16-byte loads (row pitch padded
// by 16 B so the token rows of a fragment read spread over the bank groups) and every B fragment is a
// ds_read_b128 -- for M == 1 a 4-address broadcast -- instead of a 64-lane global load fetching 64 B per token
// row, 15/16 of them wasted when M == 1.
template <int NTW, int GM, int U, bool XLDS, bool LN = false>
struct SkinnyChunk {
  u32x4 w[U][NTW];
  GroupRaw raw[U][NTW][groups_per_tile<GM>()];
  half8_t xf[XLDS ? 1 : U][XLDS ? 1 : 4];
  half8_t gf[LN ? U : 1][LN ? 4 : 1];  // RMSNorm weight fragments (LN: the norm is applied to the x fragments in registers)
};

// Weights and group constants come in through buffer loads: address = descriptor base + per-lane byte offset (a launch
// constant VGPR) + a wave-uniform byte offset in an SGPR -- no 64-bit address arithmetic per load (it was ~28 scalar and
// ~10 vector instructions per 1 KiB weight tile).  Offsets are 32-bit: tensors up to 4 GiB.
struct SkinnyBufs {
  __amdgpu_buffer_rsrc_t w, s;
  unsigned w_voff, s_voff;  // lane * 16;  4 * n16 (this lane's channel within its 16-channel block)
  unsigned wstride_bytes;   // between consecutive channel tiles of the weights
  unsigned sstride_bytes;   // between consecutive channel tiles of the (scale, zero point) words: groups * 64
};
__device__ __forceinline__ SkinnyBufs skinny_bufs(const GemmArgs& a, int lane) {
  SkinnyBufs b;
  const unsigned groups = (unsigned)(a.K / a.G);
  b.w = __builtin_amdgcn_make_buffer_rsrc((void*)a.QW, 0, (unsigned)((size_t)a.K * a.N / 2), 0x00020000);
  b.s = __builtin_amdgcn_make_buffer_rsrc((void*)a.S, 0, groups * (unsigned)a.N * 4u, 0x00020000);
  b.w_voff = (unsigned)lane * 16u;
  b.s_voff = 4u * (unsigned)(lane & 15);
  b.wstride_bytes = (unsigned)(a.K >> 7) * 1024u;
  b.sstride_bytes = groups * 64u;
  return b;
}

// chunk of U k-tiles starting at kt of channel block `cb` (in units of 16 channels: block index * NTW)
// NT: the weight requests carry the nt (streaming) cache policy -- launches with ONE token block, where every weight byte is read once
// [r05 A/B builds, profiles/r05_ab_skinny_nt.txt: 1 x 28672 x 8192 24.0 -> 21.9 us, 16 x 8192 x 57344 59.3 -> 57.5, Llama-2-70B bs = 16 1358 -> 1379 tok/s;
// with two token blocks the second one's re-read misses L2: 32 x 4096 x 8192 8.6 -> 9.1, so those keep the default policy]
template <int NTW, int GM, int U, bool XLDS, bool LN = false, bool NT = false>
__device__ __forceinline__ void skinny_load(SkinnyChunk<NTW, GM, U, XLDS, LN>& c, int kt, int kt_last, const SkinnyBufs& b,
                                            int cb, const half_t* xp, const GemmArgs& a, const half_t* gp = nullptr) {
  constexpr int NG = groups_per_tile<GM>();
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < NTW; ++j)  // past the end: replay
      c.w[u][j] = __builtin_amdgcn_raw_buffer_load_b128(b.w, b.w_voff, (unsigned)(cb + j) * b.wstride_bytes + (unsigned)min(kt + u, kt_last) * 1024u, NT ? 2 : 0);
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const unsigned g = (unsigned)group_index<GM>(min(kt + u, kt_last), i * (4 / NG), a.tpg, a.G);
        c.raw[u][j][i].sz = __builtin_amdgcn_raw_buffer_load_b32(b.s, b.s_voff, (unsigned)(cb + j) * b.sstride_bytes + g * 64u, 0);
      }
  if constexpr (!XLDS) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) c.xf[u][t] = *(const half8_t*)(xp + min(kt + u, kt_last) * 128 + 32 * t);
  }
  if constexpr (LN) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) c.gf[u][t] = *(const half8_t*)(gp + min(kt + u, kt_last) * 128 + 32 * t);
  }
}

template <int NTW, int GM, int U, bool XLDS>
__device__ __forceinline__ void skinny_compute(const SkinnyChunk<NTW, GM, U, XLDS>& c, int kt, int kt_end, const char* xl,
                                               floatx4 (&acc)[NTW]) {
  constexpr int NG = groups_per_tile<GM>();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kt + u < kt_end) {  // wave-uniform
      GroupQ grp[NTW][NG];
#pragma unroll
      for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < NG; ++i) grp[j][i] = make_group(c.raw[u][j][i]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        half8_t bf;
        if constexpr (XLDS) bf = *(const half8_t*)(xl + ((kt + u) * 128 + 32 * t) * 2);
        else bf = c.xf[u][t];
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = mfma16(dequant8(c.w[u][j][t], grp[j][group_slot<GM>(t)]), bf, acc[j]);
      }
    } else {
      // a skipped (replayed) tile still counts as consumed: otherwise hipcc's s_waitcnt pass carries its loads as
      // pending into the next iteration and stalls the next prefetch on the write-after-write hazard
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        asm volatile("" ::"v"(c.w[u][j]));
#pragma unroll
        for (int i = 0; i < NG; ++i) asm volatile("" ::"v"(c.raw[u][j][i].sz));
      }
      if constexpr (!XLDS) {
#pragma unroll
        for (int t = 0; t < 4; ++t) asm volatile("" ::"v"(c.xf[u][t]));
      }
    }
  }
}

// DEFERRED-ZERO compute (M <= 16, x in LDS).  The exact kernel spends 13 VALU ops per packed dword on fp16((w - z) * s)
// and the matrix core hides none of them; at M <= 16 that, not HBM, bounds the kernel.  Here the roles of the MFMA
// operands are swapped -- x is the A operand (rows = tokens), the still-biased weights biased8() the B operand (columns =
// channels) -- so that a lane's accumulators are 4 tokens of ONE channel and the group constants are per-lane scalars:
//     y[m, n] = sum_units s[g, n] * ( sum_{k in unit} x[m, k] * (b_k + w[n, k])  -  C[unit, m]  -  z[g, n] * A[unit, m] )
// with b_k = 1024 or 64 (see biased8), A[unit, m] = sum_k x[m, k] and C[unit, m] = sum_k b_k x[m, k] tabulated once per
// workgroup while x is copied to LDS (`tab`: per unit 16 x A then 16 x -C, fp32).  A unit is min(G, 128) consecutive k.
// The accumulator of a unit starts at -C, so the epilogue of a unit is 2 FMAs per register.  5 VALU per dword plus
// ~12 per (unit, channel tile) instead of 13 + 5; products x * (b + w) are exact in the fp32 accumulator and w - z is
// never rounded to fp16, i.e. this path differs from the exact kernel by less than the latter's own weight rounding
// (2^-11 relative per weight) -- see DESIGN.md for the bound and tests/test_gemm_gpu.py for the comparison.
template <int NTW, int GM, int U>
__device__ __forceinline__ void skinny_compute_dz(const SkinnyChunk<NTW, GM, U, true>& c, int kt, int kt_end,
                                                  const char* xl, const float* tab,
                                                  floatx4 (&acc)[NTW]) {
  constexpr int NG = groups_per_tile<GM>();  // units per 128-k tile
  constexpr int TPU = 4 / NG;                // k-steps per unit
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kt + u < kt_end) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const float* tp = tab + ((kt + u) * NG + i) * 32;
        const floatx4 xa = *(const floatx4*)tp;
        const floatx4 nc = *(const floatx4*)(tp + 16);
        floatx4 g[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) g[j] = nc;
#pragma unroll
        for (int t = i * TPU; t < (i + 1) * TPU; ++t) {
          const half8_t xf = *(const half8_t*)(xl + ((kt + u) * 128 + 32 * t) * 2);
#pragma unroll
          for (int j = 0; j < NTW; ++j) g[j] = mfma16(xf, biased8(c.w[u][j][t]), g[j]);
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const float s = group_scale_f32(c.raw[u][j][i]), z = group_zero_f32(c.raw[u][j][i]);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[j][r] = __builtin_fmaf(s, __builtin_fmaf(-z, xa[r], g[j][r]), acc[j][r]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        asm volatile("" ::"v"(c.w[u][j]));
#pragma unroll
        for (int i = 0; i < NG; ++i) asm volatile("" ::"v"(c.raw[u][j][i].sz));
      }
    }
  }
}

// Deferred-zero compute WITHOUT the LDS copy of x (fragments straight from L2, any M <= 16 x NTW tiles): the unit sums
// A = sum_k x and C = sum_k b_k x come out of the matrix core too -- one extra MFMA per k-step, shared by the NTW channel
// tiles, with a CONSTANT B operand whose even columns are all ones and whose odd columns hold b_k (1024 / 64 in
// biased8's order) -- so an accumulator lane ends up with A (even channel lane) or C (odd channel lane) of its 4 tokens
// and gets the other from its neighbour with one DPP move.  ~12 VALU per unit per wave on top of 5 per packed dword and
// ~12 per (unit, channel tile); no table, no LDS, no per-workgroup prologue.
// LN: RMSNorm folded in -- the kernel sums the squares of its rows in a pass over x in front of the loop, and the x fragments
// are normalised in registers with quick_rmsnorm_f16's rounding points (rms_scale8: fp16(fp16(x * rstd) * w)).
template <int NTW, int GM, int U, bool LN = false>
__device__ __forceinline__ void skinny_compute_dzf(const SkinnyChunk<NTW, GM, U, false, LN>& c, int kt, int kt_end,
                                                   half8_t bconst, bool odd, floatx4 (&acc)[NTW],
                                                   float rstd = 0.f) {
  constexpr int NG = groups_per_tile<GM>();  // units per 128-k tile
  constexpr int TPU = 4 / NG;                // k-steps per unit
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (kt + u < kt_end) {  // wave-uniform
      half8_t xs[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if constexpr (LN) {
          xs[t] = rms_scale8(c.xf[u][t], rstd, c.gf[u][t]);
        } else {
          xs[t] = c.xf[u][t];
        }
      }
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        floatx4 sm = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = i * TPU; t < (i + 1) * TPU; ++t) sm = mfma16(xs[t], bconst, sm);
        floatx4 xa, nc;  // A and -C of this lane's 4 tokens
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float mine = sm[r];  // (a copy: __builtin_bit_cast of the vector element itself reads element 0)
          const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, mine), 0xB1, 0xf, 0xf, false));
          xa[r] = odd ? other : mine;
          nc[r] = -(odd ? mine : other);
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          floatx4 g = nc;
#pragma unroll
          for (int t = i * TPU; t < (i + 1) * TPU; ++t) g = mfma16(xs[t], biased8(c.w[u][j][t]), g);
          const float s = group_scale_f32(c.raw[u][j][i]), z = group_zero_f32(c.raw[u][j][i]);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[j][r] = __builtin_fmaf(s, __builtin_fmaf(-z, xa[r], g[r]), acc[j][r]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        asm volatile("" ::"v"(c.w[u][j]));
#pragma unroll
        for (int i = 0; i < NG; ++i) asm volatile("" ::"v"(c.raw[u][j][i].sz));
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) asm volatile("" ::"v"(c.xf[u][t]));
      if constexpr (LN) {
#pragma unroll
        for (int t = 0; t < 4; ++t) asm volatile("" ::"v"(c.gf[u][t]));
      }
    }
  }
}

// Finishes the channel block `nb`: the waves' K partials meet in LDS (buffer `red`), wave j < NTW adds them for
// channel tile j, joins the other K slices if there are any, applies the epilogue and stores.  Returns with `acc`
// zeroed for the next block.  One workgroup barrier (two more when K is split across workgroups).
// TR: the accumulators come from the deferred-zero path (lane = channel n16, registers = tokens 4q..4q+3) and are
// written to LDS transposed, so that everything after the barrier sees the usual fragment (lane = token, registers =
// channels 4q..4q+3).
template <int NTW, int WAVES, bool TR>
__device__ __forceinline__ void skinny_finish(const GemmArgs& a, floatx4 (&acc)[NTW], floatx4* red, char* smem, int nb,
                                              int nblocks, int mb, int ks, int lane, int wave) {
  const int n16 = lane & 15, q = lane >> 4;
  if constexpr (TR && NTW == 1) {
    if (a.ksplit == 1) {
      // Deferred-zero path, K not split across workgroups: every wave finishes its own 16 / WAVES tokens (lane = one
      // output), so no wave does the whole reduction while the others wait for it at the next block's barrier.
      // Partials in LDS row-major [wave][token][channel].
      float* rf = (float*)(red + wave * 64) + 64 * q + n16;
#pragma unroll
      for (int r = 0; r < 4; ++r) rf[16 * r] = acc[0][r];
      acc[0] = floatx4{0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      constexpr int TPW = WAVES >= 16 ? 1 : 16 / WAVES;  // tokens per wave
      const int t = min(wave * TPW + q, 15), m = mb * 16 + t;
      if (wave * TPW >= min(16, a.M - mb * 16)) return;  // whole waves: the shuffle below stays wave-wide
      const float* src = (const float*)red + t * 16 + n16;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) v += src[w * 256];
      const bool live = q < TPW && m < a.M;
      if (a.silu_mul) {
        const float up = __shfl_xor(v, 8);  // channels 0..7 gate, 8..15 up
        if (live && n16 < 8) a.Y[(size_t)m * (a.N >> 1) + nb * 8 + n16] = silu_mul_f16((half_t)v, (half_t)up);
        return;
      }
      if (live) {
        const int n = nb * 16 + n16;
        if (a.bias) v += (float)a.bias[n];
        half_t o = (half_t)v;  // the residual joins the ROUNDED product, as GEMM-then-add does
        if (a.residual) o = (half_t)((float)o + (float)a.residual[(size_t)m * a.N + n]);
        a.Y[(size_t)m * a.N + n] = o;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    if constexpr (TR) {
      float* rf = (float*)(red + (wave * NTW + j) * 64) + 64 * (n16 >> 2) + 16 * q + (n16 & 3);
#pragma unroll
      for (int r = 0; r < 4; ++r) rf[4 * r] = acc[j][r];
    } else {
      red[(wave * NTW + j) * 64 + lane] = acc[j];
    }
    acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  floatx4 sum = floatx4{0.f, 0.f, 0.f, 0.f};
  if (wave < NTW) {
    sum = red[wave * 64 + lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) sum += red[(w * NTW + wave) * 64 + lane];
  }
  if (a.ksplit > 1) {  // never combined with the persistent loop: this workgroup owns exactly one block
    const int tile = mb * nblocks + nb;
    constexpr unsigned SLAB_BYTES = NTW * 1024;
    const __amdgpu_buffer_rsrc_t rs = slab_rsrc(a.slabs + (size_t)tile * a.ksplit * (NTW * 256), a.ksplit * SLAB_BYTES);
    if (wave < NTW) slab_store(rs, ks * SLAB_BYTES + (wave * 64 + lane) * 16, sum);
    if (!splitk_arrive(a.counters + tile, a.ksplit, (unsigned*)smem)) return;
    if (wave < NTW) {  // slices are added in index order (own partial from registers at its index): the result does
      const floatx4 own = sum;  // not depend on which workgroup happened to arrive last
      for (int o = 0; o < a.ksplit; ++o) {
        const floatx4 part = o == ks ? own : slab_load(rs, o * SLAB_BYTES + (wave * 64 + lane) * 16);
        sum = o == 0 ? part : sum + part;
      }
    }
  }
  if (wave >= NTW) return;
  const int m = mb * 16 + n16;
  if (a.silu_mul) {
    floatx4 up;
#pragma unroll
    for (int r = 0; r < 4; ++r) up[r] = __shfl_xor(sum[r], 32);  // lanes q = 0,1 hold gate, their partners q = 2,3 up
    if (m < a.M && q < 2) {
      half4_t o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = silu_mul_f16((half_t)sum[r], (half_t)up[r]);
      *(half4_t*)(a.Y + (size_t)m * (a.N >> 1) + (nb * NTW + wave) * 8 + 4 * q) = o;
    }
    return;
  }
  const int nc = (nb * NTW + wave) * 16 + 4 * q;  // lane holds channels nc..nc+3 of token m
  if (m < a.M) {
    if (a.bias) {
      const half4_t b = *(const half4_t*)(a.bias + nc);
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] += (float)b[r];
    }
    half4_t o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (half_t)sum[r];
    if (a.residual) {  // added to the ROUNDED product, as GEMM-then-add does
      const half4_t b = *(const half4_t*)(a.residual + (size_t)m * a.N + nc);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (half_t)((float)o[r] + (float)b[r]);
    }
    *(half4_t*)(a.Y + (size_t)m * a.N + nc) = o;
  }
}

// PERSISTENT launch (gridDim.x < channel blocks; needs ksplit == 1): a workgroup walks the channel blocks
// blockIdx.x, + gridDim.x, ...  The chunk pipeline runs across block boundaries -- while the last chunk of a block
// is computed and its partials are reduced, the first chunk of the workgroup's next block is already in flight --
// so the HBM stream does not stop for the load-latency / compute / reduce phases of each block, and x is copied to
// LDS once per workgroup instead of once per block.  Consecutive blocks alternate between two reduction buffers,
// which makes one barrier per block enough.
// Only the XLDS variants can be launched persistent.  The fragments-from-L2 variants keep the plain one-block loop: in
// the cross-block form hipcc needs 141 instead of 121 VGPRs for NTW = 1 (one workgroup per CU instead of two: -9 % on
// the Llama-2-70B shapes at M = 16 [r01]).
// (span stamps: written out at the kernel's own two exits -- moving the body into a forceinline device function called between
// two stamps changed hipcc's code for the deferred-zero paths into something that fails the parity tests [r02])
template <int NTW, int WAVES, int GM, bool XLDS, bool DZ, bool LN = false, bool SPAN = false, bool NT = false>
__global__ __launch_bounds__(WAVES * 64) void w4a16_skinny_kernel(const GemmArgs a) {
  if constexpr (SPAN) span_stamp(a.span, 0);
  constexpr bool PERSIST = XLDS;
  static_assert(!LN || (DZ && !XLDS && NTW >= 2), "the register-level RMSNorm lives in the fragment deferred-zero flavour");
  static_assert(WAVES >= NTW, "the final reduction assigns one channel tile per wave");
  constexpr int U = XLDS ? (NTW == 1 ? 4 : 2) : (NTW <= 2 ? 2 : 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nblocks = a.N / (16 * NTW);
  const int nred = (int)gridDim.x < nblocks ? 2 : 1;
  floatx4* red = (floatx4*)smem;  // [nred][WAVES][NTW][64]
  char* xlds = smem + nred * (WAVES * NTW * 64 * sizeof(floatx4));

  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int n16 = lane & 15, q = lane >> 4;
  const int mb = blockIdx.y, ks = blockIdx.z;
  // XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin, and neighbouring channel blocks share the
  // 128-byte lines of their group constants (4 blocks per line of scales, 16 per line of zero points) -- give every XCD
  // a contiguous run of blocks, so that its L2 fetches each of those lines once instead of all eight fetching it.
  const int gx = (int)gridDim.x;
  const int bx = (gx & 7) == 0 ? ((int)blockIdx.x & 7) * (gx >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
  const int KT = a.K >> 7;
  const int wg_begin = ks * a.kt_per_split, wg_end = min(KT, wg_begin + a.kt_per_split);
  const int cnt = wg_end - wg_begin;
  const int kt_begin = wg_begin + cnt * wave / WAVES, kt_end = wg_begin + cnt * (wave + 1) / WAVES;
  const int kt_last = max(kt_end - 1, kt_begin);  // clamp for replayed loads (a wave may own no k-tile at all)

  const SkinnyBufs bufs = skinny_bufs(a, lane);
  const int row = min(mb * 16 + n16, a.M - 1);  // rows >= M replay row M-1; never stored
  const half_t* xp = a.X + (size_t)row * a.K + q * 8;

  floatx4 acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // (block, k-tile) of the chunk being computed / of the chunk being loaded; both wave-uniform
  int nb_cur = bx, kt_cur = kt_begin;
  int nb_nxt = nb_cur, kt_nxt = kt_cur;
  int parity = 0;
  // The load of the next chunk is issued in a block that always issues it: a guarded load would make hipcc's
  // s_waitcnt pass assume the smaller in-flight count and wait for most of the prefetch before the compute.
#define QA_SKINNY_LOAD(c) skinny_load<NTW, GM, U, XLDS, LN, NT>(c, kt_nxt, kt_last, bufs, nb_nxt * NTW, xp, a)
#define QA_SKINNY_ADVANCE(nb, kt)                                                                                  \
  do {                                                                                                             \
    kt += U;                                                                                                       \
    if (kt >= kt_end) {                                                                                            \
      kt = kt_begin;                                                                                               \
      nb += gridDim.x;                                                                                             \
    }                                                                                                              \
  } while (0)
#define QA_SKINNY_COMPUTE(ccomp)                                                                                   \
  if constexpr (DZ && XLDS) skinny_compute_dz<NTW, GM, U>(ccomp, kt_cur, kt_end, xl, tab, acc);                    \
  else if constexpr (!DZ) skinny_compute<NTW, GM, U, XLDS>(ccomp, kt_cur, kt_end, xl, acc);                        \
  if (kt_cur + U >= kt_end) {                                                                                      \
    skinny_finish<NTW, WAVES, DZ>(a, acc, red + parity * (WAVES * NTW * 64), smem, nb_cur, nblocks, mb, ks, lane,  \
                                  wave);                                                                           \
    parity = (nred - 1) - parity;                                                                                  \
  }
#define QA_SKINNY_STEP(cload, ccomp)                                                                               \
  if (nb_nxt >= nblocks) { /* the chunk in hand is this workgroup's last */                                        \
    QA_SKINNY_COMPUTE(ccomp);                                                                                      \
    break;                                                                                                         \
  }                                                                                                                \
  QA_SKINNY_LOAD(cload);                                                                                           \
  __builtin_amdgcn_sched_barrier(0);                                                                               \
  QA_SKINNY_COMPUTE(ccomp);                                                                                        \
  nb_cur = nb_nxt;                                                                                                 \
  kt_cur = kt_nxt;                                                                                                 \
  QA_SKINNY_ADVANCE(nb_nxt, kt_nxt)

  SkinnyChunk<NTW, GM, U, XLDS, LN> cA, cB;
  if constexpr (!PERSIST) {
    const half_t* gp = LN ? a.ln_w + q * 8 : nullptr;
    // one block per workgroup, x fragments straight from L2
    const int cb = bx * NTW;
    // B operand of the sum MFMAs (deferred-zero flavour): column = lane & 15; even columns ones, odd columns b_k
    const u32x4 bc_bits = (lane & 1) ? u32x4{0x64006400u, 0x54005400u, 0x64006400u, 0x54005400u}
                                     : u32x4{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
    const half8_t bconst = __builtin_bit_cast(half8_t, bc_bits);
    // [r05, profiles/r05_skinny_variants.txt -- read before touching this loop]  Behind the GUARDED requests below hipcc's s_waitcnt pass
    // assumes the smaller in-flight count: the ISA waits vmcnt(3..0) in front of the first MFMAs of the chunk in hand, i.e. the chunk just
    // requested is drained too.  Issuing them unconditionally (replays past the wave's range) gives counted waits (vmcnt(15..12)) and
    // 3-7 % at 6..16 tokens -- and WRONG results in the four-tile instantiation (tile 0 of every block), as did an eight-tile
    // instantiation of this guarded form (tile 2, varying from run to run; 62 -> 54 us at 16 x 8192 x 57344, its x fragments being half
    // the weights' bytes instead of as many).  Both are cured by -mllvm -amdgpu-waitcnt-forcezero: the wait counts hipcc derives for
    // requests whose results die on the loop's way out cannot be trusted here.  Neither is shipped; the instantiations that are have
    // been through the parity suite in this exact form since r01.
    if (kt_begin < kt_end) skinny_load<NTW, GM, U, XLDS, LN, NT>(cA, kt_begin, kt_end - 1, bufs, cb, xp, a, gp);
    __builtin_amdgcn_sched_barrier(0);
    // LN: 1 / rms of every row before the first chunk is computed -- the first chunk's weights (and x, norm weight fragments) are
    // already on their way: each wave sums the squares of its k tiles of the rows (the fragments the loop reads, lane = row n16;
    // two tiles' requests in flight at a time), the sums meet in LDS behind the reduction buffer, one barrier
    float rstd = 0.f;
    if constexpr (LN) {
      float ss = 0.f;
#pragma unroll 2
      for (int kt = kt_begin; kt < kt_end; ++kt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const u32x4 v = *(const u32x4*)(xp + kt * 128 + 32 * t);
#pragma unroll
          for (int d = 0; d < 4; ++d) ss = __builtin_amdgcn_fdot2(as_h2(v[d]), as_h2(v[d]), ss, false);
        }
      }
      ss += __shfl_xor(ss, 16);
      ss += __shfl_xor(ss, 32);
      float* ssq_lds = (float*)(red + WAVES * NTW * 64);
      if (q == 0) ssq_lds[wave * 16 + n16] = ss;
      __syncthreads();
      float st = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) st += ssq_lds[w * 16 + n16];
      rstd = rsqrtf(st / (float)a.K + a.ln_eps);
    }
#ifdef QA_EXP_SKINNY_UNCOND   // (A/B builds only: the unconditional requests of profiles/r05_skinny_variants.txt -- wrong results in the four-tile build)
#define QA_SKINNY_IF(c)
#else
#define QA_SKINNY_IF(c) if (c)
#endif
#ifndef QA_EXP_SKINNY_WAIT
#define QA_EXP_SKINNY_WAIT 0   // (A/B builds: full waits at chosen points of the loop, to bisect which request the ISA's own waits do not cover)
#endif
#define QA_SKINNY_FULLWAIT(bit) do { if constexpr ((QA_EXP_SKINNY_WAIT >> (bit)) & 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); } while (0)
    QA_SKINNY_FULLWAIT(2);
    for (int kt = kt_begin; kt < kt_end; kt += 2 * U) {
      QA_SKINNY_IF(kt + U < kt_end) skinny_load<NTW, GM, U, XLDS, LN, NT>(cB, kt + U, kt_end - 1, bufs, cb, xp, a, gp);
      __builtin_amdgcn_sched_barrier(0);
      QA_SKINNY_FULLWAIT(0);
      if constexpr (DZ) skinny_compute_dzf<NTW, GM, U, LN>(cA, kt, kt_end, bconst, (lane & 1) != 0, acc, rstd);
      else skinny_compute<NTW, GM, U, XLDS>(cA, kt, kt_end, nullptr, acc);
      if (kt + U >= kt_end) break;
      QA_SKINNY_IF(kt + 2 * U < kt_end) skinny_load<NTW, GM, U, XLDS, LN, NT>(cA, kt + 2 * U, kt_end - 1, bufs, cb, xp, a, gp);
      __builtin_amdgcn_sched_barrier(0);
      QA_SKINNY_FULLWAIT(1);
      if constexpr (DZ) skinny_compute_dzf<NTW, GM, U, LN>(cB, kt + U, kt_end, bconst, (lane & 1) != 0, acc, rstd);
      else skinny_compute<NTW, GM, U, XLDS>(cB, kt + U, kt_end, nullptr, acc);
    }
    QA_SKINNY_FULLWAIT(3);
    skinny_finish<NTW, WAVES, DZ>(a, acc, red, smem, bx, nblocks, mb, ks, lane, wave);
    if constexpr (SPAN) span_stamp(a.span, 1);
    return;
  }
  QA_SKINNY_LOAD(cA);  // HBM requests first
  QA_SKINNY_ADVANCE(nb_nxt, kt_nxt);
  __builtin_amdgcn_sched_barrier(0);

  const char* xl = nullptr;
  const float* tab = nullptr;
  if constexpr (XLDS) {
    // copy x[mb*16 .. , wg_begin*128 .. wg_end*128) -> LDS [rows][pitch]; DZ: tabulate the unit sums on the way
    const int rows = min(16, a.M - mb * 16);
    const int kc = cnt * 16;  // 16-byte chunks per row
    const int pitch = cnt * 256 + 16;
    xl = xlds + min(n16, rows - 1) * pitch + q * 16 - wg_begin * 256;
    float* tab0 = (float*)(xlds + rows * pitch);
    constexpr int NG = groups_per_tile<GM>();
    constexpr int L = 16 / NG;  // lanes (16-byte chunks) per unit
    if constexpr (DZ) tab = tab0 + 4 * q - wg_begin * NG * 32;
    if constexpr (DZ) {
      if (a.ln_w) {
        // RMSNorm prologue (needs the whole row: ksplit == 1).  Pass 1 copies x raw and sums its squares per row;
        // pass 2, below, finds x in LDS instead of in global memory, scales it in place and tabulates the result.
        float* ssq = (float*)smem;  // [rows][WAVES], in the still unused reduction buffer
        for (int r = 0; r < rows; ++r) {
          const half_t* src = a.X + (size_t)(mb * 16 + r) * a.K;
          float ss = 0.f;
          for (int c = threadIdx.x; c < kc; c += WAVES * 64) {
            const u32x4 v = *(const u32x4*)(src + c * 8);
            *(u32x4*)(xlds + r * pitch + c * 16) = v;
#pragma unroll
            for (int i = 0; i < 4; ++i) ss = __builtin_amdgcn_fdot2(as_h2(v[i]), as_h2(v[i]), ss, false);
          }
          ss = wave_sum(ss);
          if (lane == 0) ssq[r * WAVES + wave] = ss;
        }
        __syncthreads();
      }
    }
    // Rows in batches of RB: the loads of a batch are all issued before the first of them is used.  One row at a time this loop was a
    // chain of `rows` round trips to L2 (load -> LDS store -> unit sums -> table), 1.2-1.5 us of an 8-token launch [r02 stamps]; the
    // deferred-zero table flavour lost to the exact path at 3..16 tokens for that reason alone.
    constexpr int RB = 4;
    for (int r0 = 0; r0 < rows; r0 += RB) {
      float inv[RB];
#pragma unroll
      for (int j = 0; j < RB; ++j) inv[j] = 0.f;
      if constexpr (DZ) {
        if (a.ln_w) {
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            const int r = min(r0 + j, rows - 1);
            float ss = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) ss += ((const float*)smem)[r * WAVES + w];
            inv[j] = rsqrtf(ss / (float)a.K + a.ln_eps);
          }
        }
      }
      for (int c = threadIdx.x; c < kc; c += WAVES * 64) {  // kc % 16 == 0: rows of 16 lanes are all in or all out
        u32x4 v[RB];
        bool normed = false;
        if constexpr (DZ) {
          if (a.ln_w) {  // fp16(fp16(x * inv) * weight): the rounding points of quick_rmsnorm_f16 (and of torch)
            normed = true;
            const half8_t gv = *(const half8_t*)(a.ln_w + c * 8);
#pragma unroll
            for (int j = 0; j < RB; ++j) {
              const half8_t xv = *(const half8_t*)(xlds + min(r0 + j, rows - 1) * pitch + c * 16);
              half8_t o;
#pragma unroll
              for (int i = 0; i < 8; ++i) o[i] = (half_t)((half_t)((float)xv[i] * inv[j]) * gv[i]);
              v[j] = __builtin_bit_cast(u32x4, o);
            }
          }
        }
        if (!normed) {
#pragma unroll
          for (int j = 0; j < RB; ++j)  // (past the last row: a replay of it, not stored)
            v[j] = *(const u32x4*)(a.X + (size_t)(mb * 16 + min(r0 + j, rows - 1)) * a.K + wg_begin * 128 + c * 8);
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const int r = r0 + j;
          if (r < rows) {  // workgroup-uniform
            *(u32x4*)(xlds + r * pitch + c * 16) = v[j];
            if constexpr (DZ) {
              const half2_t one2 = {(half_t)1.f, (half_t)1.f};
              const float lo = __builtin_amdgcn_fdot2(as_h2(v[j][0]), one2, __builtin_amdgcn_fdot2(as_h2(v[j][2]), one2, 0.f, false), false);
              const float hi = __builtin_amdgcn_fdot2(as_h2(v[j][1]), one2, __builtin_amdgcn_fdot2(as_h2(v[j][3]), one2, 0.f, false), false);
              const float sa = lanes_sum<L>(lo + hi);
              const float sc = lanes_sum<L>(1024.f * lo + 64.f * hi);
              if ((lane & (L - 1)) == 0) {
                float* t = tab0 + (c / L) * 32 + r;
                t[0] = sa;
                t[16] = -sc;
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }

  while (true) {
    QA_SKINNY_STEP(cB, cA);
    QA_SKINNY_STEP(cA, cB);
  }
  if constexpr (SPAN) span_stamp(a.span, 1);
#undef QA_SKINNY_STEP
#undef QA_SKINNY_COMPUTE
#undef QA_SKINNY_ADVANCE
#undef QA_SKINNY_LOAD
}

// ------------------------------------------------------------------------------------------------
// tiled kernel
// ------------------------------------------------------------------------------------------------
// per-wave state of the tiled kernel that does not change over the K loop
template <int BMT, int TN, int WK, int WN = 4>
struct TiledCtx {
  static constexpr int XPW = 4 * BMT / WN;  // x fragments staged per wave per stage (4*WK*BMT fragments, WN*WK waves)
  const u32x4* wp[TN];      // this lane's 16 bytes of weight tile (channel tile j, k-tile 0)
  int ncol[TN];             // this lane's output channel in channel tile j
  const half_t* xsrc[XPW];  // global source of the fragments this wave stages (k-tile 0 of a stage)
  int xkt[XPW];             // which of the stage's WK k-tiles fragment i belongs to
  int kt_lo, kt_hi, wave, wk;
};

// x fragments of stage s: global -> registers (ordinary loads: hipcc counts them, so they can stay in flight
// across barriers; global_load_lds cannot -- the compiler drains it at every barrier and at the first use of any
// other load)
template <int BMT, int TN, int WK, int WN>
__device__ __forceinline__ void tiled_load_x(const TiledCtx<BMT, TN, WK, WN>& c, int s, u32x4 (&xr)[4 * BMT / WN]) {
#pragma unroll
  for (int i = 0; i < 4 * BMT / WN; ++i) {
    const int kt = min(c.kt_lo + WK * s + c.xkt[i], c.kt_hi - 1);  // past the end: replay the last tile (unused)
    xr[i] = *(const u32x4*)(c.xsrc[i] + kt * 128);
  }
}
// registers -> LDS in B-fragment order: fragment f = wave*BMT + i is 1 KiB, lane l at byte 16 l
template <int BMT, int TN, int WK, int WN>
__device__ __forceinline__ void tiled_store_x(const TiledCtx<BMT, TN, WK, WN>& c, char* buf, int lane,
                                              const u32x4 (&xr)[4 * BMT / WN]) {
  constexpr int XPW = 4 * BMT / WN;
#pragma unroll
  for (int i = 0; i < XPW; ++i) *(u32x4*)(buf + (c.wave * XPW + i) * 1024 + lane * 16) = xr[i];
}

// weights + raw group constants of this wave's k-tile of stage s (no dependent ALU: see GroupRaw)
template <int BMT, int TN, int WK, int GM, int WN>
__device__ __forceinline__ void tiled_load_w(const TiledCtx<BMT, TN, WK, WN>& c, const GemmArgs& a, int s, u32x4 (&w)[TN],
                                             uint32_t (&gs)[TN][groups_per_tile<GM>()]) {
  constexpr int NG = groups_per_tile<GM>();
  const int kt = min(c.kt_lo + WK * s + c.wk, c.kt_hi - 1);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    w[j] = c.wp[j][(size_t)kt * 64];
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int g = group_index<GM>(kt, i * (4 / NG), a.tpg, a.G);
      const GroupRaw r = load_group_raw(a.S, a.QZ, g, c.ncol[j], a.N, a.K / a.G);
      gs[j][i] = r.sz;  // (the zero point travels in the same word)
    }
  }
}

// ABL (ablation bits, timing experiments only -- results are wrong when set): 1 = no global loads in the K loop,
// 2 = no LDS traffic in the K loop, 4 = no dequantisation, 8 = no barrier.
template <int BMT, int TN, int WK, int GM, int ABL, int WN>
__device__ __forceinline__ void tiled_compute(const TiledCtx<BMT, TN, WK, WN>& c, const char* sb, int s, const u32x4 (&w)[TN],
                                              const uint32_t (&gs)[TN][groups_per_tile<GM>()],
                                              floatx4 (&acc)[TN][BMT]) {
  constexpr int NG = groups_per_tile<GM>();
  if (c.kt_lo + WK * s + c.wk >= c.kt_hi) {  // wave-uniform: a ragged last stage has no tile for this wave
#pragma unroll
    for (int j = 0; j < TN; ++j) {  // "use" the loads so that both paths leave the same ones pending (see the K loop)
      asm volatile("" ::"v"(w[j]));
#pragma unroll
      for (int i = 0; i < NG; ++i) asm volatile("" ::"v"(gs[j][i]));
    }
    return;
  }
  GroupQ grp[TN][NG];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < NG; ++i) grp[j][i] = make_group(GroupRaw{gs[j][i]});
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    half8_t bf[BMT];
#pragma unroll
    for (int mt = 0; mt < BMT; ++mt) {
      if constexpr (ABL & 2) bf[mt] = __builtin_bit_cast(half8_t, w[0]);
      else bf[mt] = *(const half8_t*)(sb + (t * BMT + mt) * 1024);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      half8_t af;
      if constexpr (ABL & 4) af = __builtin_bit_cast(half8_t, w[j]);
      else af = dequant8(w[j][t], grp[j][group_slot<GM>(t)]);
#pragma unroll
      for (int mt = 0; mt < BMT; ++mt) acc[j][mt] = mfma16(af, bf[mt], acc[j][mt]);
    }
  }
}

// Tiled kernel.  Workgroup tile (BMT*16 tokens) x (4*TN*16 channels); 4*WK waves = 4 along N x WK along K.
// One stage = WK*128 k: wave (wn, wk) owns channel tiles wn*TN..+TN-1 and the wk-th 128-k weight tile of every
// stage, so no weight is dequantised twice inside a workgroup and every LDS fragment is read by 4 waves only.  The
// token tile of a stage lives in LDS *in B-fragment order* (lane l of fragment (kt, t, mt) holds
// x[mt*16 + l%16][kt*128 + 32t + 8*(l/16) ..+7]), so every ds_read_b128 / ds_write_b128 is lane-linear and
// conflict free.  The WK partial sums are added through LDS in the epilogue.
//
// Software pipeline (2 LDS buffers, 2 weight register sets, 1 x register set; loop unrolled by 2 so that every
// slot index is static):  iteration s  =  { x(s+1): regs -> LDS[other] ; issue x(s+2) loads ; compute stage s from
// LDS[cur] with weights[s%2] ; issue weights(s+2) into the set just freed ; barrier }.
// Loads past the last stage are NOT guarded: they replay the last tile (clamped index) and are never consumed -- a
// guard would merge "issued" and "not issued" paths and make hipcc drain the whole load queue at every consumer.
// For the same reason the unrolled pair has no early exit: with an odd stage count the second half replays a stage
// (stores it, skips its compute) -- an `if (s >= nstage) break` gives the waitcnt pass a path from one half-iteration
// straight into the same half again, on which the weights just requested look like the ones about to be used.
template <int BMT, int TN, int WK, int GM, int ABL = 0, int WN = 4>
__global__ __launch_bounds__(64 * WN * WK) void w4a16_tiled_kernel(const GemmArgs a) {
  constexpr int XPW = 4 * BMT / WN;
  constexpr int NG = groups_per_tile<GM>();
  constexpr int FRAGS = 4 * WK * BMT;        // 1 KiB fragments per stage
  constexpr int STAGE_BYTES = FRAGS * 1024;  // 32 KiB at BMT = 4, WK = 2
  static_assert((WK - 1) * WN * TN * BMT * 1024 <= 2 * STAGE_BYTES, "epilogue exchange must fit in the stage buffers");
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 * STAGE_BYTES

  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int wn = wave % WN, wk = wave / WN;
  const int n16 = lane & 15, q = lane >> 4;
  const int NB = a.N / (16 * WN * TN);
  int nb = blockIdx.x % NB, mb = blockIdx.x / NB;
  if (a.xcd_gm > 0) {
    // Workgroup b runs on XCD b % 8 (observed dispatch order; only speed depends on it).  Give every XCD a compact
    // rectangle of tiles so that its private L2 fetches few distinct x rows AND few distinct weight columns.
    const int MB = gridDim.x / NB, gn = 8 / a.xcd_gm;
    const int mcnt = MB / a.xcd_gm, ncnt = NB / gn;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    mb = (xcd / gn) * mcnt + idx / ncnt;
    nb = (xcd % gn) * ncnt + idx % ncnt;
  }
  const int ks = blockIdx.y;
  const int KT = a.K >> 7;
  TiledCtx<BMT, TN, WK, WN> c;
  c.kt_lo = ks * a.kt_per_split;
  c.kt_hi = min(KT, c.kt_lo + a.kt_per_split);
  c.wave = wave;
  c.wk = wk;
  const int nstage = (c.kt_hi - c.kt_lo + WK - 1) / WK;
  const int m0 = mb * BMT * 16;
  const int nt0 = (nb * WN + wn) * TN;  // first 16-channel tile of this wave

#pragma unroll
  for (int j = 0; j < TN; ++j) {
    c.wp[j] = a.QW + (size_t)(nt0 + j) * KT * 64 + lane;
    c.ncol[j] = (nt0 + j) * 16 + n16;
  }
  // fragments this wave stages: f = wave*BMT + i  ->  (k-tile f / (4 BMT), k-step (f / BMT) % 4, token tile f % BMT)
#pragma unroll
  for (int i = 0; i < XPW; ++i) {
    const int f = wave * XPW + i, t = (f / BMT) & 3, mt = f % BMT;
    c.xkt[i] = f / (4 * BMT);
    const int row = min(m0 + mt * 16 + n16, a.M - 1);
    c.xsrc[i] = a.X + (size_t)row * a.K + 32 * t + 8 * q;
  }

  floatx4 acc[TN][BMT];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int mt = 0; mt < BMT; ++mt) acc[j][mt] = floatx4{0.f, 0.f, 0.f, 0.f};

  unsigned long long t_entry = 0, r_entry = 0;
  if constexpr (ABL & 16) {
    t_entry = __builtin_amdgcn_s_memtime();
    r_entry = __builtin_amdgcn_s_memrealtime();
  }
  u32x4 xr[XPW];
  u32x4 w[2][TN];
  uint32_t gs[2][TN][NG];
  const int rd = wk * (4 * BMT * 1024) + lane * 16;  // this wave reads its k-tile's part of a stage

  if (nstage > 0) {
    // Issue order = the K loop's steady state (x(s+1) then w(s+1) in flight at the top of iteration s), and pinned:
    // hipcc's waitcnt pass merges the prologue's view of "which loads are still in flight" into every iteration, so a
    // prologue that ends on x loads (or lets the scheduler sink a scale load below them) turns the loop's
    // s_waitcnt vmcnt(7..4) into vmcnt(3..0) -- a full drain of the weight prefetch once per stage [r01: -4 %].
    tiled_load_x<BMT, TN, WK, WN>(c, 0, xr);
    __builtin_amdgcn_sched_barrier(0);
    tiled_load_w<BMT, TN, WK, GM, WN>(c, a, 0, w[0], gs[0]);
    __builtin_amdgcn_sched_barrier(0);
    tiled_store_x<BMT, TN, WK, WN>(c, smem, lane, xr);
    __builtin_amdgcn_sched_barrier(0);
    tiled_load_x<BMT, TN, WK, WN>(c, 1, xr);
    __builtin_amdgcn_sched_barrier(0);
    tiled_load_w<BMT, TN, WK, GM, WN>(c, a, 1, w[1], gs[1]);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();

  // ABL bit 16: s_memtime stamps between the phases of every iteration, summed per wave (perturbs the schedule a bit)
  unsigned long long ph[5] = {0, 0, 0, 0, 0};
  unsigned long long t_prev = 0;
#define QA_STAMP(i)                                              \
  if constexpr (ABL & 16) {                                      \
    const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
    ph[i] += t_now - t_prev;                                     \
    t_prev = t_now;                                              \
  }
  if constexpr (ABL & 16) t_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long t_loop = t_prev;
  for (int s0 = 0; s0 < nstage; s0 += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int s = s0 + u;  // (s == nstage for odd nstage: a replayed stage whose compute is skipped)
      char* const cur = smem + u * STAGE_BYTES;
      char* const nxt = smem + (u ^ 1) * STAGE_BYTES;
      if constexpr (!(ABL & 2)) tiled_store_x<BMT, TN, WK, WN>(c, nxt, lane, xr);  // stage s+1 (a replay at the very end)
      QA_STAMP(0)
      if constexpr (!(ABL & 1)) tiled_load_x<BMT, TN, WK, WN>(c, s + 2, xr);
      QA_STAMP(1)
      tiled_compute<BMT, TN, WK, GM, ABL, WN>(c, cur + rd, s, w[u], gs[u], acc);
      QA_STAMP(2)
      if constexpr (!(ABL & 1)) tiled_load_w<BMT, TN, WK, GM, WN>(c, a, s + 2, w[u], gs[u]);
      QA_STAMP(3)
      if constexpr (!(ABL & 8)) __syncthreads();
      QA_STAMP(4)
    }
  }
  if constexpr (ABL & 16) {
    if (lane == 0 && a.dbg) {
      unsigned long long* o = a.dbg + ((size_t)blockIdx.x * (WN * WK) + wave) * 8;
#pragma unroll
      for (int i = 0; i < 5; ++i) o[i] = ph[i];
      o[5] = (unsigned long long)nstage | (r_entry << 8);  // (+ when the wave started, 100 MHz ticks)
      o[6] = t_loop - t_entry;  // prologue (first loads) in shader cycles
      // shader cycles and 100 MHz ticks from entry to the end of the K loop: the clock the kernel actually ran at
      o[7] = ((__builtin_amdgcn_s_memtime() - t_entry) << 24) | ((__builtin_amdgcn_s_memrealtime() - r_entry) & 0xffffff);
    }
  }
#undef QA_STAMP

  // add the WK partial sums through LDS (the stage buffers are free after the last barrier)
  floatx4* ex = (floatx4*)smem;  // [wk-1][wn][j][mt][lane]
  if (wk > 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int mt = 0; mt < BMT; ++mt) ex[((((wk - 1) * WN + wn) * TN + j) * BMT + mt) * 64 + lane] = acc[j][mt];
  }
  __syncthreads();
  if (wk == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int mt = 0; mt < BMT; ++mt)
#pragma unroll
        for (int k = 1; k < WK; ++k) acc[j][mt] += ex[((((k - 1) * WN + wn) * TN + j) * BMT + mt) * 64 + lane];
  }
  if (a.ksplit > 1) {
    constexpr unsigned SLAB_BYTES = WN * TN * BMT * 1024;  // one fp32 partial tile
    const __amdgpu_buffer_rsrc_t rs =
        slab_rsrc(a.slabs + (size_t)blockIdx.x * a.ksplit * (SLAB_BYTES / 4), a.ksplit * SLAB_BYTES);
    const unsigned my = ((wn * TN) * BMT * 64 + lane) * 16;
    if (wk == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int mt = 0; mt < BMT; ++mt) slab_store(rs, ks * SLAB_BYTES + my + (j * BMT + mt) * 1024, acc[j][mt]);
    }
    if (!splitk_arrive(a.counters + blockIdx.x, a.ksplit, (unsigned*)smem)) return;
    if (wk == 0) {  // slices are added in index order (own partial from registers at its index): the result does not
      floatx4 own[TN][BMT];  // depend on which workgroup happened to arrive last
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int mt = 0; mt < BMT; ++mt) own[j][mt] = acc[j][mt];
      for (int o = 0; o < a.ksplit; ++o) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int mt = 0; mt < BMT; ++mt) {
            const floatx4 part = o == ks ? own[j][mt] : slab_load(rs, o * SLAB_BYTES + my + (j * BMT + mt) * 1024);
            acc[j][mt] = o == 0 ? part : acc[j][mt] + part;
          }
      }
    }
  }
  if (a.silu_mul) {
    if (wk == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int mt = 0; mt < BMT; ++mt) {
          floatx4 up;
#pragma unroll
          for (int r = 0; r < 4; ++r) up[r] = __shfl_xor(acc[j][mt][r], 32);
          const int m = m0 + mt * 16 + n16;
          if (m < a.M && q < 2) {
            half4_t o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = silu_mul_f16((half_t)acc[j][mt][r], (half_t)up[r]);
            *(half4_t*)(a.Y + (size_t)m * (a.N >> 1) + (nt0 + j) * 8 + 4 * q) = o;
          }
        }
    }
    return;
  }
  if (wk == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nc = (nt0 + j) * 16 + 4 * q;
      half4_t b = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
      if (a.bias) b = *(const half4_t*)(a.bias + nc);
#pragma unroll
      for (int mt = 0; mt < BMT; ++mt) {
        const int m = m0 + mt * 16 + n16;
        if (m < a.M) {
          half4_t o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (half_t)(acc[j][mt][r] + (float)b[r]);
          if (a.residual) {  // added to the ROUNDED product, as GEMM-then-add does
            const half4_t res = *(const half4_t*)(a.residual + (size_t)m * a.N + nc);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (half_t)((float)o[r] + (float)res[r]);
          }
          *(half4_t*)(a.Y + (size_t)m * a.N + nc) = o;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// tiled kernel, 32x32x16 MFMA flavour.  Same workgroup tile, wave grid, LDS double buffer and pipeline as above,
// but the matrix instruction is v_mfma_f32_32x32x16_f16: 32 cycles per instruction instead of 16, which -- unlike
// the 16-cycle 16x16x32 -- leaves the SIMD free to issue ~4 VALU ops per MFMA (tools/mfma_valu_overlap.hip), so
// part of the dequantisation hides under the matrix pipe inside ONE wave.
//   A operand (32 channels x 16 k; lane l: channel l%32, k-half l/32): built from the raw packed dwords of TWO
//     16-channel tiles -- whose lanes are (channel%16, k-octet l/16) -- with v_permlane16_swap + v_permlane32_swap:
//     [r0.q0 r1.q0 | r0.q1 r1.q1] feeds the first k16 step of a k32 step, [r0.q2 r1.q2 | r0.q3 r1.q3] the second.
//     The weight layout in HBM is unchanged.
//   B operand (16 k x 32 tokens; lane l: token l%32, k-half l/32): the LDS image of a stage is
//     [k-tile][k16 step 0..7][32-token tile][64 lanes x 16 B]; the staging loads keep the 16-row x 64-byte shape and
//     each lane writes its 16 bytes to the slot the 32-wide fragment wants.
//   C/D: lane l holds token l%32 and channels (r%4) + 8*(r/4) + 4*(l/32), r = 0..15, of the 32-channel pair.
// ------------------------------------------------------------------------------------------------
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));


// empty kernel with the GEMM's launch shape: what the dispatch-duration clock reads with no work at all
__global__ __launch_bounds__(512) void w4a16_empty_kernel(unsigned* sink) {
  if (sink != nullptr && threadIdx.x == 0xffffffffu) sink[0] = 1;
}

// ------------------------------------------------------------------------------------------------
// workspace check: the counter region and the exchange zone must be all-zero between launches (include/quick_amd.h, "workspace").
// One pass over them; the lowest dirty byte offset lands in *first (0xffffffff = clean).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void w4a16_workspace_scan_kernel(const u32x4* __restrict__ ws, unsigned n16, unsigned* __restrict__ first) {
  unsigned lo = 0xffffffffu;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) {
    const u32x4 v = __builtin_nontemporal_load(ws + i);
    if ((v[0] | v[1] | v[2] | v[3]) != 0u) lo = min(lo, i * 16u);
  }
  if (lo != 0xffffffffu) atomicMin(first, lo);
}

// ------------------------------------------------------------------------------------------------
// dense dequantisation (debug / parity aid): W[k, n] = fp16((w - z) * s), row-major [K, N]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void w4a16_dequant_kernel(const u32x4* __restrict__ QW, const half_t* __restrict__ S,
                                                           const uint32_t* __restrict__ QZ, half_t* __restrict__ W,
                                                           int K, int N, int G) {
  const int lane = threadIdx.x, n16 = lane & 15, q = lane >> 4;
  const int nt = blockIdx.x, kt = blockIdx.y, KT = K >> 7;
  const int n = nt * 16 + n16;
  const u32x4 w = QW[((size_t)nt * KT + kt) * 64 + lane];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k0 = kt * 128 + 32 * t + 8 * q;
    const GroupQ g = make_group(load_group_raw(S, QZ, k0 / G, n, N, K / G));
    const half8_t af = dequant8(w[t], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) W[(size_t)(k0 + j) * N + n] = af[j];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int quick_w4a16_workspace_check(const void* workspace, size_t workspace_bytes, void* hip_stream);
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// Where the main kernel goes: the stream, plus an optional event pair bound to that one dispatch
// (hipExtLaunchKernelGGL) so that a profiler-free caller can read the kernel's own duration.
struct Launch {
  hipStream_t st;
  hipEvent_t start, stop;
  unsigned long long* span = nullptr;  // device [2]: in-kernel span of this launch (see span_stamp)
};

static int check_shapes(int M, int K, int N, int G) {
  if (M <= 0 || K <= 0 || N <= 0 || G <= 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "non-positive dimension");
  // same messages as csrc/gemm_cuda_quick.cu:1479-1484
  if (N % 128 != 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "OC is not multiple of cta_N = 128");
  if (N % 8 != 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "OC is not multiple of pack_num = 8");
  if (G % 32 != 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "Group size should be a multiple of 32");
  if (K % G != 0) return fail(QUICK_ERR_UNSUPPORTED, "in_features (%d) is not a multiple of the group size (%d)", K, G);
  if (K % 128 != 0) return fail(QUICK_ERR_UNSUPPORTED, "in_features (%d) must be a multiple of 128 on MI355X", K);
  return QUICK_OK;
}

static thread_local bool g_span_unsupported = false;  // set by a launcher asked for span stamps its kernel does not carry

// [r05] EIGHT channel tiles per workgroup in the fragment deferred-zero flavour, as STRAIGHT-LINE code: 9..16 tokens on layers whose x (16 x K
// fp16) does not fit LDS (K >= 8192: Llama-2-70B).  Why eight: the launch time of this flavour follows the bytes of its x fragments, which come from L2 once per workgroup and k tile
// (64 B per token row and request: 16 cache lines per instruction) -- as many bytes as the weights at four tiles, half as many at eight (16 x 8192 x
// 57344: 62 -> 50 us); queue depth and occupancy do not move it (profiles/r05_skinny_variants.txt).  Why straight-line: the chunk loop of w4a16_skinny_kernel instantiated for eight tiles gave wrong
// results that -amdgpu-waitcnt-forcezero cured (hipcc's wait counts around guarded / replayed requests in a loop).  Here
// every wave owns EXACTLY T k tiles (the planner only picks the kernel when K / 128 == 8 waves x ksplit x T), every request is unconditional,
// nothing is replayed and no request's result dies unread: the form in which hipcc's counts are exact (as in the lean kernels).
// [r06, late] NTW = 7: the same kernel with SEVEN channel tiles per workgroup, for layers whose block count makes whole rounds that way -- 16 x 8192 x 57344 (Llama-2-70B
// gate_up: 57344 = 7 x 8192) is 448 blocks of 128 channels = 1.75 rounds of one workgroup per CU (212 registers), but 512 blocks of 112 = two whole rounds.
template <int T, bool NT, bool SPAN = false, int NTW_ = 8>
__global__ __launch_bounds__(512) void w4a16_frag8_kernel(const GemmArgs a) {
  if constexpr (SPAN) span_stamp(a.span, 0);
  constexpr int NTW = NTW_, WAVES = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  floatx4* red = (floatx4*)smem;  // [WAVES][NTW][64]
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int n16 = lane & 15, q = lane >> 4;
  const int mb = blockIdx.y, ks = blockIdx.z;
  const int nblocks = a.N / (16 * NTW);
  const int gx = (int)gridDim.x;
  const int bx = (gx & 7) == 0 ? ((int)blockIdx.x & 7) * (gx >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x;   // XCD-aware block order (skinny kernel)
  const int kt_begin = (ks * WAVES + wave) * T;   // a.kt_per_split == WAVES * T
  const SkinnyBufs bufs = skinny_bufs(a, lane);
  const int row = min(mb * 16 + n16, a.M - 1);  // rows >= M replay row M-1; never stored
  const half_t* xp = a.X + (size_t)row * a.K + q * 8;
  floatx4 acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const u32x4 bc_bits = (lane & 1) ? u32x4{0x64006400u, 0x54005400u, 0x64006400u, 0x54005400u}
                                   : u32x4{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
  const half8_t bconst = __builtin_bit_cast(half8_t, bc_bits);
  const int cb = bx * NTW;
  const int kt_far = a.K >> 7;   // (no clamp ever bites: every k tile asked for is this wave's own)
  SkinnyChunk<NTW, 0, 1, false, false> c[2];
  skinny_load<NTW, 0, 1, false, false, NT>(c[0], kt_begin, kt_far, bufs, cb, xp, a);
#pragma unroll
  for (int i = 0; i < T; ++i) {
    if (i + 1 < T) skinny_load<NTW, 0, 1, false, false, NT>(c[(i + 1) & 1], kt_begin + i + 1, kt_far, bufs, cb, xp, a);   // (compile-time condition)
    __builtin_amdgcn_sched_barrier(0);
    skinny_compute_dzf<NTW, 0, 1, false>(c[i & 1], 0, 1, bconst, (lane & 1) != 0, acc);   // (kt = 0 < kt_end = 1: the k tile is always this wave's)
  }
  skinny_finish<NTW, WAVES, true>(a, acc, red, smem, bx, nblocks, mb, ks, lane, wave);
  if constexpr (SPAN) span_stamp(a.span, 1);
}


template <int NTW, int WAVES, bool XLDS, bool DZ, bool LN = false>
static void launch_skinny_gm(const Plan& p, const GemmArgs& a, const Launch& L) {
  dim3 grid(p.grid_x, (a.M + 15) / 16, p.ksplit), block(WAVES * 64);
  const size_t lds = skinny_lds_bytes(a.M, a.G, NTW, WAVES, p.kt_per_split, p.grid_x < a.N / (16 * NTW), XLDS, DZ) + (LN ? 1024 : 0);
  if (a.span) {  // in-kernel span stamps: separate instantiations, for the small-M kernels the BASELINE sweep and the decode shapes run
    constexpr bool stamped = !LN && ((WAVES == 8 && ((NTW == 1 && XLDS && DZ) || (NTW == 1 && !XLDS && !DZ) || (NTW == 4 && !XLDS && DZ))) ||
                                     (WAVES == 16 && NTW == 1 && ((XLDS && DZ) || (!XLDS && !DZ))));
    if constexpr (stamped) {
      if (group_mode(a.G) == 0) {   // [r06, ADVICE r05] the stamped build of the kernel the product runs: nt weight requests with one token block
        auto kfn = w4a16_skinny_kernel<NTW, WAVES, 0, XLDS, DZ, LN, true>;
        auto kfn_nt = w4a16_skinny_kernel<NTW, WAVES, 0, XLDS, DZ, LN, true, true>;
        (void)hipFuncSetAttribute((const void*)(a.M <= 16 ? kfn_nt : kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu);
        if (a.M <= 16) hipExtLaunchKernelGGL(kfn_nt, grid, block, (unsigned)lds, L.st, L.start, L.stop, 0, a);
        else hipExtLaunchKernelGGL(kfn, grid, block, (unsigned)lds, L.st, L.start, L.stop, 0, a);
        return;
      }
    }
    g_span_unsupported = true;
    return;
  }
  if (a.M <= 16 && group_mode(a.G) == 0) {  // one token block: weights streamed once -> nt requests (see skinny_load)
    auto kfn = w4a16_skinny_kernel<NTW, WAVES, 0, XLDS, DZ, LN, false, true>;
    static std::atomic<unsigned long long> attr_set_nt{0};
    (void)lds_limit_once(attr_set_nt, (const void*)kfn, (int)kLdsPerCu);
    hipExtLaunchKernelGGL(kfn, grid, block, (unsigned)lds, L.st, L.start, L.stop, 0, a);
    return;
  }
#define QA_SKINNY(GMV)                                                                                             \
  do {                                                                                                             \
    auto kfn = w4a16_skinny_kernel<NTW, WAVES, GMV, XLDS, DZ, LN>;                                                 \
    static std::atomic<unsigned long long> attr_set{0};                                                                \
    (void)lds_limit_once(attr_set, (const void*)kfn, (int)kLdsPerCu);                                              \
    hipExtLaunchKernelGGL(kfn, grid, block, (unsigned)lds, L.st, L.start, L.stop, 0, a);                           \
  } while (0)
  if constexpr (LN) {  // only reached with G % 128 == 0
    if (group_mode(a.G) == 0) QA_SKINNY(0);
    else QA_SKINNY(1);
  } else {
    switch (group_mode(a.G)) {
      case 0: QA_SKINNY(0); break;
      case 1: QA_SKINNY(1); break;
      case 2: QA_SKINNY(2); break;
      // (sixteen waves of the table flavour with > 2 units per k tile: no build -- it spilled; make_plan hands such a request eight waves)
      case 3: if constexpr (!(WAVES == 16 && DZ)) QA_SKINNY(3); break;
      default: if constexpr (!(WAVES == 16 && DZ)) QA_SKINNY(4); break;
    }
  }
#undef QA_SKINNY
}

template <int NTW>
static void launch_skinny(const Plan& p, const GemmArgs& a, const Launch& L) {
  if constexpr (NTW == 1) {
    if (p.dz) {  // M <= 16: one channel tile per workgroup
      if (p.waves == 4) launch_skinny_gm<1, 4, true, true>(p, a, L);
      else if (p.waves == 16) launch_skinny_gm<1, 16, true, true>(p, a, L);
      else launch_skinny_gm<1, 8, true, true>(p, a, L);
      return;
    }
  }
  if constexpr (NTW >= 2) {
    if (p.dz && !p.xlds) {
      if (a.ln_w) launch_skinny_gm<NTW, 8, false, true, true>(p, a, L);  // RMSNorm on the fragments (run_gemm checked waves == 8)
      else if (p.waves == 4) launch_skinny_gm<NTW, 4, false, true>(p, a, L);
      else launch_skinny_gm<NTW, 8, false, true>(p, a, L);
      return;
    }
  }
  // (sixteen waves: one-tile workgroups only -- make_plan never asks for more, and with 128 registers per lane the two- and four-tile builds spilled)
  if (p.xlds) {
    if (p.waves == 4) launch_skinny_gm<NTW, 4, true, false>(p, a, L);
    else if (NTW == 1 && p.waves == 16) launch_skinny_gm<1, 16, true, false>(p, a, L);
    else launch_skinny_gm<NTW, 8, true, false>(p, a, L);
  } else {
    if (p.waves == 4) launch_skinny_gm<NTW, 4, false, false>(p, a, L);
    else if (NTW == 1 && p.waves == 16) launch_skinny_gm<1, 16, false, false>(p, a, L);
    else launch_skinny_gm<NTW, 8, false, false>(p, a, L);
  }
}

template <int BMT, int WK, int WN = 4, int TCH = 128>
static void launch_tiled(const Plan& p, const GemmArgs& a, const Launch& L) {
  constexpr int TN = TCH / 16 / WN;  // channel tiles per wave
  dim3 grid((a.N / TCH) * ((a.M + BMT * 16 - 1) / (BMT * 16)), p.ksplit), block(64 * WN * WK);
  const unsigned lds = 2 * 4 * WK * BMT * 1024;
  if (a.span) {
    g_span_unsupported = true;
    return;
  }
#define QA_TILED_K(GMV, ABLV)                                                                                      \
  do {                                                                                                             \
    auto kfn = w4a16_tiled_kernel<BMT, TN, WK, GMV, ABLV, WN>;                                                        \
    static std::atomic<unsigned long long> attr_set{0};                                                                \
    (void)lds_limit_once(attr_set, (const void*)kfn, (int)lds);                                                    \
    hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);                                     \
  } while (0)
#ifdef QUICK_AMD_TOOLS
  if constexpr (BMT == 4 && WN == 4 && TCH == 128) if (p.ablate && a.G == 128) {  // timing experiments (tools/): results are wrong on purpose
    switch (p.ablate) {
      case 1: QA_TILED_K(0, 1); return;
      case 2: QA_TILED_K(0, 2); return;
      case 3: QA_TILED_K(0, 3); return;
      case 4: QA_TILED_K(0, 4); return;
      case 7: QA_TILED_K(0, 7); return;
      case 15: QA_TILED_K(0, 15); return;
      case 16: QA_TILED_K(0, 16); return;
      case 17: QA_TILED_K(0, 17); return;
      case 18: QA_TILED_K(0, 18); return;
      case 20: QA_TILED_K(0, 20); return;
      case 22: QA_TILED_K(0, 22); return;
      case 23: QA_TILED_K(0, 23); return;
      default: break;
    }
  }
#endif
  switch (group_mode(a.G)) {
    case 0: QA_TILED_K(0, 0); break;
    case 1: QA_TILED_K(1, 0); break;
    case 2: QA_TILED_K(2, 0); break;
    case 3: QA_TILED_K(3, 0); break;
    default: QA_TILED_K(4, 0); break;
  }
#undef QA_TILED_K
}

template <int MB, int PAIRS, int NBUF, int WK = 1>
static void launch_ring(const Plan& p, const GemmArgs& a, const Launch& L) {
  dim3 grid(p.ntiles, p.ksplit), block(256 * WK);
  constexpr unsigned lds = NBUF * (MB * 8192 + PAIRS * 8192 + WK * PAIRS * 1024);
#define QA_RING_K(GMV)                                                                                             \
  do {                                                                                                             \
    auto kfn = w4a16_ring_kernel<MB, PAIRS, GMV, NBUF, 0, WK>;                                                     \
    static std::atomic<unsigned long long> attr_set{0};                                                                \
    (void)lds_limit_once(attr_set, (const void*)kfn, (int)lds);                                                    \
    hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);                                     \
  } while (0)
#ifdef QUICK_AMD_TOOLS
  if constexpr ((MB == 2 && PAIRS == 1 && NBUF == 4 && WK == 2) || (MB == 4 && PAIRS == 1 && NBUF == 3 && WK == 2))
    if (p.ablate == 16 && a.G == 128) {  // phase stamps into the workspace (tools/wide_phases.py), nothing else changes
      auto kfn = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 64, WK>;
      (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
      return;
    }
  if constexpr (MB == 2 && PAIRS == 1 && NBUF == 6 && WK == 1)
    if (p.ablate && a.G == 128) {  // timing experiments (results are wrong on purpose)
      auto kfn1 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 1>;
      auto kfn2 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 2>;
      auto kfn5 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 5>;
      auto kfn9 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 9>;
      auto kfn18 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 18>;
      auto kfn = p.ablate == 1 ? kfn1 : (p.ablate == 5 ? kfn5 : (p.ablate == 9 ? kfn9 : (p.ablate == 18 ? kfn18 : kfn2)));
      (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
      return;
    }
  if constexpr (MB == 2 && PAIRS == 1 && WK == 2)
    if (p.ablate && a.G == 128) {
      auto kfn1 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 1, WK>;
      auto kfn2 = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 2, WK>;
      auto kfn = p.ablate == 1 ? kfn1 : kfn2;
      (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
      return;
    }
#endif
  if (a.span) {
    if constexpr (MB == 2 && PAIRS == 1 && ((NBUF == 6 && WK == 1) || (NBUF == 4 && WK == 2))) {
      if (group_mode(a.G) == 0) {
        auto kfn = w4a16_ring_kernel<MB, PAIRS, 0, NBUF, 32, WK>;   // ABL bit 32 = span stamps, nothing else
        (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
        return;
      }
    }
    g_span_unsupported = true;
    return;
  }
  if (group_mode(a.G) == 0) QA_RING_K(0);
  else QA_RING_K(1);
#undef QA_RING_K
}

template <int MB, int PAIRS>
static void launch_wide(const Plan& p, const GemmArgs& a, const Launch& L) {
  if constexpr (MB <= 4 && MB * PAIRS <= 4) {
    if (p.wide_nbuf >= 3 && p.waves == 8) {  // eight waves (two per SIMD), the k16 steps split by parity
      constexpr int NMAX8 = wide_ring_nbuf(MB, PAIRS, 2);
      if (p.wide_nbuf == 3) launch_ring<MB, PAIRS, 3, 2>(p, a, L);
      else if (NMAX8 >= 4 && p.wide_nbuf == 4) launch_ring<MB, PAIRS, (NMAX8 >= 4 ? 4 : 3), 2>(p, a, L);
      else launch_ring<MB, PAIRS, NMAX8, 2>(p, a, L);
      return;
    }
  }
  if constexpr (MB <= 4) {
    if (p.wide_nbuf >= 3) {
      constexpr int NMAX = wide_ring_nbuf(MB, PAIRS);
      if (p.wide_nbuf == 3) launch_ring<MB, PAIRS, 3>(p, a, L);
      else if (NMAX >= 4 && p.wide_nbuf == 4) launch_ring<MB, PAIRS, (NMAX >= 4 ? 4 : 3)>(p, a, L);
      else launch_ring<MB, PAIRS, NMAX>(p, a, L);
      return;
    }
  }
  dim3 grid(p.ntiles, p.ksplit), block(256);
  const unsigned lds = 2 * MB * 32 * 256;
  if (a.span) {
    g_span_unsupported = true;
    return;
  }
#define QA_WIDE_K(GMV)                                                                                             \
  do {                                                                                                             \
    auto kfn = w4a16_wide_kernel<MB, PAIRS, GMV>;                                                                  \
    static std::atomic<unsigned long long> attr_set{0};                                                                \
    (void)lds_limit_once(attr_set, (const void*)kfn, (int)lds);                                                    \
    hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);                                     \
  } while (0)
#ifdef QUICK_AMD_TOOLS
  if constexpr ((MB == 2 && PAIRS == 1) || (MB == 8 && PAIRS == 2) || (MB == 4 && PAIRS == 2))
    if (p.ablate && a.G == 128) {  // timing experiments (results are wrong on purpose)
      auto kfn1 = w4a16_wide_kernel<MB, PAIRS, 0, 1>;
      auto kfn2 = w4a16_wide_kernel<MB, PAIRS, 0, 2>;
      auto kfn64 = w4a16_wide_kernel<MB, PAIRS, 0, 64>;  // phase stamps into the workspace, nothing else changes
      auto kfn = p.ablate == 1 ? kfn1 : (p.ablate == 16 ? kfn64 : kfn2);
      (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
      return;
    }
#endif
  if (group_mode(a.G) == 0) QA_WIDE_K(0);
  else QA_WIDE_K(1);
#undef QA_WIDE_K
}

struct Fusion {
  const void* bias = nullptr;
  const void* residual = nullptr;
  const void* ln_w = nullptr;
  float ln_eps = 0.f;
  int silu_mul = 0;
};

static int run_gemm(const void* x, const void* qweight, const void* scales, const void* qzeros, const Fusion& f, void* y,
                    void* workspace, size_t workspace_bytes, int M, int K, int N, int G, int kernel, int grid_split_k,
                    const Launch& L) {
  if (int rc = check_shapes(M, K, N, G)) return rc;
  const KernelId id = decode_kernel_id(kernel);
  if (id.family > QUICK_KERNEL_XM || kernel < 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "unknown kernel id %d", kernel);
#ifndef QUICK_AMD_TOOLS
  if (id.ablate)  // the timing-experiment builds (wrong results on purpose, phase stamps) are not in the product library
    return fail(QUICK_ERR_INVALID_ARGUMENT, "kernel id %d: bits 16-20 select timing experiments that only a QUICK_AMD_TOOLS build contains", kernel);
  if (id.family == QUICK_KERNEL_XK && (id.b12 || id.b13))  // the twelve-wave (loader waves, bit 12) and sixteen-wave (bit 13) flavours: measured level with the eight-wave one, DESIGN.md 5.9
    return fail(QUICK_ERR_INVALID_ARGUMENT, "kernel id %d: the loader-wave / sixteen-wave flavours of the exchange-K kernels are only in a QUICK_AMD_TOOLS build", kernel);
#endif
  if (id.family == QUICK_KERNEL_TILED && id.b13)  // r01's 32x32x16 flavour of the tiled kernel (measured behind the 16x16x32 one, spilled registers): retired in r06
    return fail(QUICK_ERR_INVALID_ARGUMENT, "kernel id %d: the 32x32x16 flavour of the tiled kernel (bit 13) was retired in r06", kernel);
  if (!x || !qweight || !scales || !qzeros || !y) return fail(QUICK_ERR_INVALID_ARGUMENT, "null tensor pointer");
  const Plan p = plan_for(M, K, N, G, kernel, grid_split_k, f.silu_mul != 0, f.ln_w != nullptr);
  if (f.silu_mul && (f.bias || f.residual)) return fail(QUICK_ERR_INVALID_ARGUMENT, "silu_mul excludes bias and residual");
  if (f.ln_w && !plan_takes_rmsnorm(p))
    return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
  GemmArgs a{(const half_t*)x, (const u32x4*)qweight, (const half_t*)scales, (const uint32_t*)qzeros, (const half_t*)f.bias,
             (const half_t*)f.residual, f.silu_mul, (half_t*)y, nullptr, nullptr, M, K, N, G, std::max(1, G / 128), p.ksplit, p.kt_per_split, p.xcd_gm, nullptr, (const half_t*)f.ln_w, f.ln_eps};
  // (phase stamps: the LAST 2 MiB of the workspace, behind whatever a K split needs)
  if (p.ablate >= 16 && workspace && workspace_bytes >= (size_t)4096 * 8 * 64 + workspace_need(p))
    a.dbg = (unsigned long long*)((char*)workspace + workspace_bytes - (size_t)4096 * 8 * 64);
  a.span = L.span;
  g_span_unsupported = false;
  if (p.ksplit > 1) {
    if (p.ntiles > kMaxSplitTiles) return fail(QUICK_ERR_UNSUPPORTED, "K split over %d output tiles (limit %d)", p.ntiles, kMaxSplitTiles);
    const size_t need = workspace_need(p);
    if (!workspace || workspace_bytes < need)
      return fail(QUICK_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    // QUICK_AMD_CHECK_WORKSPACE=1 (a debugging aid: it synchronises the stream): every launch that meets its partners through the workspace
    // first proves the guarded regions all-zero and answers QUICK_ERR_WORKSPACE otherwise -- a stale granule is indistinguishable from a
    // partner's partial sum, see include/quick_amd.h
    static const bool check_ws = [] {
      const char* e = getenv("QUICK_AMD_CHECK_WORKSPACE");
      return e && *e && atoi(e) != 0;
    }();
    if (check_ws)
      if (int rcw = quick_w4a16_workspace_check(workspace, workspace_bytes, (void*)L.st)) return rcw;
    a.counters = (unsigned*)workspace;  // zero on entry (caller's contract), zero again when the launch completes
    a.slabs = (float*)((char*)workspace + ((p.kernel == QUICK_KERNEL_XK || p.kernel == QUICK_KERNEL_XW) ? counters_bytes(p) : slabs_offset(p)));  // (exchange-K / XW: the zone)
  }
  if (p.kernel == QUICK_KERNEL_LEAN) {
    int abl = a.span ? 32 : 0;
#ifdef QUICK_AMD_TOOLS
    if (p.ablate == 16) abl = 64;  // phase stamps into the workspace (tools/lean_phases.py)
    else if (p.ablate) return fail(QUICK_ERR_INVALID_ARGUMENT, "LEAN: timing-experiment bit 16 (stamps) only");
#endif
    if (!p.lean_tmax || !lean_launch(p.waves, p.lean_tmax, p.mt, abl, a, p.grid_x, (M + 15) / 16, L.st, L.start, L.stop)) {
      if (abl == 32) g_span_unsupported = true;
      return fail(QUICK_ERR_UNSUPPORTED, "no lean build for K=%d G=%d waves=%d (G %% 128 == 0, waves <= K / 128 <= 16 waves, x + table within 160 KiB of LDS)", K, G, p.waves);
    }
  } else if (p.kernel == QUICK_KERNEL_XM) {
    if (f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
    int abl = a.span ? 32 : 0;
#ifdef QUICK_AMD_TOOLS
    if (p.ablate == 16) abl = 64;  // phase stamps into the workspace (tools/xm_phases.py)
    else if (p.ablate) return fail(QUICK_ERR_INVALID_ARGUMENT, "XM: timing-experiment bit 16 (stamps) only");
#endif
    if (!p.lean_tmax || !xm_launch(p.wide_mb, p.wide_pairs, abl, a, p.grid_x, p.ntiles / p.grid_x, L.st, L.start, L.stop))
      return fail(QUICK_ERR_UNSUPPORTED, "no mid-token build for K=%d G=%d (G a power-of-two multiple of 128, 32-bit offsets)", K, G);
  } else if (p.kernel == QUICK_KERNEL_XW) {
    if (f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
    int abl = a.span ? 32 : 0;
#ifdef QUICK_AMD_TOOLS
    if (p.ablate == 16) {               // phase stamps (QUICK_XW_EXP: + a loop experiment, tools/gen_xw_loop.py)
      abl = 64;
      if (const char* e = getenv("QUICK_XW_EXP")) abl += 256 * atoi(e);
    }
    else if (p.ablate == 20) abl = 68;  // ... and no exchange (wrong results)
    else if (p.ablate) return fail(QUICK_ERR_INVALID_ARGUMENT, "XW: timing-experiment bits 16 (stamps) and 20 (no exchange) only");
#endif
    a.xcd_gm |= p.poll_log2 << 8;  // (the kernel reads the tile-order rows from the low byte)
    if (p.xw_stagger) {            // staggered K ranges: its own build, d in bits 16-17
      abl |= 128;
      a.xcd_gm |= p.xw_stagger << 16;
    }
    if (!xw_launch(p.wide_mb, p.wide_pairs, p.ksplit, abl, a, p.ntiles * p.ksplit, L.st, L.start, L.stop)) {
      if (abl == 32) g_span_unsupported = true;
      return fail(QUICK_ERR_UNSUPPORTED, "no four-wave build for tokens=%d channels=%d slices=%d abl=%d", p.wide_mb * 32, p.tch, p.ksplit, abl);
    }
  } else if (p.kernel == QUICK_KERNEL_XK) {
    if (f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
    if (f.silu_mul && !xk_takes_silu(p))
      return fail(QUICK_ERR_UNSUPPORTED, "exchange-K kernels: SiLU * mul only where a wave finishes whole 32-token blocks");
    // (tools builds: kernel bits 16-20 = 16 phase stamps only; 17 loads only; 18 no loads; 19 no loads, no B-fragment reads; 20 no cross-CU
    // exchange; 21 no loads, no dequantisation; 22 MFMAs + barrier; 23 no loads, no barrier; 24 MFMAs only -- all with the stamps)
    static const int xk_abl[9] = {64, 65, 66, 82, 68, 74, 90, 98, 122};
    int abl = p.ablate == 0 ? (a.span ? 32 : 0) : ((p.ablate >= 16 && p.ablate <= 24) ? xk_abl[p.ablate - 16] : -1);  // (32: in-kernel span stamps, a measurement aid)
#ifdef QUICK_AMD_TOOLS
    if (p.ablate)  // (experiments whose bits do not fit the kernel id: the ABL value itself, tools/xk_phases.py --env-abl)
      if (const char* e = getenv("QUICK_XK_ABL")) abl = atoi(e) == 0 && a.span ? 32 : atoi(e);
#endif
    if (const char* e = getenv("QUICK_AMD_EXCHANGE_POLL_LOG2")) a.xcd_gm |= std::max(0, std::min(31, atoi(e))) << 8;   // (tests: 1 = every wave gives its part up at once)
    if (!xk_launch(XkConfig{p.wide_mb, p.ksplit, p.xk_nbuf, p.xk_wd, abl, p.xk_kq, p.xk_loader ? 1 : 0}, a, p.ntiles * p.ksplit, L.st, L.start, L.stop)) {
      if (abl == 32) {
        g_span_unsupported = true;
        return fail(QUICK_ERR_UNSUPPORTED, "no span-stamped build of the kernel this shape runs");
      }
      return fail(QUICK_ERR_UNSUPPORTED, "no exchange-K build for tokens=%d slices=%d ring=%d queue=%d%s", p.wide_mb * 32, p.ksplit, p.xk_nbuf,
                  p.xk_wd, abl ? " (timing-experiment bits need a QUICK_AMD_TOOLS build)" : "");
    }
  } else if (p.kernel == QUICK_KERNEL_WIDE) {
    if (f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
    const int sel = p.wide_mb * 10 + p.wide_pairs;
    switch (sel) {
      case 21: launch_wide<2, 1>(p, a, L); break;
      case 22: launch_wide<2, 2>(p, a, L); break;
      case 41: launch_wide<4, 1>(p, a, L); break;
      case 42: launch_wide<4, 2>(p, a, L); break;
      case 81: launch_wide<8, 1>(p, a, L); break;
#ifdef QUICK_AMD_TOOLS
      default: launch_wide<8, 2>(p, a, L); break;   // r02's hipcc-scheduled 256 x 256 tile (92 bytes of scratch): the A/B partner of the generated loop, tools builds only
#else
      default: return fail(QUICK_ERR_UNSUPPORTED, "the hipcc-scheduled 256 x 256 tile is only in a QUICK_AMD_TOOLS build (the product runs the generated loop, w4a16_xw.hpp, or 128 x 256 tiles)");
#endif
    }
  } else if (p.kernel == QUICK_KERNEL_SKINNY) {
    switch (p.mt) {
      case 1: launch_skinny<1>(p, a, L); break;
      case 2: launch_skinny<2>(p, a, L); break;
      case 7: {   // seven tiles per workgroup: the straight-line fragment kernel with T = 8, one slice
        if (p.frag8_t != 8 || p.ksplit != 1 || f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "skinny: seven channel tiles per workgroup only in the straight-line fragment kernel (K = 8192, one slice), no RMSNorm prologue");
        dim3 grid(p.grid_x, (M + 15) / 16, 1), block(512);
        const unsigned lds = 8 * 7 * 1024;
        if (a.span) {
          auto kfn = w4a16_frag8_kernel<8, true, true, 7>;
          static std::atomic<unsigned long long> attr_set_s{0};
          (void)lds_limit_once(attr_set_s, (const void*)kfn, (int)kLdsPerCu);
          hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
        } else {
          auto kfn = w4a16_frag8_kernel<8, true, false, 7>;
          static std::atomic<unsigned long long> attr_set{0};
          (void)lds_limit_once(attr_set, (const void*)kfn, (int)kLdsPerCu);
          hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);
        }
        break;
      }
      case 8: {
        if (!p.frag8_t || f.ln_w) return fail(QUICK_ERR_UNSUPPORTED, "skinny: eight channel tiles per workgroup only in the straight-line fragment kernel, no RMSNorm prologue");
        dim3 grid(p.grid_x, (M + 15) / 16, p.ksplit), block(512);
        const unsigned lds = 8 * 8 * 1024;
#define QA_FRAG8(TV)                                                                                               \
  do {                                                                                                             \
    if (a.span) { /* in-kernel span stamps (a measurement aid): the same kernel + two stamps */                    \
      auto kfn = w4a16_frag8_kernel<TV, true, true>;                                                               \
      static std::atomic<unsigned long long> attr_set_s{0};                                                        \
      (void)lds_limit_once(attr_set_s, (const void*)kfn, (int)kLdsPerCu);                                          \
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);                                   \
    } else {                                                                                                       \
      auto kfn = w4a16_frag8_kernel<TV, true>;                                                                     \
      static std::atomic<unsigned long long> attr_set{0};                                                          \
      (void)lds_limit_once(attr_set, (const void*)kfn, (int)kLdsPerCu);                                            \
      hipExtLaunchKernelGGL(kfn, grid, block, lds, L.st, L.start, L.stop, 0, a);                                   \
    }                                                                                                              \
  } while (0)
        switch (p.frag8_t) {
          case 2: QA_FRAG8(2); break;
          case 4: QA_FRAG8(4); break;
          case 7: QA_FRAG8(7); break;
          default: QA_FRAG8(8); break;
        }
#undef QA_FRAG8
        break;
      }
      default: launch_skinny<4>(p, a, L); break;
    }
  } else {
    if (p.tch == 256 && p.mt == 8) launch_tiled<8, 1, 4, 256>(p, a, L);  // 128 x 256, four waves of 128 tokens x 64 channels
    else if (p.tch == 256) launch_tiled<4, 2, 4, 256>(p, a, L);    // 64 tokens x 256 channels, 4 channel tiles per wave
    else if (p.mt == 4 && p.wn2) launch_tiled<4, 4, 2>(p, a, L);  // 2 waves along N x 4 along K, 64 channels per wave
    else if (p.mt == 2) launch_tiled<2, 2>(p, a, L);
    else if (p.mt == 8) launch_tiled<8, 2>(p, a, L);
    else if (p.waves == 8) launch_tiled<4, 2>(p, a, L);
    else launch_tiled<4, 4>(p, a, L);
  }
  if (g_span_unsupported) return fail(QUICK_ERR_UNSUPPORTED, "no span-stamped build of the kernel this shape runs");
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(QUICK_ERR_LAUNCH, "kernel launch failed: %s", hipGetErrorString(e));
  return QUICK_OK;
}

}  // namespace quick_amd

using namespace quick_amd;

extern "C" {

int quick_amd_abi_version(void) { return QUICK_AMD_ABI_VERSION; }
const char* quick_amd_last_error(void) { return g_err; }

size_t quick_w4a16_workspace_bytes_ex(int M, int K, int N, int group_size, int kernel, int grid_split_k) {
  if (check_shapes(M, K, N, group_size) != QUICK_OK) return 0;
  return plan_workspace_bytes(M, K, N, group_size, kernel, grid_split_k);
}

size_t quick_w4a16_workspace_bytes(int M, int K, int N, int group_size, int split_k_iters) {
  (void)split_k_iters;
  return quick_w4a16_workspace_bytes_ex(M, K, N, group_size, QUICK_KERNEL_AUTO, 0);
}

int quick_w4a16_gemm_f16_ex(const void* x, const void* qweight, const void* scales, const void* qzeros,
                            const void* bias, void* y, void* workspace, size_t workspace_bytes, int M, int K, int N,
                            int group_size, int kernel, int grid_split_k, void* hip_stream) {
  const Launch L{(hipStream_t)hip_stream, nullptr, nullptr};
  Fusion f;
  f.bias = bias;
  return run_gemm(x, qweight, scales, qzeros, f, y, workspace, workspace_bytes, M, K, N, group_size, kernel, grid_split_k, L);
}

int quick_w4a16_gemm_f16_fused(const void* x, const void* qweight, const void* scales, const void* qzeros,
                               const quick_gemm_fusion* fusion, void* y, void* workspace, size_t workspace_bytes, int M,
                               int K, int N, int group_size, int kernel, int grid_split_k, void* hip_stream) {
  const Launch L{(hipStream_t)hip_stream, nullptr, nullptr};
  Fusion f;
  if (fusion) {
    f.bias = fusion->bias;
    f.residual = fusion->residual;
    f.ln_w = fusion->rmsnorm_weight;
    f.ln_eps = fusion->rmsnorm_eps;
    f.silu_mul = fusion->silu_mul;
  }
  return run_gemm(x, qweight, scales, qzeros, f, y, workspace, workspace_bytes, M, K, N, group_size, kernel, grid_split_k, L);
}

int quick_w4a16_can_fuse_rmsnorm(int M, int K, int N, int group_size) {
  if (check_shapes(M, K, N, group_size) != QUICK_OK) return 0;
  // the deferred-zero skinny kernel copies (and tabulates) x per workgroup anyway: normalising on the way costs a
  // second pass over LDS, not a launch
  const Plan p = plan_for(M, K, N, group_size, QUICK_KERNEL_AUTO, 0, false, false);
  if (!plan_takes_rmsnorm(p)) return 0;
  if (p.kernel == QUICK_KERNEL_LEAN) return p.lean_tmax > 0;   // sums of squares of the LDS copy, one barrier, x normalised in LDS
  // The fragment flavour pays for the norm in registers (a pass over x for the sums of squares in front of the loop, the normalisation
  // fp16(fp16(x * rstd) * w) on every x fragment of every channel block; the bound below was measured with r05's construction, x * w in
  // fp16 and the squares on every fragment): on a very large layer that is more than a separate launch of quick_rmsnorm_f16.  Llama-2-70B at bs = 16, one-session
  // A/B (profiles/r05_decode70_ab.txt): gate_up (8192 x 57344) un-fused 1412 -> 1456 tok/s, every fragment launch un-fused 1426; Mistral-7B's
  // 4096 x 28672 at bs = 32 LOSES 2 % un-fused.  So: fused up to K * N = 2^28.
  if (!p.xlds && (long)K * N > (1L << 28)) return 0;
  return 1;
}

int quick_w4a16_plan_describe(int M, int K, int N, int group_size, int kernel, int grid_split_k, char* text, size_t text_bytes) {
  const int rc = check_shapes(M, K, N, group_size);
  if (rc != QUICK_OK) return rc;
  if (!text || text_bytes == 0) return fail(QUICK_ERR_INVALID_ARGUMENT, "no text buffer");
  plan_describe(M, K, N, group_size, kernel, grid_split_k, text, text_bytes);
  return QUICK_OK;
}

int quick_w4a16_gemm_profile(const void* x, const void* const* qweights, const void* const* scales,
                             const void* const* qzeros, int n_sets, void* y, void* workspace, size_t workspace_bytes,
                             int M, int K, int N, int group_size, int kernel, int grid_split_k, int iters,
                             float* kernel_us, void* hip_stream) {
  if (n_sets < 1 || iters < 1 || !kernel_us) return fail(QUICK_ERR_INVALID_ARGUMENT, "bad profile arguments");
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<hipEvent_t> ev(2 * (size_t)iters);
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(QUICK_ERR_LAUNCH, "hipEventCreate failed");
  int rc = QUICK_OK;
  for (int i = 0; i < iters && rc == QUICK_OK; ++i) {
    const int s = i % n_sets;
    const Launch L{st, ev[2 * i], ev[2 * i + 1]};
    rc = run_gemm(x, qweights[s], scales[s], qzeros[s], Fusion{}, y, workspace, workspace_bytes, M, K, N, group_size,
                  kernel, grid_split_k, L);
  }
  if (rc == QUICK_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(QUICK_ERR_LAUNCH, "stream synchronize failed");
  for (int i = 0; i < iters; ++i) {
    float ms = 0.f;
    if (rc == QUICK_OK && hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess)
      rc = fail(QUICK_ERR_LAUNCH, "hipEventElapsedTime failed");
    kernel_us[i] = ms * 1000.f;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

int quick_w4a16_gemm_span(const void* x, const void* const* qweights, const void* const* scales, const void* const* qzeros,
                          int n_sets, void* y, void* workspace, size_t workspace_bytes, int M, int K, int N, int group_size,
                          int kernel, int grid_split_k, int iters, float* span_us, void* hip_stream) {
  if (n_sets < 1 || iters < 1 || iters > 256 || !span_us) return fail(QUICK_ERR_INVALID_ARGUMENT, "bad span arguments (1..256 launches)");
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t per = 2 * (size_t)kSpanWaves;  // u64 words per launch
  unsigned long long* dev = nullptr;
  if (hipMalloc(&dev, (size_t)iters * per * 8) != hipSuccess) return fail(QUICK_ERR_LAUNCH, "hipMalloc failed");
  int rc = QUICK_OK;
  for (int i = 0; i < iters && rc == QUICK_OK; ++i) {  // starts: all ones, ends: zero
    if (hipMemsetAsync(dev + i * per, 0xff, kSpanWaves * 8, st) != hipSuccess ||
        hipMemsetAsync(dev + i * per + kSpanWaves, 0, kSpanWaves * 8, st) != hipSuccess)
      rc = fail(QUICK_ERR_LAUNCH, "memset failed");
  }
  for (int i = 0; i < iters && rc == QUICK_OK; ++i) {
    const int s = i % n_sets;
    Launch L{st, nullptr, nullptr};
    L.span = dev + i * per;
    rc = run_gemm(x, qweights[s], scales[s], qzeros[s], Fusion{}, y, workspace, workspace_bytes, M, K, N, group_size, kernel,
                  grid_split_k, L);
  }
  std::vector<unsigned long long> host(per);
  for (int i = 0; i < iters; ++i) {
    span_us[i] = 0.f;
    if (rc != QUICK_OK) continue;
    if (hipMemcpyAsync(host.data(), dev + i * per, per * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      rc = fail(QUICK_ERR_LAUNCH, "reading the span stamps back failed");
      continue;
    }
    unsigned long long lo = ~0ull, hi = 0ull;
    for (unsigned w = 0; w < kSpanWaves; ++w) {
      lo = std::min(lo, host[w]);
      hi = std::max(hi, host[kSpanWaves + w]);
    }
    span_us[i] = hi > lo ? (float)((double)(hi - lo) * 0.01) : 0.f;  // 100 MHz ticks
  }
  (void)hipFree(dev);
  return rc;
}

int quick_amd_dispatch_floor(int iters, float* kernel_us, void* hip_stream) {
  if (iters < 1 || !kernel_us) return fail(QUICK_ERR_INVALID_ARGUMENT, "bad arguments");
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<hipEvent_t> ev(2 * (size_t)iters);
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(QUICK_ERR_LAUNCH, "hipEventCreate failed");
  for (int i = 0; i < iters; ++i)
    hipExtLaunchKernelGGL(w4a16_empty_kernel, dim3(256), dim3(512), 0, st, ev[2 * i], ev[2 * i + 1], 0, (unsigned*)nullptr);
  int rc = hipStreamSynchronize(st) == hipSuccess ? QUICK_OK : fail(QUICK_ERR_LAUNCH, "stream synchronize failed");
  for (int i = 0; i < iters; ++i) {
    float ms = 0.f;
    if (rc == QUICK_OK && hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess)
      rc = fail(QUICK_ERR_LAUNCH, "hipEventElapsedTime failed");
    kernel_us[i] = ms * 1000.f;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

int quick_w4a16_workspace_check(const void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!workspace || workspace_bytes == 0) return QUICK_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  // [r06, ADVICE r05] the scan allocates, copies back and synchronises: none of that is legal while the stream is being captured into a graph --
  // say so instead of invalidating the capture (QUICK_AMD_CHECK_WORKSPACE=1 reaches here from every split launch)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(QUICK_ERR_INVALID_ARGUMENT, "quick_w4a16_workspace_check synchronises the stream and cannot run while it is being captured into a hipGraph (unset QUICK_AMD_CHECK_WORKSPACE for captured launches)");
  const size_t guarded = std::min(workspace_bytes, (size_t)kMaxSplitTiles * 4 + kXkZoneBytesHost) & ~(size_t)15;
  unsigned* first = nullptr;
  if (hipMalloc(&first, sizeof(unsigned)) != hipSuccess) return fail(QUICK_ERR_LAUNCH, "hipMalloc failed");
  int rc = QUICK_OK;
  unsigned host = 0xffffffffu;
  if (hipMemsetAsync(first, 0xff, sizeof(unsigned), st) != hipSuccess) rc = fail(QUICK_ERR_LAUNCH, "memset failed");
  if (rc == QUICK_OK) {
    hipLaunchKernelGGL(w4a16_workspace_scan_kernel, dim3(1024), dim3(256), 0, st, (const u32x4*)workspace, (unsigned)(guarded / 16), first);
    if (hipGetLastError() != hipSuccess) rc = fail(QUICK_ERR_LAUNCH, "workspace scan kernel did not launch");
    if (rc == QUICK_OK) if (hipMemcpyAsync(&host, first, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      rc = fail(QUICK_ERR_LAUNCH, "workspace scan failed: %s", hipGetErrorString(hipGetLastError()));
  }
  (void)hipFree(first);
  if (rc == QUICK_OK && host != 0xffffffffu)
    rc = fail(QUICK_ERR_WORKSPACE, "workspace is not zero at byte %u (%s): an aborted launch, a buffer that was never zeroed, or two streams sharing it; zero it again before the next call",
              host, (size_t)host < (size_t)kMaxSplitTiles * 4 ? "arrival counters / part state words" : "exchange zone");
  return rc;
}

int quick_w4a16_gemm_f16(const void* x, const void* qweight, const void* scales, const void* qzeros, void* y,
                         void* workspace, size_t workspace_bytes, int M, int K, int N, int group_size,
                         int split_k_iters, void* hip_stream) {
  if (split_k_iters < 1) return fail(QUICK_ERR_INVALID_ARGUMENT, "split_k_iters must be >= 1");
  return quick_w4a16_gemm_f16_ex(x, qweight, scales, qzeros, nullptr, y, workspace, workspace_bytes, M, K, N,
                                 group_size, QUICK_KERNEL_AUTO, 0, hip_stream);
}

int quick_dequantize_mi355x_f16(const void* qweight, const void* scales, const void* qzeros, void* w_out, int K,
                                int N, int group_size, void* hip_stream) {
  if (int rc = check_shapes(1, K, N, group_size)) return rc;
  hipLaunchKernelGGL(w4a16_dequant_kernel, dim3(N / 16, K / 128), dim3(64), 0, (hipStream_t)hip_stream,
                     (const u32x4*)qweight, (const half_t*)scales, (const uint32_t*)qzeros, (half_t*)w_out, K, N,
                     group_size);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(QUICK_ERR_LAUNCH, "kernel launch failed: %s", hipGetErrorString(e));
  return QUICK_OK;
}

}  // extern "C"
