// W4A16 GEMM for MI355X (gfx950): y[M,N] = x[M,K] @ fp16((w - z) * s).  The skinny family (M <= 64): kernels, instantiations and launcher.
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
//     from L2.  (The tiled kernel for large M is in w4a16_tiled.hip.)
#include "w4a16_common.hpp"

#include "w4a16_args.hpp"
#include "w4a16_launch.hpp"
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
    for (int kt = kt_begin; kt < kt_end; kt += 2 * U) {
      if (kt + U < kt_end) skinny_load<NTW, GM, U, XLDS, LN, NT>(cB, kt + U, kt_end - 1, bufs, cb, xp, a, gp);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (DZ) skinny_compute_dzf<NTW, GM, U, LN>(cA, kt, kt_end, bconst, (lane & 1) != 0, acc, rstd);
      else skinny_compute<NTW, GM, U, XLDS>(cA, kt, kt_end, nullptr, acc);
      if (kt + U >= kt_end) break;
      if (kt + 2 * U < kt_end) skinny_load<NTW, GM, U, XLDS, LN, NT>(cA, kt + 2 * U, kt_end - 1, bufs, cb, xp, a, gp);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (DZ) skinny_compute_dzf<NTW, GM, U, LN>(cB, kt + U, kt_end, bconst, (lane & 1) != 0, acc, rstd);
      else skinny_compute<NTW, GM, U, XLDS>(cB, kt + U, kt_end, nullptr, acc);
    }
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

template <int NTW, int WAVES, int GM, bool XLDS, bool DZ, bool LN, bool SPAN = false, bool NT = false>
static bool skinny_go(const GemmArgs& a, const Launch& L, dim3 grid, unsigned lds) {
  launch_kernel<w4a16_skinny_kernel<NTW, WAVES, GM, XLDS, DZ, LN, SPAN, NT>>(L, grid, dim3(WAVES * 64), lds, (int)kLdsPerCu, a);
  return true;
}

template <int NTW, int WAVES, bool XLDS, bool DZ, bool LN = false>
static bool launch_skinny_gm(const Plan& p, const GemmArgs& a, const Launch& L) {
  const dim3 grid(p.grid_x, (a.M + 15) / 16, p.ksplit);
  const unsigned lds = (unsigned)(skinny_lds_bytes(a.M, a.G, NTW, WAVES, p.kt_per_split, p.grid_x < a.N / (16 * NTW), XLDS, DZ) + (LN ? 1024 : 0));
  const int gm = group_mode(a.G);
  if (a.span) {  // in-kernel span stamps: separate instantiations, for the small-M kernels the BASELINE sweep and the decode shapes run
    constexpr bool stamped = !LN && ((WAVES == 8 && ((NTW == 1 && XLDS && DZ) || (NTW == 1 && !XLDS && !DZ) || (NTW == 4 && !XLDS && DZ))) ||
                                     (WAVES == 16 && NTW == 1 && ((XLDS && DZ) || (!XLDS && !DZ))));
    if constexpr (stamped) {
      if (gm == 0) {   // [r06, ADVICE r05] the stamped build of the kernel the product runs: nt weight requests with one token block
        if (a.M <= 16) return skinny_go<NTW, WAVES, 0, XLDS, DZ, LN, true, true>(a, L, grid, lds);
        return skinny_go<NTW, WAVES, 0, XLDS, DZ, LN, true>(a, L, grid, lds);
      }
    }
    return false;
  }
  if (a.M <= 16 && gm == 0)  // one token block: weights streamed once -> nt requests (see skinny_load)
    return skinny_go<NTW, WAVES, 0, XLDS, DZ, LN, false, true>(a, L, grid, lds);
  if constexpr (LN) {  // only reached with G % 128 == 0
    if (gm == 0) return skinny_go<NTW, WAVES, 0, XLDS, DZ, LN>(a, L, grid, lds);
    return skinny_go<NTW, WAVES, 1, XLDS, DZ, LN>(a, L, grid, lds);
  } else {
    switch (gm) {
      case 0: return skinny_go<NTW, WAVES, 0, XLDS, DZ, LN>(a, L, grid, lds);
      case 1: return skinny_go<NTW, WAVES, 1, XLDS, DZ, LN>(a, L, grid, lds);
      case 2: return skinny_go<NTW, WAVES, 2, XLDS, DZ, LN>(a, L, grid, lds);
      // (sixteen waves of the table flavour with > 2 units per k tile: no build -- it spilled; make_plan hands such a request eight waves)
      case 3:
        if constexpr (!(WAVES == 16 && DZ)) return skinny_go<NTW, WAVES, 3, XLDS, DZ, LN>(a, L, grid, lds);
        return false;
      default:
        if constexpr (!(WAVES == 16 && DZ)) return skinny_go<NTW, WAVES, 4, XLDS, DZ, LN>(a, L, grid, lds);
        return false;
    }
  }
}

template <int NTW>
static bool launch_skinny(const Plan& p, const GemmArgs& a, const Launch& L) {
  if constexpr (NTW == 1) {
    if (p.dz) {  // M <= 16: one channel tile per workgroup
      if (p.waves == 4) return launch_skinny_gm<1, 4, true, true>(p, a, L);
      if (p.waves == 16) return launch_skinny_gm<1, 16, true, true>(p, a, L);
      return launch_skinny_gm<1, 8, true, true>(p, a, L);
    }
  }
  if constexpr (NTW >= 2) {
    if (p.dz && !p.xlds) {
      if (a.ln_w) return launch_skinny_gm<NTW, 8, false, true, true>(p, a, L);  // RMSNorm on the fragments (plan_takes_rmsnorm: eight waves only)
      if (p.waves == 4) return launch_skinny_gm<NTW, 4, false, true>(p, a, L);
      return launch_skinny_gm<NTW, 8, false, true>(p, a, L);
    }
  }
  // (sixteen waves: one-tile workgroups only -- make_plan never asks for more, and with 128 registers per lane the two- and four-tile builds spilled)
  if (p.xlds) {
    if (p.waves == 4) return launch_skinny_gm<NTW, 4, true, false>(p, a, L);
    if (NTW == 1 && p.waves == 16) return launch_skinny_gm<1, 16, true, false>(p, a, L);
    return launch_skinny_gm<NTW, 8, true, false>(p, a, L);
  }
  if (p.waves == 4) return launch_skinny_gm<NTW, 4, false, false>(p, a, L);
  if (NTW == 1 && p.waves == 16) return launch_skinny_gm<1, 16, false, false>(p, a, L);
  return launch_skinny_gm<NTW, 8, false, false>(p, a, L);
}

// the straight-line fragment kernel: T k tiles per wave, NTW channel tiles per workgroup; every build has its span-stamped twin
template <int T, int NTW>
static bool launch_frag8(const Plan& p, const GemmArgs& a, const Launch& L) {
  const dim3 grid(p.grid_x, (a.M + 15) / 16, p.ksplit), block(512);
  const unsigned lds = 8 * NTW * 1024;
  if (a.span) launch_kernel<w4a16_frag8_kernel<T, true, true, NTW>>(L, grid, block, lds, (int)kLdsPerCu, a);
  else launch_kernel<w4a16_frag8_kernel<T, true, false, NTW>>(L, grid, block, lds, (int)kLdsPerCu, a);
  return true;
}

bool skinny_launch(const Plan& p, const GemmArgs& a, const Launch& L) {
  switch (p.mt) {
    case 1: return launch_skinny<1>(p, a, L);
    case 2: return launch_skinny<2>(p, a, L);
    case 7: return launch_frag8<8, 7>(p, a, L);  // seven tiles per workgroup: T = 8, one slice (run_skinny checked both)
    case 8:
      switch (p.frag8_t) {
        case 2: return launch_frag8<2, 8>(p, a, L);
        case 4: return launch_frag8<4, 8>(p, a, L);
        case 7: return launch_frag8<7, 8>(p, a, L);
        default: return launch_frag8<8, 8>(p, a, L);
      }
    default: return launch_skinny<4>(p, a, L);
  }
}

}  // namespace quick_amd
