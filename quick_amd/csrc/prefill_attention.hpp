// Causal attention of T new tokens over the KV cache (prefill, chunked prefill, second chat turn, speculative verify): query t of a
// sequence attends cache rows 0 .. *pos0 + t.  The reference does this in eager torch with a materialised mask
// (quick/awq/modules/fused/attn.py:166-210); here it is one launch with both products on the matrix core and no score matrix in memory.
//
// Tiling.  A workgroup is four waves and serves 64 consecutive query rows of one (sequence, query head), 16 per wave; the rotated query
// rows stay in registers for the whole launch (the B operand of v_mfma_f32_16x16x32_f16: query = lane % 16, dims 32 s + 8 (lane / 16) ..).
// The cache is walked in tiles of 32 rows, staged ONCE per workgroup in LDS through registers: the requests for tile i + 1 leave before
// tile i is consumed and are written behind the next barrier.  K lies row-major with its 16-byte pieces XOR-swizzled by the row (the
// A-operand reads of 16 rows at one column range are then conflict-free); V lies TRANSPOSED, [dim][key slot], so that the A operand of
// the second product is one 16-byte read.  Tiles wholly behind the workgroup's (a wave: behind its own) last query are skipped, and only
// the tiles that straddle a wave's diagonal are masked.
//
//   S^T = K Q^T   two 16-key blocks x four k steps: lane (query, quarter) holds the scores of keys 16 blk + 4 quarter + i of the tile
//   softmax       online, in the log2 domain: running max and sum per query in fp32 (the max shared by the query's four lanes, the sum
//                 kept per lane and added up once at the end)
//   O^T = V^T P^T eight 16-dim blocks: the weights of a lane ARE its B fragment (key slot 8 quarter + 4 blk + i -- V is staged in that
//                 order), and the accumulators hold the query on the lane, like the running max: the rescale needs no lane traffic
//
// Rounding points.  Scores are fp32 sums of exact fp16 x fp16 products (four 32-product MFMAs), times scale * log2 e in fp32; max, exp2
// and the running sum in fp32.  P IS ROUNDED TO FP16 as the operand of the second product (the sum l adds the unrounded fp32 weights);
// P V accumulates in fp32, one rescale per tile; at the end one fp32 division by l and one rounding to fp16.
//
// Poisoned rows.  Rows at or behind *pos0 + T may hold anything.  They are never requested: staging clamps the row index to
// *pos0 + T - 1, so the tail of the last tile holds copies of a written (finite) row, whose weights the causal mask sets to zero -- a zero
// weight times an Inf value would be NaN inside the MFMA, masking P alone is not enough there.  Scores are replaced by -inf by the row
// INDEX before the max and the exp, so a NaN score cannot reach either.  The kernel reads the caches and never writes them; no atomics,
// no spinning, no workspace.  O leaves through LDS as whole rows in 16-byte pieces, [B * T, nh * D]: the matrix o_proj's GEMM consumes.
// This header holds the kernel and its launcher for ONE of two forms, chosen by the unit that includes it: PA_KERNEL names the kernel and
// PA_SEQ says whether it reads one position for the batch (false: prefill_attention.hip, quick_prefill_attention_f16) or one per sequence
// (true: prefill_attention_seq.hip, quick_prefill_attention_seq_f16).  Plain kernels, not instantiations of a template: as a template the
// shared form's LDS arrays were laid out in another order and its address arithmetic came out rearranged -- 1 to 3 % slower on one-sequence
// shapes (profiles/per_sequence_attention.txt) -- while the plain kernel of that name compiles to the code it always was.
#pragma once
#include <cstdio>
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

namespace quick_amd {

constexpr int PA_QROWS = 64;    // query rows per workgroup (16 per wave)
constexpr int PA_KVROWS = 32;   // cache rows per tile
constexpr int PA_WAVES = 4;
constexpr int PA_VSTRIDE = 20;  // dwords per row of the transposed V image: 16 key pairs + 4 of padding (rows stay 16-byte aligned)

// SEQ: pos0 holds one start per sequence (workgroup (., ., b) uses pos0[b]); a sequence whose start lies outside 0 .. L - T is skipped,
// its workgroups leave before the first barrier and write nothing.  The shared form (SEQ = false) pulls *pos0 inside, as it always did.
__global__ __launch_bounds__(PA_WAVES * 64) void PA_KERNEL(const half_t* __restrict__ q, const half_t* __restrict__ k_cache,
                                                                          const half_t* __restrict__ v_cache, const long* __restrict__ pos0,
                                                                          half_t* __restrict__ out, int T, int nh, int nkv, int L, float scale) {
  constexpr int D = 128;
  constexpr bool SEQ = PA_SEQ;
  __shared__ __attribute__((aligned(16))) half_t k_lds[PA_KVROWS * D];        // [key][16-byte piece ^ (key & 15)]
  __shared__ __attribute__((aligned(16))) uint32_t v_lds[D * PA_VSTRIDE];     // [dim][key pair], quads of pairs XOR-ed with (dim / 16) & 3
  __shared__ __attribute__((aligned(16))) half_t o_lds[PA_WAVES][16 * D];     // the waves' output rows on their way out
  const int b = blockIdx.z, h = blockIdx.y, kvh = h / (nh / nkv), t0 = blockIdx.x * PA_QROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int qi = lane & 15, rsel = lane >> 4;
  // (the caller keeps 0 <= *pos0 <= L - T; a value outside is pulled inside so that no address leaves the caches)
  const long praw = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (praw < 0 || praw > L - T) return;   // (workgroup-uniform)
  }
  const int p0 = uniform(min(max((int)praw, 0), L - T));
  const int last = p0 + T - 1;                                   // the last written cache row: staging reads nothing behind it
  const int tw0 = t0 + 16 * wave;                                // this wave's first query
  const bool wave_active = tw0 < T;
  const int wave_first = p0 + tw0, wave_last = p0 + min(tw0 + 15, T - 1);   // the causal limits of its first and last query
  const int tq = min(tw0 + qi, T - 1);                           // (rows behind T: the last query again, not stored)
  const int limit = p0 + tq;                                     // this lane's query attends cache rows 0 .. limit
  const int ntiles = (p0 + min(t0 + PA_QROWS - 1, T - 1)) / PA_KVROWS + 1;

  const half_t* qp = q + (((size_t)b * nh + h) * T + tq) * D + 8 * rsel;
  half8_t qb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qb[s] = *(const half8_t*)(qp + 32 * s);

  // staging: thread (row pair pi = tid / 16, piece c = tid % 16).  K rows pi and 16 + pi; V the two rows of key-slot pair pi, which are
  // neighbours in the cache: slots 8 r + j hold rows 4 r + j (j < 4) and 16 + 4 r + j - 4 (j >= 4)
  const int pi = tid >> 4, c = tid & 15;
  const int vrow = (pi & 2 ? 16 : 0) + 4 * (pi >> 2) + 2 * (pi & 1);
  const half_t* kp = k_cache + ((size_t)b * nkv + kvh) * L * D + c * 8;
  const half_t* vp = v_cache + ((size_t)b * nkv + kvh) * L * D + c * 8;
  half8_t kreg[2], vreg[2];
  auto request = [&](int tile0) __attribute__((always_inline)) {
    kreg[0] = *(const half8_t*)(kp + (size_t)min(tile0 + pi, last) * D);
    kreg[1] = *(const half8_t*)(kp + (size_t)min(tile0 + 16 + pi, last) * D);
    vreg[0] = *(const half8_t*)(vp + (size_t)min(tile0 + vrow, last) * D);
    vreg[1] = *(const half8_t*)(vp + (size_t)min(tile0 + vrow + 1, last) * D);
  };
  auto stage = [&]() __attribute__((always_inline)) {
    *(half8_t*)(k_lds + pi * D + ((c ^ pi) * 8)) = kreg[0];             // (rows pi and 16 + pi: the same row & 15)
    *(half8_t*)(k_lds + (16 + pi) * D + ((c ^ pi) * 8)) = kreg[1];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = c * 8 + e;
      v_lds[d * PA_VSTRIDE + (((pi >> 2) ^ ((d >> 4) & 3)) * 4) + (pi & 3)] = as_u32(half2_t{vreg[0][e], vreg[1][e]});
    }
  };

  const float qk_scale = scale * 1.44269504088896f;   // scores in the log2 domain
  float m_ = -INFINITY, l_ = 0.f;                     // of query qi: the max over all rows so far, the sum over this lane's rows
  floatx4 oacc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) oacc[db] = floatx4{0.f, 0.f, 0.f, 0.f};

  request(0);
  for (int it = 0; it < ntiles; ++it) {
    const int tile0 = it * PA_KVROWS;
    __syncthreads();   // the previous tile has been read by everyone
    stage();
    __syncthreads();
    if (it + 1 < ntiles) request(tile0 + PA_KVROWS);
    if (wave_active && tile0 <= wave_last) {   // (wave-uniform; else the tile lies wholly behind this wave's last query)
      floatx4 d4[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8_t ka = *(const half8_t*)(k_lds + (16 * blk + qi) * D + (((4 * s + rsel) ^ qi) * 8));
          d4[blk] = mfma16(ka, qb[s], d4[blk]);
        }
      const bool diagonal = tile0 + PA_KVROWS - 1 > wave_first;   // (wave-uniform) some query of the wave does not see the whole tile
      float sc[2][4], mb = m_;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = d4[blk][i] * qk_scale;
          sc[blk][i] = (!diagonal || tile0 + 16 * blk + 4 * rsel + i <= limit) ? x : -INFINITY;   // by the row index: x may be NaN
          mb = fmaxf(mb, sc[blk][i]);
        }
      mb = fmaxf(mb, __shfl_xor(mb, 16));
      mb = fmaxf(mb, __shfl_xor(mb, 32));
      const float mref = mb == -INFINITY ? 0.f : mb;   // (row 0 is visible to every query: finite from the first tile on)
      const float corr = exp2f(m_ - mref);
      m_ = mb;
      l_ *= corr;
      half8_t pb;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = exp2f(sc[blk][i] - mref);   // (0 for a masked row)
          l_ += e;
          pb[4 * blk + i] = (half_t)e;
        }
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        const half8_t va = *(const half8_t*)(v_lds + (16 * db + qi) * PA_VSTRIDE + ((rsel ^ (db & 3)) * 4));
        oacc[db] = mfma16(va, pb, oacc[db] * corr);
      }
    }
  }
  // the four lanes of a query add up their sums; one division, one rounding
  l_ += __shfl_xor(l_, 16);
  l_ += __shfl_xor(l_, 32);
#pragma unroll
  for (int db = 0; db < 8; ++db) {
    half4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (half_t)(oacc[db][i] / l_);
    *(half4_t*)(o_lds[wave] + qi * D + 16 * db + 4 * rsel) = o;
  }
  __syncthreads();
  half_t* op = out + ((size_t)b * T + tw0) * nh * D + (size_t)h * D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * r + rsel, piece = qi;
    if (tw0 + row < T) *(half8_t*)(op + (size_t)row * nh * D + piece * 8) = *(const half8_t*)(o_lds[wave] + row * D + piece * 8);
  }
}

static int prefill_attention_check(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len) {
  if (batch <= 0 || tokens <= 0 || n_heads <= 0 || n_kv_heads <= 0 || cache_len <= 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "prefill attention: batch, tokens, n_heads, n_kv_heads and cache_len must be positive");
  if (tokens > cache_len)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "prefill attention: more tokens than the cache has rows (tokens > cache_len)");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "prefill attention: head_dim must be 128");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "prefill attention: n_heads must be a multiple of n_kv_heads");
  if (n_heads > 65535 || batch > 65535)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "prefill attention: n_heads and batch are grid dimensions and must not exceed 65535");
  return QUICK_OK;
}

static int prefill_attention_launch(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                    int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, void* hip_stream) {
  const int rc = prefill_attention_check(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len);
  if (rc != QUICK_OK) return rc;
  if (!q || !k_cache || !v_cache || !pos0 || !out) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "prefill attention: a null pointer");
  const dim3 grid((unsigned)((tokens + PA_QROWS - 1) / PA_QROWS), (unsigned)n_heads, (unsigned)batch);
  hipLaunchKernelGGL(PA_KERNEL, grid, dim3(PA_WAVES * 64), 0, (hipStream_t)hip_stream, (const half_t*)q,
                     (const half_t*)k_cache, (const half_t*)v_cache, (const long*)pos0, (half_t*)out, tokens, n_heads, n_kv_heads,
                     cache_len, scale);
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "prefill attention: the launch failed");
  return QUICK_OK;
}

}  // namespace quick_amd

