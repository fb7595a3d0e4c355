// Sliding-window attention over a RING KV cache (fp16): RoPE + cache write, the fused decode step and the MFMA prefill attention over
// caches [B, nkv, R, 128].  A unit of its own beside decode_ops.hip, prefill_attention.hpp and kv_fp8.hip: those kernels are not touched
// and compile to the code they were (prefill_attention.hpp records what templating one of them cost).
//
// Window.  The query at position p attends positions max(0, p - W + 1) .. p.  Keys keep the RoPE of their own ABSOLUTE position: nothing
// is re-labelled when the window moves (the reference's roll_kv_n_steps shifts start_pos and so re-labels cached keys; not copied).
// Ring.    Position j lives in cache row j % R, W <= R.  A sweep walks LOGICAL positions lo .. p: lo % R is reduced once per workgroup
// and every further row is lo % R + (j - lo), minus R where that passes the end -- a compare and a subtract, no division per row.  That
// needs j - lo < R for every requested j, which the launchers guarantee: a decode step requests W <= R positions; a prefill chunk of T
// tokens requests at most W + T - 1 positions and is refused unless W + T - 1 <= R or the ring can never wrap (R >= table_rows, the
// exclusive bound on positions: then j % R == j).
// Ring rule.  A chunk is written before it is attended and overwrites the rows of positions <= pos0 + T - 1 - R.  The oldest position
// any query of the chunk attends is pos0 - W + 1; with W + T - 1 <= R it is > pos0 + T - 1 - R: no attended row has been overwritten.
//
// Never read.  Every request is clamped, as a LOGICAL position, to [lo of the launch's (prefill: the workgroup's) first query, the last
// written position] before it is mapped to a row: rows of the ring that hold no position of that span -- rows not yet written before the
// first wrap, stale rows of positions in front of the window after it -- may hold NaN keys and +-Inf values.  Positions inside the span
// but outside a given query's own window are requested (they are finite) and masked by the row INDEX before the max and the exp, as the
// causal diagonal is.  The prefill kernel never writes a cache; the decode kernel writes row *pos % R and nothing else.
//
// Rounding points are those of the kernels these were made from: decode_rope_attention_gqa_mfma_kernel (fp32 scores from four 32-product
// MFMAs, times scale * log2 e in fp32; max, exp2, sum and P V in fp32 on the vector ALUs; one division and one rounding at the end) and
// prefill_attention.hpp (the same scores; P ROUNDED TO FP16 as the operand of the second MFMA product, the sum from the unrounded weights;
// one rescale per tile; one division, one rounding; out through LDS).  No atomics, no workspace, no spinning.
#include <climits>
#include <cstdio>
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

namespace quick_amd {
namespace {

constexpr int D = 128;

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the value of lane g of each 16-lane row, to all 16 (g: a constant after unrolling)
__device__ __forceinline__ float row_bcast_w(float x, int g) {
#define QA_BC(G) case G: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x150 + G, 0xf, 0xf, false));
  switch (g) {
    QA_BC(0) QA_BC(1) QA_BC(2) QA_BC(3) QA_BC(4) QA_BC(5) QA_BC(6) QA_BC(7)
    default: return x;
  }
#undef QA_BC
}

// RoPE + ring write for T >= 1 tokens: rope_kv_prefill_kernel of decode_ops.hip (the same products, each rounded to fp16, the same sum:
// q_out and the stored rows are bit for bit that kernel's) with token t stored at row (pos0 + t) % R.  NP = table_rows bounds the
// positions.  SEQ: a sequence whose start lies outside 0 .. NP - T is skipped; the shared form pulls *pos0 inside.
template <bool SEQ>
__global__ __launch_bounds__(64) void rope_kv_write_win_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t,
                                                               const half_t* __restrict__ sin_t, const long* __restrict__ pos0,
                                                               half_t* __restrict__ q_out, half_t* __restrict__ k_cache,
                                                               half_t* __restrict__ v_cache, int T, int nh, int nkv, int R, int NP) {
  const int bt = blockIdx.y, b = bt / T, t = bt % T, slot = blockIdx.x;
  long pb = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (pb < 0 || pb > NP - T) return;
  } else {
    pb = clampl(pb, 0, NP - T);   // (no address leaves the tables)
  }
  const long p = pb + t;
  const int prow = (int)(p % R);   // (one reduction per workgroup: a workgroup is one token's slot)
  const half_t* src = qkv + (size_t)bt * (nh + 2 * nkv) * D + (size_t)slot * D;
  const int i = threadIdx.x;
  if (slot < nh + nkv) {
    #pragma clang fp contract(off)  // (each product rounded to fp16 on its own: hipcc would fuse one into a v_fma_f16 with the add)
    const float x0 = (float)src[i], x1 = (float)src[i + D / 2];
    const float c0 = (float)cos_t[p * D + i], s0 = (float)sin_t[p * D + i];
    const float c1 = (float)cos_t[p * D + i + D / 2], s1 = (float)sin_t[p * D + i + D / 2];
    const half_t r0 = (half_t)((float)(half_t)(x0 * c0) + (float)(half_t)(-x1 * s0));
    const half_t r1 = (half_t)((float)(half_t)(x1 * c1) + (float)(half_t)(x0 * s1));
    half_t* dst = slot < nh ? q_out + (((size_t)b * nh + slot) * T + t) * D
                            : k_cache + (((size_t)b * nkv + (slot - nh)) * R + prow) * D;
    dst[i] = r0;
    dst[i + D / 2] = r1;
  } else {
    half_t* dst = v_cache + (((size_t)b * nkv + (slot - nh - nkv)) * R + prow) * D;
    dst[i] = src[i];
    dst[i + D / 2] = src[i + D / 2];
  }
}

// Fused decode step over the ring: decode_rope_attention_gqa_mfma_kernel (one 16-row chunk per register set) with the sweep running
// over INDICES 0 .. n - 1 of the window, index i = logical position lo + i = cache row ring(i); this token is index n - 1 = pe and comes
// from registers.  One workgroup per (sequence, KV head) serves all GROUP query heads from one sweep.  Requests are clamped to index
// pe - 1 (at pe == 0 to index 0, which is row *pos % R itself: the lanes of that row take their values from registers and every other
// clamped lane is masked by its index).
template <int GROUP, bool SEQ>
__global__ __launch_bounds__(256, 2) void decode_rope_attention_win_kernel(
    const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t, const half_t* __restrict__ sin_t,
    const long* __restrict__ pos, half_t* __restrict__ k_cache, half_t* __restrict__ v_cache, half_t* __restrict__ out,
    int nh, int nkv, int R, int W, int NP, float scale) {
  static_assert(GROUP >= 1 && GROUP <= 8, "query heads per KV head");
  __shared__ float part[4][GROUP][D + 2];  // per wave and query head: 128 output dims, running max, running sum
  const int b = blockIdx.y, kvh = blockIdx.x, hbase = kvh * GROUP;
  const int lane = threadIdx.x & 63, wave = uniform((int)(threadIdx.x >> 6));
  const int sub = lane & 15, rsel = lane >> 4;
  const half_t* row = qkv + (size_t)b * (nh + 2 * nkv) * D;
  half_t* krow = k_cache + ((size_t)b * nkv + kvh) * R * D;
  half_t* vrow = v_cache + ((size_t)b * nkv + kvh) * R * D;
  const half_t* kp = krow + rsel * 8;   // + row * D + 32 s
  const half_t* vp = vrow + sub * 8;    // + row * D
  half8_t qraw[4], kraw[4];
  const int hq = min(sub, GROUP - 1);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qraw[s] = *(const half8_t*)(row + (size_t)(hbase + hq) * D + 32 * s + 8 * rsel);
    kraw[s] = *(const half8_t*)(row + (size_t)(nh + kvh) * D + 32 * s + 8 * rsel);
  }
  const half8_t vn = *(const half8_t*)(row + (size_t)(nh + nkv + kvh) * D + sub * 8);

  const long pl = pos[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (pl < 0 || pl >= NP) return;  // a skipped sequence: nothing requested from the caches, nothing written
  }
  const int p = uniform((int)clampl(pl, 0, NP - 1));   // (shared form: a value outside is pulled inside)
  const int lo = max(p - W + 1, 0);        // the first attended position
  const int lo_r = uniform(lo % R);        // its row: the one reduction of this workgroup
  const int pe = p - lo;                   // this token's index in the sweep; n = pe + 1 <= W <= R indices
  const int plast = max(pe - 1, 0);
  auto ring = [&](int idx) __attribute__((always_inline)) {   // index -> cache row, idx < R
    const int r = lo_r + idx;
    return r >= R ? r - R : r;
  };
  const int p_r = ring(pe);

  auto request = [&](half8_t (&ka)[4], half8_t (&va)[4], int tb) __attribute__((always_inline)) {
    const int kr = ring(min(tb + sub, plast));
#pragma unroll
    for (int s = 0; s < 4; ++s) ka[s] = *(const half8_t*)(kp + (size_t)kr * D + 32 * s);
#pragma unroll
    for (int i = 0; i < 4; ++i) va[i] = *(const half8_t*)(vp + (size_t)ring(min(tb + 4 * rsel + i, plast)) * D);
  };
  half8_t kva[4], vva[4], kvb[4], vvb[4];
  constexpr int STEP = 64;
  int tb = wave * 16;   // first index of this wave's first chunk; a trip of the workgroup covers 64 indices
  request(kva, vva, tb);

  // rotate the q heads and the new k (dims 32 s + 8 rsel + j pair with the same j of k step s ^ 2) while the first rows are in flight
  half8_t qb[4], kh[4];
  {
    #pragma clang fp contract(off)  // (each product rounded to fp16 on its own: hipcc would fuse one into a v_fma_f16 with the add)
    half8_t cs[4], sn[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      cs[s] = *(const half8_t*)(cos_t + (size_t)p * D + 32 * s + 8 * rsel);
      sn[s] = *(const half8_t*)(sin_t + (size_t)p * D + 32 * s + 8 * rsel);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float sign = s < 2 ? -1.f : 1.f;  // rotate_half: dims 0..63 pair with -x[i+64], dims 64..127 with +x[i-64]
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = (float)cs[s][j], sj = (float)sn[s][j];
        qb[s][j] = sub < GROUP ? (half_t)((float)(half_t)((float)qraw[s][j] * c) + (float)(half_t)(sign * (float)qraw[s ^ 2][j] * sj)) : (half_t)0.f;
        kh[s][j] = (half_t)((float)(half_t)((float)kraw[s][j] * c) + (float)(half_t)(sign * (float)kraw[s ^ 2][j] * sj));
      }
    }
    if (wave == 0 && sub == 0) {  // append to the ring (row p_r is requested by nobody, except at pe == 0: see above)
#pragma unroll
      for (int s = 0; s < 4; ++s) *(half8_t*)(krow + (size_t)p_r * D + 32 * s + 8 * rsel) = kh[s];
    }
    if (wave == 0 && rsel == 0) *(half8_t*)(vrow + (size_t)p_r * D + sub * 8) = vn;
  }

  const float qk_scale = scale * 1.44269504088896f;   // scores in the log2 domain
  float m_ = -INFINITY, l_ = 0.f;   // lane (head sub, row quarter rsel): running max / sum of that head over this quarter's rows
  float acc[GROUP][8];
#pragma unroll
  for (int g = 0; g < GROUP; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;

  auto consume = [&](half8_t (&ka)[4], half8_t (&va)[4], int base) __attribute__((always_inline)) {
    float sc[4], mb = m_;
    if (base <= pe && pe < base + 16) {  // (wave-uniform) this chunk holds this token: from registers
      if (base + sub == pe) {
#pragma unroll
        for (int s = 0; s < 4; ++s) ka[s] = kh[s];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (base + 4 * rsel + i == pe) va[i] = vn;
    }
    floatx4 d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) d4 = mfma16(ka[s], qb[s], d4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = base + 4 * rsel + i <= pe ? d4[i] * qk_scale : -INFINITY;   // by the index: a clamped lane's score is not its own
      mb = fmaxf(mb, sc[i]);
    }
    const float mref = mb == -INFINITY ? 0.f : mb;
    const float corr = exp2f(m_ - mref);
    l_ *= corr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = exp2f(sc[i] - mref);   // (0 for a masked row)
      l_ += sc[i];
    }
    m_ = mb;
#pragma unroll
    for (int g = 0; g < GROUP; ++g) {
      const float cg = row_bcast_w(corr, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= cg;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float pg[GROUP];
#pragma unroll
      for (int g = 0; g < GROUP; ++g) pg[g] = row_bcast_w(sc[i], g);   // (DPP: every lane takes part, also for masked rows)
      if (base + 4 * rsel + i <= pe) {
        float vf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = (float)va[i][j];
#pragma unroll
        for (int g = 0; g < GROUP; ++g)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[g][j] += pg[g] * vf[j];
      }
    }
  };
  if (tb <= pe) {
    while (true) {  // wave-uniform trip counts; the requests for the next set leave before this one is consumed
      const bool more_b = tb + STEP <= pe;
      if (more_b) request(kvb, vvb, tb + STEP);
      consume(kva, vva, tb);
      if (!more_b) break;
      const bool more_a = tb + 2 * STEP <= pe;
      if (more_a) request(kva, vva, tb + 2 * STEP);
      consume(kvb, vvb, tb + STEP);
      if (!more_a) break;
      tb += 2 * STEP;
    }
  }
#pragma unroll
  for (int g = 0; g < GROUP; ++g) {
    const float mg = row_bcast_w(m_, g), lg = row_bcast_w(l_, g);   // this row quarter's state of head g, in all of its 16 lanes
    // merge the 4 row quarters of the wave, then the 4 waves through LDS
    float mw = fmaxf(mg, __shfl_xor(mg, 16));
    mw = fmaxf(mw, __shfl_xor(mw, 32));
    const float sc_ = exp2f(mg - (mw == -INFINITY ? 0.f : mw));
    float lw = lg * sc_;
    lw += __shfl_xor(lw, 16);
    lw += __shfl_xor(lw, 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[g][j] * sc_;
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (rsel == 0) part[wave][g][sub * 8 + j] = a;
    }
    if (lane == 0) {
      part[wave][g][D] = mw;
      part[wave][g][D + 1] = lw;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GROUP * D; i += 256) {
    const int g = i / D, dd = i % D;
    const float M = fmaxf(fmaxf(part[0][g][D], part[1][g][D]), fmaxf(part[2][g][D], part[3][g][D]));  // finite: this token is in somebody's sweep
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = exp2f(part[w][g][D] - M);
      num += part[w][g][dd] * f;
      den += part[w][g][D + 1] * f;
    }
    out[((size_t)b * nh + hbase + g) * D + dd] = (half_t)(num / den);
  }
}

// MFMA prefill attention (prefill_attention.hpp: tiling, LDS images, online softmax, rounding points, way out) with a window over the
// ring.  Tiles stay aligned to multiples of 32 LOGICAL positions.  New: the first tile of a workgroup is the one that holds the window
// start of its first query (wg_lo); staging clamps the logical position to [wg_lo, pos0 + T - 1] and maps it to its ring row; a second,
// lower diagonal (position > limit - W) is masked by the row index in the tiles that straddle it; a wave skips the tiles wholly in
// front of its first query's window as well as those behind its last query.  A query whose window starts behind the wave's first
// tiles sees only -inf there: its max stays -inf, the guard on mref keeps the rescale finite (0) and its accumulators stay 0.
constexpr int PW_QROWS = 64;    // query rows per workgroup (16 per wave)
constexpr int PW_KVROWS = 32;   // positions per tile
constexpr int PW_WAVES = 4;
constexpr int PW_VSTRIDE = 20;  // dwords per row of the transposed V image: 16 key pairs + 4 of padding

template <bool SEQ>
__global__ __launch_bounds__(PW_WAVES * 64) void prefill_attention_win_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k_cache,
                                                                              const half_t* __restrict__ v_cache, const long* __restrict__ pos0,
                                                                              half_t* __restrict__ out, int T, int nh, int nkv, int R, int W,
                                                                              int NP, float scale) {
  __shared__ __attribute__((aligned(16))) half_t k_lds[PW_KVROWS * D];        // [key][16-byte piece ^ (key & 15)]
  __shared__ __attribute__((aligned(16))) uint32_t v_lds[D * PW_VSTRIDE];     // [dim][key pair], quads of pairs XOR-ed with (dim / 16) & 3
  __shared__ __attribute__((aligned(16))) half_t o_lds[PW_WAVES][16 * D];     // the waves' output rows on their way out
  const int b = blockIdx.z, h = blockIdx.y, kvh = h / (nh / nkv), t0 = blockIdx.x * PW_QROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int qi = lane & 15, rsel = lane >> 4;
  const long praw = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (praw < 0 || praw > NP - T) return;   // (workgroup-uniform)
  }
  const int p0 = uniform((int)clampl(praw, 0, NP - T));   // (shared form: a value outside is pulled inside)
  const int last = p0 + T - 1;                                   // the last written position: staging reads nothing behind it
  const int wg_lo = max(p0 + t0 - W + 1, 0);                     // the window start of the workgroup's first query: nothing in front of it
  const int lo_r = uniform(wg_lo % R);                           // its row: the one reduction of this workgroup
  const int tw0 = t0 + 16 * wave;                                // this wave's first query
  const bool wave_active = tw0 < T;
  const int wave_first = p0 + tw0, wave_last = p0 + min(tw0 + 15, T - 1);   // the causal limits of its first and last query
  const int wave_lo = wave_first - W + 1, wave_lo_last = wave_last - W + 1; // the window starts of both (may be negative: no lower edge)
  const int tq = min(tw0 + qi, T - 1);                           // (rows behind T: the last query again, not stored)
  const int limit = p0 + tq;                                     // this lane's query attends positions limit - W + 1 .. limit
  const int lowlim = limit - W;                                  // ... that is, positions > lowlim
  const int it0 = wg_lo / PW_KVROWS;
  const int ntiles = (p0 + min(t0 + PW_QROWS - 1, T - 1)) / PW_KVROWS + 1;

  const half_t* qp = q + (((size_t)b * nh + h) * T + tq) * D + 8 * rsel;
  half8_t qb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qb[s] = *(const half8_t*)(qp + 32 * s);

  // staging: thread (row pair pi = tid / 16, piece c = tid % 16).  K positions pi and 16 + pi of the tile; V the two positions of key-slot
  // pair pi, neighbours in position (in the ring they may be the last row and row 0)
  const int pi = tid >> 4, c = tid & 15;
  const int vrow = (pi & 2 ? 16 : 0) + 4 * (pi >> 2) + 2 * (pi & 1);
  const half_t* kp = k_cache + ((size_t)b * nkv + kvh) * R * D + c * 8;
  const half_t* vp = v_cache + ((size_t)b * nkv + kvh) * R * D + c * 8;
  auto ring = [&](int j) __attribute__((always_inline)) {   // logical position -> cache row; clamped to the span, whose length is <= R
    const int r = lo_r + (min(max(j, wg_lo), last) - wg_lo);
    return r >= R ? r - R : r;
  };
  half8_t kreg[2], vreg[2];
  auto request = [&](int tile0) __attribute__((always_inline)) {
    kreg[0] = *(const half8_t*)(kp + (size_t)ring(tile0 + pi) * D);
    kreg[1] = *(const half8_t*)(kp + (size_t)ring(tile0 + 16 + pi) * D);
    vreg[0] = *(const half8_t*)(vp + (size_t)ring(tile0 + vrow) * D);
    vreg[1] = *(const half8_t*)(vp + (size_t)ring(tile0 + vrow + 1) * D);
  };
  auto stage = [&]() __attribute__((always_inline)) {
    *(half8_t*)(k_lds + pi * D + ((c ^ pi) * 8)) = kreg[0];             // (rows pi and 16 + pi: the same row & 15)
    *(half8_t*)(k_lds + (16 + pi) * D + ((c ^ pi) * 8)) = kreg[1];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = c * 8 + e;
      v_lds[d * PW_VSTRIDE + (((pi >> 2) ^ ((d >> 4) & 3)) * 4) + (pi & 3)] = as_u32(half2_t{vreg[0][e], vreg[1][e]});
    }
  };

  const float qk_scale = scale * 1.44269504088896f;   // scores in the log2 domain
  float m_ = -INFINITY, l_ = 0.f;                     // of query qi: the max over all rows so far, the sum over this lane's rows
  floatx4 oacc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) oacc[db] = floatx4{0.f, 0.f, 0.f, 0.f};

  request(it0 * PW_KVROWS);
  for (int it = it0; it < ntiles; ++it) {
    const int tile0 = it * PW_KVROWS;
    __syncthreads();   // the previous tile has been read by everyone
    stage();
    __syncthreads();
    if (it + 1 < ntiles) request(tile0 + PW_KVROWS);
    // (wave-uniform; else the tile lies wholly behind this wave's last query or wholly in front of its first query's window)
    if (wave_active && tile0 <= wave_last && tile0 + PW_KVROWS - 1 >= wave_lo) {
      floatx4 d4[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8_t ka = *(const half8_t*)(k_lds + (16 * blk + qi) * D + (((4 * s + rsel) ^ qi) * 8));
          d4[blk] = mfma16(ka, qb[s], d4[blk]);
        }
      const bool diagonal = tile0 + PW_KVROWS - 1 > wave_first;   // (wave-uniform) some query of the wave does not see the tile's end
      const bool lower = tile0 < wave_lo_last;                    // (wave-uniform) some query of the wave does not see the tile's start
      float sc[2][4], mb = m_;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = d4[blk][i] * qk_scale;
          const int j = tile0 + 16 * blk + 4 * rsel + i;
          sc[blk][i] = ((!diagonal || j <= limit) && (!lower || j > lowlim)) ? x : -INFINITY;   // by the row index
          mb = fmaxf(mb, sc[blk][i]);
        }
      mb = fmaxf(mb, __shfl_xor(mb, 16));
      mb = fmaxf(mb, __shfl_xor(mb, 32));
      const float mref = mb == -INFINITY ? 0.f : mb;   // (a query whose window starts behind this tile: nothing seen yet)
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
        const half8_t va = *(const half8_t*)(v_lds + (16 * db + qi) * PW_VSTRIDE + ((rsel ^ (db & 3)) * 4));
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
    const int orow = 4 * r + rsel, piece = qi;
    if (tw0 + orow < T) *(half8_t*)(op + (size_t)orow * nh * D + piece * 8) = *(const half8_t*)(o_lds[wave] + orow * D + piece * 8);
  }
}

// The shape rules of the three launches, in the order of the header's table.  The write has no window; the decode launch serves a KV
// head's whole group (1, 2, 4 or 8 heads).
enum class Win { WRITE, DECODE, PREFILL };

int win_check(Win kind, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows, int window, int table_rows) {
  if (batch <= 0 || tokens <= 0 || n_heads <= 0 || n_kv_heads <= 0 || ring_rows <= 0 || table_rows <= 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT,
                          "window attention: batch, tokens, n_heads, n_kv_heads, ring_rows and table_rows must be positive");
  if (kind != Win::WRITE) {
    if (window < 1) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window attention: window must be at least 1");
    if (window > ring_rows)
      return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window attention: the window does not fit the ring (window > ring_rows)");
  }
  if (tokens > ring_rows)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window attention: more tokens than the ring has rows (tokens > ring_rows)");
  if (tokens > table_rows)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window attention: more tokens than there are positions (tokens > table_rows)");
  if (kind != Win::WRITE && ring_rows < table_rows && (long)window + tokens - 1 > ring_rows)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT,
                          "window attention: a chunk would overwrite rows it attends (window + tokens - 1 > ring_rows on a ring that can "
                          "wrap, ring_rows < table_rows): feed fewer tokens at a time");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "window attention: head_dim must be 128");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "window attention: n_heads must be a multiple of n_kv_heads");
  if (kind == Win::DECODE) {
    const int group = n_heads / n_kv_heads;
    if (group != 1 && group != 2 && group != 4 && group != 8)
      return set_last_error(QUICK_ERR_UNSUPPORTED, "window attention: 1, 2, 4 or 8 query heads per KV head in the decode launch");
  }
  if (kind == Win::WRITE ? (long)batch * tokens > 65535 : (batch > 65535 || n_heads > 65535))
    return set_last_error(QUICK_ERR_UNSUPPORTED,
                          "window attention: a grid dimension (write: batch * tokens; attention: batch, n_heads) must not exceed 65535");
  return QUICK_OK;
}

}  // namespace
}  // namespace quick_amd

using namespace quick_amd;

extern "C" {

int quick_rope_kv_write_win_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_cache,
                                void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows,
                                int table_rows, int per_sequence, void* hip_stream) {
  const int rc = win_check(Win::WRITE, batch, tokens, n_heads, n_kv_heads, head_dim, ring_rows, -1, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!qkv || !cos_table || !sin_table || !pos0 || !q_out || !k_cache || !v_cache)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window rope_kv_write: a null pointer");
  const dim3 grid((unsigned)(n_heads + 2 * n_kv_heads), (unsigned)(batch * tokens));
#define QA_WRITE(SEQ)                                                                                                              \
  hipLaunchKernelGGL(rope_kv_write_win_kernel<SEQ>, grid, dim3(64), 0, (hipStream_t)hip_stream, (const half_t*)qkv,                 \
                     (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos0, (half_t*)q_out, (half_t*)k_cache,       \
                     (half_t*)v_cache, tokens, n_heads, n_kv_heads, ring_rows, table_rows)
  if (per_sequence) QA_WRITE(true);
  else QA_WRITE(false);
#undef QA_WRITE
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "window rope_kv_write: the launch failed");
  return QUICK_OK;
}

int quick_decode_rope_attention_win_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_cache,
                                        void* v_cache, void* out, int batch, int n_heads, int n_kv_heads, int head_dim, int ring_rows,
                                        int window, int table_rows, float scale, int per_sequence, void* hip_stream) {
  const int rc = win_check(Win::DECODE, batch, 1, n_heads, n_kv_heads, head_dim, ring_rows, window, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!qkv || !cos_table || !sin_table || !pos || !k_cache || !v_cache || !out)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window decode attention: a null pointer");
  const dim3 grid((unsigned)n_kv_heads, (unsigned)batch);
#define QA_DEC(GROUP, SEQ)                                                                                                          \
  hipLaunchKernelGGL((decode_rope_attention_win_kernel<GROUP, SEQ>), grid, dim3(256), 0, (hipStream_t)hip_stream,                \
                     (const half_t*)qkv, (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos, (half_t*)k_cache,    \
                     (half_t*)v_cache, (half_t*)out, n_heads, n_kv_heads, ring_rows, window, table_rows, scale)
#define QA_DEC2(GROUP)                     \
  do {                                     \
    if (per_sequence) QA_DEC(GROUP, true); \
    else QA_DEC(GROUP, false);             \
  } while (0)
  switch (n_heads / n_kv_heads) {
    case 1: QA_DEC2(1); break;
    case 2: QA_DEC2(2); break;
    case 4: QA_DEC2(4); break;
    default: QA_DEC2(8); break;
  }
#undef QA_DEC2
#undef QA_DEC
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "window decode attention: the launch failed");
  return QUICK_OK;
}

int quick_prefill_attention_win_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                    int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows, int window, int table_rows,
                                    float scale, int per_sequence, void* hip_stream) {
  const int rc = win_check(Win::PREFILL, batch, tokens, n_heads, n_kv_heads, head_dim, ring_rows, window, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!q || !k_cache || !v_cache || !pos0 || !out)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window prefill attention: a null pointer");
  const dim3 grid((unsigned)((tokens + PW_QROWS - 1) / PW_QROWS), (unsigned)n_heads, (unsigned)batch);
#define QA_PF(SEQ)                                                                                                                  \
  hipLaunchKernelGGL(prefill_attention_win_kernel<SEQ>, grid, dim3(PW_WAVES * 64), 0, (hipStream_t)hip_stream, (const half_t*)q,     \
                     (const half_t*)k_cache, (const half_t*)v_cache, (const long*)pos0, (half_t*)out, tokens, n_heads, n_kv_heads,   \
                     ring_rows, window, table_rows, scale)
  if (per_sequence) QA_PF(true);
  else QA_PF(false);
#undef QA_PF
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "window prefill attention: the launch failed");
  return QUICK_OK;
}

int quick_attention_win_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows, int window,
                                 int table_rows, char* text, size_t text_bytes) {
  const bool decode = tokens == 1;
  const int rc = win_check(decode ? Win::DECODE : Win::PREFILL, batch, tokens, n_heads, n_kv_heads, head_dim, ring_rows, window, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!text || text_bytes == 0) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "window attention: no room for the description");
  if (decode)
    snprintf(text, text_bytes, "decode-win-mfma heads=%d waves=4 set_rows=64 ring_rows=%d window=%d grid=%dx%d", n_heads / n_kv_heads,
             ring_rows, window, n_kv_heads, batch);
  else
    snprintf(text, text_bytes, "prefill-win-mfma q_rows=%d kv_rows=%d waves=%d ring_rows=%d window=%d grid=%dx%dx%d", PW_QROWS, PW_KVROWS,
             PW_WAVES, ring_rows, window, (tokens + PW_QROWS - 1) / PW_QROWS, n_heads, batch);
  return QUICK_OK;
}

}  // extern "C"
