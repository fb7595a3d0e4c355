// Attention over a PAGED KV cache (fp16): RoPE + pool write, the fused decode step and the MFMA prefill attention over pools
// [num_pages, nkv, P, 128] addressed through a block table.  A unit of its own beside decode_ops.hip, prefill_attention.hpp, kv_fp8.hip
// and attention_window.hip: those kernels are not touched and compile to the code they were.
//
// Layout.  A page holds P consecutive positions of ONE sequence, for all KV heads; P is 32, 64, 128 or 256.  table[b][i] (int32,
// [batch, max_pages]) names the pool page of positions i P .. i P + P - 1 of sequence b: position j of sequence b, KV head h, lives at
// pool row (table[b][j / P], h, j % P).  P is a power of two: the kernels take its log2 and map with a shift and a mask.  P is a whole
// multiple of the decode sweep's 16-row chunk and of the prefill kernel's 32-row tile, both aligned to their own size, so a chunk or
// a tile never straddles a page: the table is read ONCE per chunk or tile, on a wave-uniform index, and every row of the chunk is that
// page's base plus its row -- no division and no table read per lane.
// Positions are bounded by NPOS = min(table_rows, max_pages * P): the rows of the cos / sin tables and the columns of the block table.
//
// Never read.  Every request is clamped, as a LOGICAL position, to [0, last written position] before it is mapped: table columns behind
// the last written position's page are never read and may hold anything (-1), and pool pages named by no needed column are never read
// and may hold NaN keys and +-Inf values.  Rows of a needed page behind the last written position are not requested either.
// A needed table entry outside 0 .. num_pages - 1: a WRITE drops that row (the write launch, the decode launch's append); a READ never
// leaves the pool -- the decode sweep pulls the id inside the pool, the prefill staging takes zeros in place of that tile (a zero weight
// times a pulled-in page's Inf would be NaN inside the MFMA and reach the queries of the wave that do not attend the tile: right-padded
// rows of a ragged chunk lie in pages nobody reserved).  No address leaves the pool and no other sequence's page is written, whatever the
// table holds; that sequence's output is unspecified.  The same page id may stand in several sequences' rows (a shared prefix): reads
// need nothing for that, keeping writers apart is the caller's business.
//
// Rounding points are those of the kernels these were made from: rope_kv_prefill_kernel (each product rounded to fp16, then the sum),
// decode_rope_attention_win_kernel = the grouped MFMA sweep (fp32 scores from four 32-product MFMAs, times scale * log2 e in fp32; max,
// exp2, sum and P V in fp32 on the vector ALUs; one division and one rounding at the end) and prefill_attention.hpp (the same scores;
// P ROUNDED TO FP16 as the operand of the second MFMA product, the sum from the unrounded weights; one rescale per tile; one division,
// one rounding; out through LDS) -- the same operations in the same order, so the results are those kernels' bit for bit on the
// gathered linear cache.  No atomics, no workspace, no spinning.
#include <climits>
#include <cstdio>
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

namespace quick_amd {
namespace {

constexpr int D = 128;

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the value of lane g of each 16-lane row, to all 16 (g: a constant after unrolling)
__device__ __forceinline__ float row_bcast_p(float x, int g) {
#define QA_BC(G) case G: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x150 + G, 0xf, 0xf, false));
  switch (g) {
    QA_BC(0) QA_BC(1) QA_BC(2) QA_BC(3) QA_BC(4) QA_BC(5) QA_BC(6) QA_BC(7)
    default: return x;
  }
#undef QA_BC
}

// RoPE + pool write for T >= 1 tokens: rope_kv_prefill_kernel of decode_ops.hip (the same products, each rounded to fp16, the same sum:
// q_out and the stored rows are bit for bit that kernel's) with token t stored at pool row (table[b][(pos0 + t) / P], kvh, (pos0 + t) % P).
// NPOS bounds the positions.  SEQ: a sequence whose start lies outside 0 .. NPOS - T is skipped; the shared form pulls *pos0 inside.
// A token whose table entry names no page of the pool keeps its q_out row and stores no K / V row.
template <bool SEQ>
__global__ __launch_bounds__(64) void rope_kv_write_paged_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t,
                                                                 const half_t* __restrict__ sin_t, const long* __restrict__ pos0,
                                                                 half_t* __restrict__ q_out, half_t* __restrict__ k_pool,
                                                                 half_t* __restrict__ v_pool, const int* __restrict__ table, int T, int nh,
                                                                 int nkv, int num_pages, int psh, int max_pages, int NPOS) {
  const int bt = blockIdx.y, b = bt / T, t = bt % T, slot = blockIdx.x;
  long pb = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (pb < 0 || pb > NPOS - T) return;
  } else {
    pb = clampl(pb, 0, NPOS - T);   // (no address leaves the tables)
  }
  const long p = pb + t;
  const half_t* src = qkv + (size_t)bt * (nh + 2 * nkv) * D + (size_t)slot * D;
  const int i = threadIdx.x;
  half_t* dst;
  if (slot < nh) {
    dst = q_out + (((size_t)b * nh + slot) * T + t) * D;
  } else {
    const int pg = table[(size_t)b * max_pages + (int)(p >> psh)];   // (one read per workgroup: a workgroup is one token's slot)
    if (pg < 0 || pg >= num_pages) return;                           // a write outside the pool is dropped
    const int prow = (int)p & ((1 << psh) - 1);
    const int kvh = slot < nh + nkv ? slot - nh : slot - nh - nkv;
    dst = (slot < nh + nkv ? k_pool : v_pool) + ((((size_t)pg * nkv + kvh) << psh) + prow) * D;
  }
  if (slot < nh + nkv) {
    #pragma clang fp contract(off)  // (each product rounded to fp16 on its own: hipcc would fuse one into a v_fma_f16 with the add)
    const float x0 = (float)src[i], x1 = (float)src[i + D / 2];
    const float c0 = (float)cos_t[p * D + i], s0 = (float)sin_t[p * D + i];
    const float c1 = (float)cos_t[p * D + i + D / 2], s1 = (float)sin_t[p * D + i + D / 2];
    const half_t r0 = (half_t)((float)(half_t)(x0 * c0) + (float)(half_t)(-x1 * s0));
    const half_t r1 = (half_t)((float)(half_t)(x1 * c1) + (float)(half_t)(x0 * s1));
    dst[i] = r0;
    dst[i + D / 2] = r1;
  } else {
    dst[i] = src[i];
    dst[i + D / 2] = src[i + D / 2];
  }
}

// Fused decode step over the pool: decode_rope_attention_win_kernel with no window (the sweep runs over positions 0 .. p, this token is
// index pe = p and comes from registers) and the chunk's rows found through the table.  One workgroup per (sequence, KV head) serves
// all GROUP query heads from one sweep.  Requests are clamped to position pe - 1 (at pe == 0 to position 0, which is this token's own
// row: the lanes of that row take their values from registers and every other clamped lane is masked by its index).  The clamped
// positions of a 16-row chunk share one page -- that of min(chunk start, pe - 1) -- so the table is read once per chunk by the wave.
template <int GROUP, bool SEQ>
__global__ __launch_bounds__(256, 2) void decode_rope_attention_paged_kernel(
    const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t, const half_t* __restrict__ sin_t,
    const long* __restrict__ pos, half_t* __restrict__ k_pool, half_t* __restrict__ v_pool, half_t* __restrict__ out,
    const int* __restrict__ table, int nh, int nkv, int num_pages, int psh, int max_pages, int NPOS, float scale) {
  static_assert(GROUP >= 1 && GROUP <= 8, "query heads per KV head");
  __shared__ float part[4][GROUP][D + 2];  // per wave and query head: 128 output dims, running max, running sum
  const int b = blockIdx.y, kvh = blockIdx.x, hbase = kvh * GROUP;
  const int lane = threadIdx.x & 63, wave = uniform((int)(threadIdx.x >> 6));
  const int sub = lane & 15, rsel = lane >> 4;
  const half_t* row = qkv + (size_t)b * (nh + 2 * nkv) * D;
  const int* trow = table + (size_t)b * max_pages;
  const int pmask = (1 << psh) - 1;
  const half_t* kp = k_pool + rsel * 8;   // + page base + row * D + 32 s
  const half_t* vp = v_pool + sub * 8;    // + page base + row * D
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
    if (pl < 0 || pl >= NPOS) return;  // a skipped sequence: nothing requested from the pools, nothing written
  }
  const int p = uniform((int)clampl(pl, 0, NPOS - 1));   // (shared form: a value outside is pulled inside)
  const int pe = p;                        // this token's index in the sweep; n = pe + 1 indices
  const int plast = max(pe - 1, 0);
  // first element of (page, kvh, row 0) for the page of position j (wave-uniform); an id outside the pool is pulled inside
  auto page_base = [&](int j) __attribute__((always_inline)) {
    const int pg = uniform(min(max(trow[j >> psh], 0), num_pages - 1));
    return (((size_t)pg * nkv + kvh) << psh) * D;
  };

  auto request = [&](half8_t (&ka)[4], half8_t (&va)[4], int tb) __attribute__((always_inline)) {
    const size_t base = page_base(min(tb, plast));   // (the page of every clamped row of this chunk)
    const int kr = min(tb + sub, plast) & pmask;
#pragma unroll
    for (int s = 0; s < 4; ++s) ka[s] = *(const half8_t*)(kp + base + (size_t)kr * D + 32 * s);
#pragma unroll
    for (int i = 0; i < 4; ++i) va[i] = *(const half8_t*)(vp + base + (size_t)(min(tb + 4 * rsel + i, plast) & pmask) * D);
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
    // append at this token's page and row (requested by nobody, except at pe == 0: see above); dropped where the table names no page
    const int pg_w = uniform(trow[p >> psh]);
    if (wave == 0 && pg_w >= 0 && pg_w < num_pages) {
      const size_t wrow = ((((size_t)pg_w * nkv + kvh) << psh) + (p & pmask)) * D;
      if (sub == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) *(half8_t*)(k_pool + wrow + 32 * s + 8 * rsel) = kh[s];
      }
      if (rsel == 0) *(half8_t*)(v_pool + wrow + sub * 8) = vn;
    }
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
      const float cg = row_bcast_p(corr, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= cg;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float pg[GROUP];
#pragma unroll
      for (int g = 0; g < GROUP; ++g) pg[g] = row_bcast_p(sc[i], g);   // (DPP: every lane takes part, also for masked rows)
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
    const float mg = row_bcast_p(m_, g), lg = row_bcast_p(l_, g);   // this row quarter's state of head g, in all of its 16 lanes
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

// MFMA prefill attention over the pool: prefill_attention.hpp (tiling, LDS images, online softmax, rounding points, way out) with each
// 32-row tile fetched through the table.  Tiles are aligned to multiples of 32 positions and tile0 <= last for every tile of the loop, so
// the clamped positions min(tile0 + r, last) of a tile share the page of tile0: one workgroup-uniform table read per tile.  A tile whose
// entry names no page of the pool is staged as zeros and requests nothing.  The kernel never writes the pool.
constexpr int PP_QROWS = 64;    // query rows per workgroup (16 per wave)
constexpr int PP_KVROWS = 32;   // positions per tile
constexpr int PP_WAVES = 4;
constexpr int PP_VSTRIDE = 20;  // dwords per row of the transposed V image: 16 key pairs + 4 of padding

template <bool SEQ>
__global__ __launch_bounds__(PP_WAVES * 64) void prefill_attention_paged_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k_pool,
                                                                                const half_t* __restrict__ v_pool, const long* __restrict__ pos0,
                                                                                half_t* __restrict__ out, const int* __restrict__ table, int T,
                                                                                int nh, int nkv, int num_pages, int psh, int max_pages, int NPOS,
                                                                                float scale) {
  __shared__ __attribute__((aligned(16))) half_t k_lds[PP_KVROWS * D];        // [key][16-byte piece ^ (key & 15)]
  __shared__ __attribute__((aligned(16))) uint32_t v_lds[D * PP_VSTRIDE];     // [dim][key pair], quads of pairs XOR-ed with (dim / 16) & 3
  __shared__ __attribute__((aligned(16))) half_t o_lds[PP_WAVES][16 * D];     // the waves' output rows on their way out
  const int b = blockIdx.z, h = blockIdx.y, kvh = h / (nh / nkv), t0 = blockIdx.x * PP_QROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int qi = lane & 15, rsel = lane >> 4;
  const long praw = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (praw < 0 || praw > NPOS - T) return;   // (workgroup-uniform)
  }
  const int p0 = uniform((int)clampl(praw, 0, NPOS - T));   // (shared form: a value outside is pulled inside)
  const int last = p0 + T - 1;                                   // the last written position: staging reads nothing behind it
  const int tw0 = t0 + 16 * wave;                                // this wave's first query
  const bool wave_active = tw0 < T;
  const int wave_first = p0 + tw0, wave_last = p0 + min(tw0 + 15, T - 1);   // the causal limits of its first and last query
  const int tq = min(tw0 + qi, T - 1);                           // (rows behind T: the last query again, not stored)
  const int limit = p0 + tq;                                     // this lane's query attends positions 0 .. limit
  const int ntiles = (p0 + min(t0 + PP_QROWS - 1, T - 1)) / PP_KVROWS + 1;

  const half_t* qp = q + (((size_t)b * nh + h) * T + tq) * D + 8 * rsel;
  half8_t qb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qb[s] = *(const half8_t*)(qp + 32 * s);

  // staging: thread (row pair pi = tid / 16, piece c = tid % 16).  K positions pi and 16 + pi of the tile; V the two positions of key-slot
  // pair pi, neighbours in position and so in the page
  const int pi = tid >> 4, c = tid & 15;
  const int vrow = (pi & 2 ? 16 : 0) + 4 * (pi >> 2) + 2 * (pi & 1);
  const int* trow = table + (size_t)b * max_pages;
  const int pmask = (1 << psh) - 1;
  const half_t* kp = k_pool + c * 8;
  const half_t* vp = v_pool + c * 8;
  half8_t kreg[2], vreg[2];
  auto request = [&](int tile0) __attribute__((always_inline)) {
    const int pg = uniform(trow[min(tile0, last) >> psh]);
    if (pg >= 0 && pg < num_pages) {   // (workgroup-uniform)
      const size_t base = (((size_t)pg * nkv + kvh) << psh) * D;
      kreg[0] = *(const half8_t*)(kp + base + (size_t)(min(tile0 + pi, last) & pmask) * D);
      kreg[1] = *(const half8_t*)(kp + base + (size_t)(min(tile0 + 16 + pi, last) & pmask) * D);
      vreg[0] = *(const half8_t*)(vp + base + (size_t)(min(tile0 + vrow, last) & pmask) * D);
      vreg[1] = *(const half8_t*)(vp + base + (size_t)(min(tile0 + vrow + 1, last) & pmask) * D);
    } else {
      const half8_t zero = {};
      kreg[0] = kreg[1] = vreg[0] = vreg[1] = zero;
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
    *(half8_t*)(k_lds + pi * D + ((c ^ pi) * 8)) = kreg[0];             // (rows pi and 16 + pi: the same row & 15)
    *(half8_t*)(k_lds + (16 + pi) * D + ((c ^ pi) * 8)) = kreg[1];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = c * 8 + e;
      v_lds[d * PP_VSTRIDE + (((pi >> 2) ^ ((d >> 4) & 3)) * 4) + (pi & 3)] = as_u32(half2_t{vreg[0][e], vreg[1][e]});
    }
  };

  const float qk_scale = scale * 1.44269504088896f;   // scores in the log2 domain
  float m_ = -INFINITY, l_ = 0.f;                     // of query qi: the max over all rows so far, the sum over this lane's rows
  floatx4 oacc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) oacc[db] = floatx4{0.f, 0.f, 0.f, 0.f};

  request(0);
  for (int it = 0; it < ntiles; ++it) {
    const int tile0 = it * PP_KVROWS;
    __syncthreads();   // the previous tile has been read by everyone
    stage();
    __syncthreads();
    if (it + 1 < ntiles) request(tile0 + PP_KVROWS);
    if (wave_active && tile0 <= wave_last) {   // (wave-uniform; else the tile lies wholly behind this wave's last query)
      floatx4 d4[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8_t ka = *(const half8_t*)(k_lds + (16 * blk + qi) * D + (((4 * s + rsel) ^ qi) * 8));
          d4[blk] = mfma16(ka, qb[s], d4[blk]);
        }
      const bool diagonal = tile0 + PP_KVROWS - 1 > wave_first;   // (wave-uniform) some query of the wave does not see the whole tile
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
      const float mref = mb == -INFINITY ? 0.f : mb;   // (position 0 is visible to every query: finite from the first tile on)
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
        const half8_t va = *(const half8_t*)(v_lds + (16 * db + qi) * PP_VSTRIDE + ((rsel ^ (db & 3)) * 4));
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

// The shape rules of the three launches, in the order of the header's table.  The decode launch serves a KV head's whole group (1, 2, 4
// or 8 heads).
enum class Paged { WRITE, DECODE, PREFILL };

int page_shift(int page_size) {
  switch (page_size) {
    case 32: return 5;
    case 64: return 6;
    case 128: return 7;
    case 256: return 8;
    default: return -1;
  }
}

int paged_check(Paged kind, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int num_pages, int page_size, int max_pages,
                int table_rows) {
  if (batch <= 0 || tokens <= 0 || n_heads <= 0 || n_kv_heads <= 0 || num_pages <= 0 || page_size <= 0 || max_pages <= 0 || table_rows <= 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT,
                          "paged attention: batch, tokens, n_heads, n_kv_heads, num_pages, page_size, max_pages and table_rows must be positive");
  if (page_shift(page_size) < 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged attention: page_size must be 32, 64, 128 or 256");
  if (tokens > table_rows)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged attention: more tokens than there are positions (tokens > table_rows)");
  if ((long)max_pages * page_size < tokens)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT,
                          "paged attention: more tokens than a block table row can map (max_pages * page_size < tokens)");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "paged attention: head_dim must be 128");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "paged attention: n_heads must be a multiple of n_kv_heads");
  if (kind == Paged::DECODE) {
    const int group = n_heads / n_kv_heads;
    if (group != 1 && group != 2 && group != 4 && group != 8)
      return set_last_error(QUICK_ERR_UNSUPPORTED, "paged attention: 1, 2, 4 or 8 query heads per KV head in the decode launch");
  }
  if (kind == Paged::WRITE ? (long)batch * tokens > 65535 : (batch > 65535 || n_heads > 65535))
    return set_last_error(QUICK_ERR_UNSUPPORTED,
                          "paged attention: a grid dimension (write: batch * tokens; attention: batch, n_heads) must not exceed 65535");
  return QUICK_OK;
}

// the exclusive bound on positions: the rows of the cos / sin tables and the positions a block table row can map
int position_bound(int page_size, int max_pages, int table_rows) {
  const long mapped = (long)max_pages * page_size;
  return mapped < table_rows ? (int)mapped : table_rows;
}

}  // namespace
}  // namespace quick_amd

using namespace quick_amd;

extern "C" {

int quick_rope_kv_write_paged_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_pool,
                                  void* v_pool, const void* block_table, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                                  int num_pages, int page_size, int max_pages, int table_rows, int per_sequence, void* hip_stream) {
  const int rc = paged_check(Paged::WRITE, batch, tokens, n_heads, n_kv_heads, head_dim, num_pages, page_size, max_pages, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!qkv || !cos_table || !sin_table || !pos0 || !q_out || !k_pool || !v_pool || !block_table)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged rope_kv_write: a null pointer");
  const dim3 grid((unsigned)(n_heads + 2 * n_kv_heads), (unsigned)(batch * tokens));
#define QA_WRITE(SEQ)                                                                                                              \
  hipLaunchKernelGGL(rope_kv_write_paged_kernel<SEQ>, grid, dim3(64), 0, (hipStream_t)hip_stream, (const half_t*)qkv,               \
                     (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos0, (half_t*)q_out, (half_t*)k_pool,        \
                     (half_t*)v_pool, (const int*)block_table, tokens, n_heads, n_kv_heads, num_pages, page_shift(page_size),       \
                     max_pages, position_bound(page_size, max_pages, table_rows))
  if (per_sequence) QA_WRITE(true);
  else QA_WRITE(false);
#undef QA_WRITE
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "paged rope_kv_write: the launch failed");
  return QUICK_OK;
}

int quick_decode_rope_attention_paged_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_pool,
                                          void* v_pool, void* out, const void* block_table, int batch, int n_heads, int n_kv_heads,
                                          int head_dim, int num_pages, int page_size, int max_pages, int table_rows, float scale,
                                          int per_sequence, void* hip_stream) {
  const int rc = paged_check(Paged::DECODE, batch, 1, n_heads, n_kv_heads, head_dim, num_pages, page_size, max_pages, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!qkv || !cos_table || !sin_table || !pos || !k_pool || !v_pool || !out || !block_table)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged decode attention: a null pointer");
  const dim3 grid((unsigned)n_kv_heads, (unsigned)batch);
#define QA_DEC(GROUP, SEQ)                                                                                                          \
  hipLaunchKernelGGL((decode_rope_attention_paged_kernel<GROUP, SEQ>), grid, dim3(256), 0, (hipStream_t)hip_stream,                 \
                     (const half_t*)qkv, (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos, (half_t*)k_pool,     \
                     (half_t*)v_pool, (half_t*)out, (const int*)block_table, n_heads, n_kv_heads, num_pages, page_shift(page_size), \
                     max_pages, position_bound(page_size, max_pages, table_rows), scale)
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
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "paged decode attention: the launch failed");
  return QUICK_OK;
}

int quick_prefill_attention_paged_f16(const void* q, const void* k_pool, const void* v_pool, const void* pos0, void* out,
                                      const void* block_table, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                                      int num_pages, int page_size, int max_pages, int table_rows, float scale, int per_sequence,
                                      void* hip_stream) {
  const int rc = paged_check(Paged::PREFILL, batch, tokens, n_heads, n_kv_heads, head_dim, num_pages, page_size, max_pages, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!q || !k_pool || !v_pool || !pos0 || !out || !block_table)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged prefill attention: a null pointer");
  const dim3 grid((unsigned)((tokens + PP_QROWS - 1) / PP_QROWS), (unsigned)n_heads, (unsigned)batch);
#define QA_PF(SEQ)                                                                                                                  \
  hipLaunchKernelGGL(prefill_attention_paged_kernel<SEQ>, grid, dim3(PP_WAVES * 64), 0, (hipStream_t)hip_stream, (const half_t*)q,   \
                     (const half_t*)k_pool, (const half_t*)v_pool, (const long*)pos0, (half_t*)out, (const int*)block_table, tokens, \
                     n_heads, n_kv_heads, num_pages, page_shift(page_size), max_pages,                                              \
                     position_bound(page_size, max_pages, table_rows), scale)
  if (per_sequence) QA_PF(true);
  else QA_PF(false);
#undef QA_PF
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "paged prefill attention: the launch failed");
  return QUICK_OK;
}

int quick_attention_paged_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int num_pages, int page_size,
                                   int max_pages, int table_rows, char* text, size_t text_bytes) {
  const bool decode = tokens == 1;
  const int rc = paged_check(decode ? Paged::DECODE : Paged::PREFILL, batch, tokens, n_heads, n_kv_heads, head_dim, num_pages, page_size,
                             max_pages, table_rows);
  if (rc != QUICK_OK) return rc;
  if (!text || text_bytes == 0) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "paged attention: no room for the description");
  if (decode)
    snprintf(text, text_bytes, "decode-paged-mfma heads=%d waves=4 set_rows=64 page_size=%d max_pages=%d grid=%dx%d", n_heads / n_kv_heads,
             page_size, max_pages, n_kv_heads, batch);
  else
    snprintf(text, text_bytes, "prefill-paged-mfma q_rows=%d kv_rows=%d waves=%d page_size=%d max_pages=%d grid=%dx%dx%d", PP_QROWS,
             PP_KVROWS, PP_WAVES, page_size, max_pages, (tokens + PP_QROWS - 1) / PP_QROWS, n_heads, batch);
  return QUICK_OK;
}

}  // extern "C"
