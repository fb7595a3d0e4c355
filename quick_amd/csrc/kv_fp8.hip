// One-byte KV cache (OCP e4m3fn, never the fnuz encoding): RoPE + cache write, the fused decode step and the MFMA prefill attention over
// caches [B, nkv, L, 128] of bytes.  A unit of its own beside decode_ops.hip and prefill_attention.hpp: the fp16 kernels are not touched.
//
// Format.  One scale per cache (k_scale, v_scale: host floats, constants of a captured graph).  Stored byte = rne_e4m3(clamp(float(h) *
// inv, -448, 448)) with h the fp16 value the fp16 launch stores at that place (rotated K rounded to fp16 exactly as there, V copied) and
// inv = 1.0f / scale from the host; the clamp is explicit (no conversion mode is relied on) and lets NaN through.  Dequantised value =
// float(byte) * scale -- but no kernel forms it: k_scale rides in the fp32 score factor (scale * log2 e * k_scale) and v_scale in the one
// fp32 multiply at the final division.  Inside the sweeps a byte becomes its exact fp16 value (every e4m3 value is an fp16 value) and
// nothing else; the MFMA products keep fp16 operands.  Conversions are hipcc's own instructions (builtins), nothing sits in an asm statement.
//
// Poisoned rows.  Rows at or behind a sequence's position may hold any byte, the NaN codes 0x7F / 0xFF included: requests are clamped
// to the last valid row and scores / value sums are masked by the row INDEX, as in the fp16 kernels.  The per-sequence skip rule is
// theirs too.
#include <cmath>
#include <cstdio>
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

namespace quick_amd {
namespace {

constexpr int D = 128;

__device__ __forceinline__ float sat448(float x) {
  const float c = fminf(fmaxf(x, -448.f), 448.f);
  return x != x ? x : c;   // (fmaxf / fminf drop a NaN: it is put back)
}
// eight fp16 values -> eight e4m3 bytes (memory order), one fp32 multiply, the clamp, one rounding (to nearest even)
__device__ __forceinline__ u32x2 quant8(half8_t h, float inv) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = sat448((float)h[j] * inv);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}
// eight bytes -> their exact fp16 values (v_cvt_scalef32_pk_f16_fp8 at scale 1)
__device__ __forceinline__ half8_t bytes_to_half8(uint32_t lo, uint32_t hi) {
  const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.0f, false);
  const half2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.0f, true);
  const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.0f, false);
  const half2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.0f, true);
  return half8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// the value of lane g of each 16-lane row, to all 16 (g: a constant after unrolling)
__device__ __forceinline__ float row_bcast8(float x, int g) {
#define QA_BC(G) case G: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x150 + G, 0xf, 0xf, false));
  switch (g) {
    QA_BC(0) QA_BC(1) QA_BC(2) QA_BC(3) QA_BC(4) QA_BC(5) QA_BC(6) QA_BC(7)
    default: return x;
  }
#undef QA_BC
}

// RoPE + cache write for T >= 1 tokens: qkv [B * T, (nh + 2 nkv) * D] -> q_out [B, nh, T, D] in fp16, bit for bit what
// rope_kv_prefill_kernel writes (the same products, each rounded to fp16, the same sum), K and V rows as bytes.  Sixteen lanes per
// (token, head slot), eight dims each: a 16-byte store of q, an 8-byte store of K or V; a workgroup of 64 takes four slots.
template <bool SEQ>
__global__ __launch_bounds__(64) void rope_kv_write_fp8_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t,
                                                               const half_t* __restrict__ sin_t, const long* __restrict__ pos0,
                                                               half_t* __restrict__ q_out, uint8_t* __restrict__ k_cache,
                                                               uint8_t* __restrict__ v_cache, int T, int nh, int nkv, int L, float k_inv,
                                                               float v_inv) {
  const int bt = blockIdx.y, b = bt / T, t = bt % T, nslots = nh + 2 * nkv;
  const int sub = threadIdx.x & 15, slot_raw = blockIdx.x * 4 + (threadIdx.x >> 4);
  const int slot = min(slot_raw, nslots - 1);   // (lanes behind the last slot do its work again and store nothing)
  const long pb = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (pb < 0 || pb > L - T) return;   // a skipped sequence (workgroup-uniform)
  }
  const long p = pb + t;
  const half8_t x = *(const half8_t*)(qkv + (size_t)bt * nslots * D + (size_t)slot * D + sub * 8);
  half8_t r;
  {
    #pragma clang fp contract(off)  // (each product rounded to fp16 on its own)
    const half8_t c = *(const half8_t*)(cos_t + (size_t)p * D + sub * 8), sn = *(const half8_t*)(sin_t + (size_t)p * D + sub * 8);
    const float sign = sub < 8 ? -1.f : 1.f;  // rotate_half: dims 0..63 pair with -x[i+64], dims 64..127 with +x[i-64]
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xj = (float)x[j];
      const float partner = __shfl_xor(xj, 8);  // lane sub ^ 8 of the same slot holds the paired dims
      r[j] = (half_t)((float)(half_t)(xj * (float)c[j]) + (float)(half_t)(sign * partner * (float)sn[j]));
    }
  }
  if (slot_raw >= nslots) return;
  if (slot < nh) {
    *(half8_t*)(q_out + (((size_t)b * nh + slot) * T + t) * D + sub * 8) = r;
  } else if (slot < nh + nkv) {
    *(u32x2*)(k_cache + (((size_t)b * nkv + (slot - nh)) * L + p) * D + sub * 8) = quant8(r, k_inv);
  } else {
    *(u32x2*)(v_cache + (((size_t)b * nkv + (slot - nh - nkv)) * L + p) * D + sub * 8) = quant8(x, v_inv);
  }
}

// Fused decode step over a byte cache: the grouped-query MFMA sweep of decode_ops.hip (one workgroup per (sequence, KV head) serves all
// GROUP query heads from ONE sweep of that head's rows) with 16 ELEMENTS per 16-byte request.
//   K  A operand of v_mfma_f32_16x16x32_f16, row = lane % 16.  Lane (row, quarter q) requests bytes 16 q .. + 15 and 64 + 16 q .. + 15 of
//      the row: two requests, four k steps -- step s takes dims 64 (s / 2) + 16 q + 8 (s % 2) .. + 7, and the rotated query heads (the B
//      operand) are gathered in the same order (the order of the 128 products inside a score is free).  Bytes -> fp16, exact.
//   V  on the vector ALUs as before, but eight lanes cover a row: lane (dims 16 (lane % 8) .. + 15, row parity (lane % 16) / 8, quarter q)
//      requests rows 4 q + 2 i + parity, i < 2, and sums 16 dims over half of the quarter's rows; the two halves meet at the end.
// Row *pos -- this token -- is part of the sweep with its QUANTISED K and V: the lanes that would request it take the new bytes from
// registers, so step p attends exactly what step p + 1 reads from the cache.  Rows behind it are masked by the row index.  Requests are
// clamped to row *pos - 1 (no request leaves before *pos is known, so the first-trip clamp of the flash kernel has no counterpart here).
// Software-pipelined: two register sets of one 16-row chunk per wave, the requests for trip t + 1 leave before trip t is consumed.  (Two
// chunks per set fit in 160 / 182 / 218 VGPRs at 1 / 2 / 4 heads and spill at 8: not instantiated, so no parameter for it.)
template <int GROUP, bool SEQ>
__global__ __launch_bounds__(256, 2) void decode_rope_attention_fp8_kernel(
    const half_t* __restrict__ qkv, const half_t* __restrict__ cos_t, const half_t* __restrict__ sin_t, const long* __restrict__ pos,
    uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache, half_t* __restrict__ out, int nh, int nkv, int L, float qk_scale,
    float k_inv, float v_inv, float v_scale) {
  static_assert(GROUP >= 1 && GROUP <= 8, "query heads per KV head");
  __shared__ float part[4][GROUP][D + 2];  // per wave and query head: 128 output dims, running max, running sum
  const int b = blockIdx.y, kvh = blockIdx.x, hbase = kvh * GROUP;
  const int lane = threadIdx.x & 63, wave = uniform((int)(threadIdx.x >> 6));
  const int sub = lane & 15, rsel = lane >> 4, vd = sub & 7, vr = sub >> 3;
  const half_t* row = qkv + (size_t)b * (nh + 2 * nkv) * D;
  uint8_t* krow = k_cache + ((size_t)b * nkv + kvh) * L * D;
  uint8_t* vrow = v_cache + ((size_t)b * nkv + kvh) * L * D;
  const uint8_t* kp = krow + 16 * rsel;   // + row * D + 64 r
  const uint8_t* vp = vrow + 16 * vd;     // + row * D
  half8_t qraw[4], kraw[4];
  const int hq = min(sub, GROUP - 1);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int off = 64 * (s >> 1) + 16 * rsel + 8 * (s & 1);
    qraw[s] = *(const half8_t*)(row + (size_t)(hbase + hq) * D + off);
    kraw[s] = *(const half8_t*)(row + (size_t)(nh + kvh) * D + off);
  }
  const half8_t vn0 = *(const half8_t*)(row + (size_t)(nh + nkv + kvh) * D + 16 * vd);
  const half8_t vn1 = *(const half8_t*)(row + (size_t)(nh + nkv + kvh) * D + 16 * vd + 8);

  auto request = [&](u32x4 (&ka)[2], u32x4 (&va)[2], int tb, int last) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 2; ++r) ka[r] = *(const u32x4*)(kp + (size_t)min(tb + sub, last) * D + 64 * r);
#pragma unroll
    for (int i = 0; i < 2; ++i) va[i] = *(const u32x4*)(vp + (size_t)min(tb + 4 * rsel + 2 * i + vr, last) * D);
  };
  u32x4 kva[2], vva[2], kvb[2], vvb[2];
  constexpr int STEP = 64;
  int tb = wave * 16;   // first row of this wave's first chunk; a trip of the workgroup covers 64 rows
  const long pl = pos[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (pl < 0 || pl >= L) return;  // a skipped sequence: nothing requested from the caches, nothing written
  }
  const int p = (int)pl;  // cache rows 0..p-1 come from memory, row p (this token) from registers
  const int plast = max(p - 1, 0);
  request(kva, vva, tb, plast);

  // rotate the q heads and the new k (dims of k step s pair with the same j of k step s ^ 2) while the first rows are in flight
  half8_t qb[4];
  u32x4 knew[2], vnew;
  {
    #pragma clang fp contract(off)  // (each product rounded to fp16 on its own)
    half8_t cs[4], sn[4], kh[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int off = 64 * (s >> 1) + 16 * rsel + 8 * (s & 1);
      cs[s] = *(const half8_t*)(cos_t + (size_t)p * D + off);
      sn[s] = *(const half8_t*)(sin_t + (size_t)p * D + off);
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
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const u32x2 a = quant8(kh[2 * r], k_inv), c = quant8(kh[2 * r + 1], k_inv);
      knew[r] = u32x4{a[0], a[1], c[0], c[1]};
    }
    const u32x2 a = quant8(vn0, v_inv), c = quant8(vn1, v_inv);
    vnew = u32x4{a[0], a[1], c[0], c[1]};
    if (wave == 0 && sub == 0) {  // append to the caches.  (Row p is requested by nobody, except at p == 0, where the clamp row is row 0 itself: harmless -- the
                                  // lanes of row p take their bytes from registers and every other clamped lane is masked by its row index.)
#pragma unroll
      for (int r = 0; r < 2; ++r) *(u32x4*)(krow + (size_t)p * D + 64 * r + 16 * rsel) = knew[r];
    }
    if (wave == 0 && rsel == 0 && sub < 8) *(u32x4*)(vrow + (size_t)p * D + 16 * sub) = vnew;
  }

  float m_ = -INFINITY, l_ = 0.f;   // lane (head sub, row quarter rsel): running max / sum of that head over this quarter's rows
  float acc[GROUP][16];
#pragma unroll
  for (int g = 0; g < GROUP; ++g)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[g][j] = 0.f;

  auto consume = [&](u32x4 (&ka)[2], u32x4 (&va)[2], int base) __attribute__((always_inline)) {
    float sc[4], mb = m_;
    if (base <= p && p < base + 16) {  // (wave-uniform) this chunk holds row p: its bytes come from registers
      if (base + sub == p) {
        ka[0] = knew[0];
        ka[1] = knew[1];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (base + 4 * rsel + 2 * i + vr == p) va[i] = vnew;
    }
    floatx4 d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      d4 = mfma16(bytes_to_half8(ka[r][0], ka[r][1]), qb[2 * r], d4);
      d4 = mfma16(bytes_to_half8(ka[r][2], ka[r][3]), qb[2 * r + 1], d4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = base + 4 * rsel + i <= p ? d4[i] * qk_scale : -INFINITY;   // by the row index: a row behind p may hold a NaN code
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
      const float cg = row_bcast8(corr, g);
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[g][j] *= cg;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float pg[GROUP];
#pragma unroll
      for (int g = 0; g < GROUP; ++g) {   // (DPP: every lane takes part, also for masked rows)
        const float even = row_bcast8(sc[2 * i], g), odd = row_bcast8(sc[2 * i + 1], g);
        pg[g] = vr ? odd : even;
      }
      if (base + 4 * rsel + 2 * i + vr <= p) {  // (a row behind the sequence holds anything: 0 * NaN would poison the sum)
        float vf[16];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)va[i][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)va[i][w], true);
          vf[4 * w] = lo[0];
          vf[4 * w + 1] = lo[1];
          vf[4 * w + 2] = hi[0];
          vf[4 * w + 3] = hi[1];
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[g][j] += pg[g] * vf[j];
      }
    }
  };
  if (tb <= p) {
    while (true) {  // wave-uniform trip counts; the requests for the next set leave before this one is consumed
      const bool more_b = tb + STEP <= p;
      if (more_b) request(kvb, vvb, tb + STEP, plast);
      consume(kva, vva, tb);
      if (!more_b) break;
      const bool more_a = tb + 2 * STEP <= p;
      if (more_a) request(kva, vva, tb + 2 * STEP, plast);
      consume(kvb, vvb, tb + STEP);
      if (!more_a) break;
      tb += 2 * STEP;
    }
  }
#pragma unroll
  for (int g = 0; g < GROUP; ++g) {
    const float mg = row_bcast8(m_, g), lg = row_bcast8(l_, g);   // this row quarter's state of head g, in all of its 16 lanes
    // merge the 4 row quarters of the wave, then the 4 waves through LDS
    float mw = fmaxf(mg, __shfl_xor(mg, 16));
    mw = fmaxf(mw, __shfl_xor(mw, 32));
    const float sc_ = exp2f(mg - (mw == -INFINITY ? 0.f : mw));
    float lw = lg * sc_;
    lw += __shfl_xor(lw, 16);
    lw += __shfl_xor(lw, 32);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float a = acc[g][j] * sc_;
      a += __shfl_xor(a, 8);    // the two row parities of the quarter
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (lane < 8) part[wave][g][lane * 16 + j] = a;
    }
    if (lane == 0) {
      part[wave][g][D] = mw;
      part[wave][g][D + 1] = lw;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GROUP * D; i += 256) {
    const int g = i / D, dd = i % D;
    const float M = fmaxf(fmaxf(part[0][g][D], part[1][g][D]), fmaxf(part[2][g][D], part[3][g][D]));  // finite: row p is in somebody's sweep
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = exp2f(part[w][g][D] - M);
      num += part[w][g][dd] * f;
      den += part[w][g][D + 1] * f;
    }
    out[((size_t)b * nh + hbase + g) * D + dd] = (half_t)(num / den * v_scale);
  }
}

// MFMA prefill attention (prefill_attention.hpp) over a byte cache.  The only change is in staging: every request carries half the bytes
// (8 instead of 16: the same thread -> (row, piece) mapping) and is converted to fp16 on the way into the same LDS images -- K rows
// swizzled, V transposed.  Tiling, masking, online softmax, rounding points and the way out are that kernel's; k_scale rides in the
// score factor and v_scale in the multiply at the final division.
constexpr int PF_QROWS = 64;    // query rows per workgroup (16 per wave)
constexpr int PF_KVROWS = 32;   // cache rows per tile
constexpr int PF_WAVES = 4;
constexpr int PF_VSTRIDE = 20;  // dwords per row of the transposed V image: 16 key pairs + 4 of padding

template <bool SEQ>
__global__ __launch_bounds__(PF_WAVES * 64) void prefill_attention_fp8_kernel(const half_t* __restrict__ q, const uint8_t* __restrict__ k_cache,
                                                                              const uint8_t* __restrict__ v_cache, const long* __restrict__ pos0,
                                                                              half_t* __restrict__ out, int T, int nh, int nkv, int L,
                                                                              float qk_scale, float v_scale) {
  __shared__ __attribute__((aligned(16))) half_t k_lds[PF_KVROWS * D];        // [key][16-byte piece ^ (key & 15)]
  __shared__ __attribute__((aligned(16))) uint32_t v_lds[D * PF_VSTRIDE];     // [dim][key pair], quads of pairs XOR-ed with (dim / 16) & 3
  __shared__ __attribute__((aligned(16))) half_t o_lds[PF_WAVES][16 * D];     // the waves' output rows on their way out
  const int b = blockIdx.z, h = blockIdx.y, kvh = h / (nh / nkv), t0 = blockIdx.x * PF_QROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int qi = lane & 15, rsel = lane >> 4;
  const long praw = pos0[SEQ ? b : 0];
  if constexpr (SEQ) {
    if (praw < 0 || praw > L - T) return;   // (workgroup-uniform)
  }
  const int p0 = uniform(min(max((int)praw, 0), L - T));          // (shared form: a value outside is pulled inside)
  const int last = p0 + T - 1;                                   // the last written cache row: staging reads nothing behind it
  const int tw0 = t0 + 16 * wave;                                // this wave's first query
  const bool wave_active = tw0 < T;
  const int wave_first = p0 + tw0, wave_last = p0 + min(tw0 + 15, T - 1);   // the causal limits of its first and last query
  const int tq = min(tw0 + qi, T - 1);                           // (rows behind T: the last query again, not stored)
  const int limit = p0 + tq;                                     // this lane's query attends cache rows 0 .. limit
  const int ntiles = (p0 + min(t0 + PF_QROWS - 1, T - 1)) / PF_KVROWS + 1;

  const half_t* qp = q + (((size_t)b * nh + h) * T + tq) * D + 8 * rsel;
  half8_t qb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qb[s] = *(const half8_t*)(qp + 32 * s);

  // staging: thread (row pair pi = tid / 16, piece c = tid % 16), 8 bytes = 8 dims per request.  K rows pi and 16 + pi; V the two rows of
  // key-slot pair pi, which are neighbours in the cache
  const int pi = tid >> 4, c = tid & 15;
  const int vrow = (pi & 2 ? 16 : 0) + 4 * (pi >> 2) + 2 * (pi & 1);
  const uint8_t* kp = k_cache + ((size_t)b * nkv + kvh) * L * D + c * 8;
  const uint8_t* vp = v_cache + ((size_t)b * nkv + kvh) * L * D + c * 8;
  u32x2 kreg[2], vreg[2];
  auto request = [&](int tile0) __attribute__((always_inline)) {
    kreg[0] = *(const u32x2*)(kp + (size_t)min(tile0 + pi, last) * D);
    kreg[1] = *(const u32x2*)(kp + (size_t)min(tile0 + 16 + pi, last) * D);
    vreg[0] = *(const u32x2*)(vp + (size_t)min(tile0 + vrow, last) * D);
    vreg[1] = *(const u32x2*)(vp + (size_t)min(tile0 + vrow + 1, last) * D);
  };
  auto stage = [&]() __attribute__((always_inline)) {
    *(half8_t*)(k_lds + pi * D + ((c ^ pi) * 8)) = bytes_to_half8(kreg[0][0], kreg[0][1]);   // (rows pi and 16 + pi: the same row & 15)
    *(half8_t*)(k_lds + (16 + pi) * D + ((c ^ pi) * 8)) = bytes_to_half8(kreg[1][0], kreg[1][1]);
    const half8_t v0 = bytes_to_half8(vreg[0][0], vreg[0][1]), v1 = bytes_to_half8(vreg[1][0], vreg[1][1]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = c * 8 + e;
      v_lds[d * PF_VSTRIDE + (((pi >> 2) ^ ((d >> 4) & 3)) * 4) + (pi & 3)] = as_u32(half2_t{v0[e], v1[e]});
    }
  };

  float m_ = -INFINITY, l_ = 0.f;                     // of query qi: the max over all rows so far, the sum over this lane's rows
  floatx4 oacc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) oacc[db] = floatx4{0.f, 0.f, 0.f, 0.f};

  request(0);
  for (int it = 0; it < ntiles; ++it) {
    const int tile0 = it * PF_KVROWS;
    __syncthreads();   // the previous tile has been read by everyone
    stage();
    __syncthreads();
    if (it + 1 < ntiles) request(tile0 + PF_KVROWS);
    if (wave_active && tile0 <= wave_last) {   // (wave-uniform; else the tile lies wholly behind this wave's last query)
      floatx4 d4[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8_t ka = *(const half8_t*)(k_lds + (16 * blk + qi) * D + (((4 * s + rsel) ^ qi) * 8));
          d4[blk] = mfma16(ka, qb[s], d4[blk]);
        }
      const bool diagonal = tile0 + PF_KVROWS - 1 > wave_first;   // (wave-uniform) some query of the wave does not see the whole tile
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
        const half8_t va = *(const half8_t*)(v_lds + (16 * db + qi) * PF_VSTRIDE + ((rsel ^ (db & 3)) * 4));
        oacc[db] = mfma16(va, pb, oacc[db] * corr);
      }
    }
  }
  // the four lanes of a query add up their sums; one division, the one multiply that carries v_scale, one rounding
  l_ += __shfl_xor(l_, 16);
  l_ += __shfl_xor(l_, 32);
#pragma unroll
  for (int db = 0; db < 8; ++db) {
    half4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (half_t)(oacc[db][i] / l_ * v_scale);
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

bool aligned(const void* p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
bool good_scale(float s) { return std::isfinite(s) && s > 0.f; }

int write_check(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float k_scale, float v_scale) {
  if (batch <= 0 || tokens <= 0 || n_heads <= 0 || n_kv_heads <= 0 || cache_len <= 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 rope_kv_write: batch, tokens, n_heads, n_kv_heads and cache_len must be positive");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 rope_kv_write: n_heads must be a multiple of n_kv_heads");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 rope_kv_write: head_dim must be 128");
  if ((long)batch * tokens > 65535)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 rope_kv_write: batch * tokens is a grid dimension and must not exceed 65535");
  if (!good_scale(k_scale) || !good_scale(v_scale))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 rope_kv_write: k_scale and v_scale must be finite and positive");
  return QUICK_OK;
}

int decode_check(int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len) {
  if (batch <= 0 || n_heads <= 0 || n_kv_heads <= 0 || cache_len <= 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 decode attention: batch, n_heads, n_kv_heads and cache_len must be positive");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 decode attention: head_dim must be 128");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 decode attention: n_heads must be a multiple of n_kv_heads");
  const int group = n_heads / n_kv_heads;
  if (group != 1 && group != 2 && group != 4 && group != 8)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 decode attention: 1, 2, 4 or 8 query heads per KV head");
  if (batch > 65535) return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 decode attention: batch is a grid dimension and must not exceed 65535");
  return QUICK_OK;
}

int prefill_check(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len) {
  if (batch <= 0 || tokens <= 0 || n_heads <= 0 || n_kv_heads <= 0 || cache_len <= 0)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 prefill attention: batch, tokens, n_heads, n_kv_heads and cache_len must be positive");
  if (tokens > cache_len)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 prefill attention: more tokens than the cache has rows (tokens > cache_len)");
  if (head_dim != 128) return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 prefill attention: head_dim must be 128");
  if (n_heads % n_kv_heads != 0)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 prefill attention: n_heads must be a multiple of n_kv_heads");
  if (n_heads > 65535 || batch > 65535)
    return set_last_error(QUICK_ERR_UNSUPPORTED, "fp8 prefill attention: n_heads and batch are grid dimensions and must not exceed 65535");
  return QUICK_OK;
}

}  // namespace
}  // namespace quick_amd

using namespace quick_amd;

extern "C" {

int quick_rope_kv_write_fp8(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_cache,
                            void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float k_scale,
                            float v_scale, int per_sequence, void* hip_stream) {
  const int rc = write_check(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len, k_scale, v_scale);
  if (rc != QUICK_OK) return rc;
  if (!aligned(qkv, 16) || !aligned(cos_table, 16) || !aligned(sin_table, 16) || !aligned(pos0, 8) || !aligned(q_out, 16) ||
      !aligned(k_cache, 16) || !aligned(v_cache, 16))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 rope_kv_write: a null or misaligned pointer (16 bytes; pos0: 8)");
  const float k_inv = 1.0f / k_scale, v_inv = 1.0f / v_scale;
  const dim3 grid((unsigned)((n_heads + 2 * n_kv_heads + 3) / 4), (unsigned)(batch * tokens));
#define QA_WRITE(SEQ)                                                                                                              \
  hipLaunchKernelGGL(rope_kv_write_fp8_kernel<SEQ>, grid, dim3(64), 0, (hipStream_t)hip_stream, (const half_t*)qkv,                 \
                     (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos0, (half_t*)q_out, (uint8_t*)k_cache,      \
                     (uint8_t*)v_cache, tokens, n_heads, n_kv_heads, cache_len, k_inv, v_inv)
  if (per_sequence) QA_WRITE(true);
  else QA_WRITE(false);
#undef QA_WRITE
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "fp8 rope_kv_write: the launch failed");
  return QUICK_OK;
}

int quick_decode_rope_attention_fp8(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_cache,
                                    void* v_cache, void* out, int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len,
                                    float scale, float k_scale, float v_scale, int per_sequence, void* hip_stream) {
  const int rc = decode_check(batch, n_heads, n_kv_heads, head_dim, cache_len);
  if (rc != QUICK_OK) return rc;
  if (!good_scale(k_scale) || !good_scale(v_scale))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 decode attention: k_scale and v_scale must be finite and positive");
  if (!aligned(qkv, 16) || !aligned(cos_table, 16) || !aligned(sin_table, 16) || !aligned(pos, 8) || !aligned(k_cache, 16) ||
      !aligned(v_cache, 16) || !aligned(out, 16))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 decode attention: a null or misaligned pointer (16 bytes; pos: 8)");
  const float k_inv = 1.0f / k_scale, v_inv = 1.0f / v_scale;
  const float qk_scale = scale * 1.44269504088896f * k_scale;   // scores in the log2 domain, k_scale folded in
  const dim3 grid((unsigned)n_kv_heads, (unsigned)batch);
#define QA_DEC(GROUP, SEQ)                                                                                                          \
  hipLaunchKernelGGL((decode_rope_attention_fp8_kernel<GROUP, SEQ>), grid, dim3(256), 0, (hipStream_t)hip_stream,                \
                     (const half_t*)qkv, (const half_t*)cos_table, (const half_t*)sin_table, (const long*)pos, (uint8_t*)k_cache,   \
                     (uint8_t*)v_cache, (half_t*)out, n_heads, n_kv_heads, cache_len, qk_scale, k_inv, v_inv, v_scale)
#define QA_DEC2(GROUP)        \
  do {                        \
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
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "fp8 decode attention: the launch failed");
  return QUICK_OK;
}

int quick_decode_rope_attention_fp8_describe(int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len, char* text,
                                             size_t text_bytes) {
  const int rc = decode_check(batch, n_heads, n_kv_heads, head_dim, cache_len);
  if (rc != QUICK_OK) return rc;
  if (!text || text_bytes == 0) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 decode attention: no room for the description");
  snprintf(text, text_bytes, "gqa-mfma-fp8 heads=%d gsplit=1 waves=4 set_rows=64 grid=%dx%d", n_heads / n_kv_heads, n_kv_heads, batch);
  return QUICK_OK;
}

int quick_prefill_attention_fp8(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch, int tokens,
                                int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, float k_scale, float v_scale,
                                int per_sequence, void* hip_stream) {
  const int rc = prefill_check(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len);
  if (rc != QUICK_OK) return rc;
  if (!good_scale(k_scale) || !good_scale(v_scale))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 prefill attention: k_scale and v_scale must be finite and positive");
  if (!aligned(q, 16) || !aligned(k_cache, 16) || !aligned(v_cache, 16) || !aligned(pos0, 8) || !aligned(out, 16))
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "fp8 prefill attention: a null or misaligned pointer (16 bytes; pos0: 8)");
  const float qk_scale = scale * 1.44269504088896f * k_scale;   // scores in the log2 domain, k_scale folded in
  const dim3 grid((unsigned)((tokens + PF_QROWS - 1) / PF_QROWS), (unsigned)n_heads, (unsigned)batch);
#define QA_PF(SEQ)                                                                                                                  \
  hipLaunchKernelGGL(prefill_attention_fp8_kernel<SEQ>, grid, dim3(PF_WAVES * 64), 0, (hipStream_t)hip_stream, (const half_t*)q,     \
                     (const uint8_t*)k_cache, (const uint8_t*)v_cache, (const long*)pos0, (half_t*)out, tokens, n_heads, n_kv_heads, \
                     cache_len, qk_scale, v_scale)
  if (per_sequence) QA_PF(true);
  else QA_PF(false);
#undef QA_PF
  if (hipGetLastError() != hipSuccess) return set_last_error(QUICK_ERR_LAUNCH, "fp8 prefill attention: the launch failed");
  return QUICK_OK;
}

}  // extern "C"
