// W4A16 GEMM for MI355X (gfx950), the tiled family (large M): 64 x 128 workgroup tile, x staged in LDS *in fragment order* by
// global_load_lds, 8 waves = 4 along N x 2 along K.  Kernels, instantiations and launcher (the design: w4a16_skinny.hip).
#include "w4a16_common.hpp"

#include "w4a16_args.hpp"
#include "w4a16_launch.hpp"
#include "w4a16_plan.hpp"

namespace quick_amd {

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

template <int BMT, int TN, int WK, int GM, int ABL, int WN>
static bool tiled_go(const GemmArgs& a, const Launch& L, dim3 grid) {
  constexpr unsigned lds = 2 * 4 * WK * BMT * 1024;
  launch_kernel<w4a16_tiled_kernel<BMT, TN, WK, GM, ABL, WN>>(L, grid, dim3(64 * WN * WK), lds, (int)lds, a);
  return true;
}

template <int BMT, int WK, int WN = 4, int TCH = 128>
static bool launch_tiled(const Plan& p, const GemmArgs& a, const Launch& L) {
  constexpr int TN = TCH / 16 / WN;  // channel tiles per wave
  const dim3 grid((a.N / TCH) * ((a.M + BMT * 16 - 1) / (BMT * 16)), p.ksplit);
  if (a.span) return false;  // no tiled kernel carries span stamps
#ifdef QUICK_AMD_TOOLS
  if constexpr (BMT == 4 && WN == 4 && TCH == 128) if (p.ablate && a.G == 128) {  // timing experiments (tools/): results are wrong on purpose
    switch (p.ablate) {
      case 1: return tiled_go<BMT, TN, WK, 0, 1, WN>(a, L, grid);
      case 2: return tiled_go<BMT, TN, WK, 0, 2, WN>(a, L, grid);
      case 3: return tiled_go<BMT, TN, WK, 0, 3, WN>(a, L, grid);
      case 4: return tiled_go<BMT, TN, WK, 0, 4, WN>(a, L, grid);
      case 7: return tiled_go<BMT, TN, WK, 0, 7, WN>(a, L, grid);
      case 15: return tiled_go<BMT, TN, WK, 0, 15, WN>(a, L, grid);
      case 16: return tiled_go<BMT, TN, WK, 0, 16, WN>(a, L, grid);
      case 17: return tiled_go<BMT, TN, WK, 0, 17, WN>(a, L, grid);
      case 18: return tiled_go<BMT, TN, WK, 0, 18, WN>(a, L, grid);
      case 20: return tiled_go<BMT, TN, WK, 0, 20, WN>(a, L, grid);
      case 22: return tiled_go<BMT, TN, WK, 0, 22, WN>(a, L, grid);
      case 23: return tiled_go<BMT, TN, WK, 0, 23, WN>(a, L, grid);
      default: break;
    }
  }
#endif
  switch (group_mode(a.G)) {
    case 0: return tiled_go<BMT, TN, WK, 0, 0, WN>(a, L, grid);
    case 1: return tiled_go<BMT, TN, WK, 1, 0, WN>(a, L, grid);
    case 2: return tiled_go<BMT, TN, WK, 2, 0, WN>(a, L, grid);
    case 3: return tiled_go<BMT, TN, WK, 3, 0, WN>(a, L, grid);
    default: return tiled_go<BMT, TN, WK, 4, 0, WN>(a, L, grid);
  }
}

bool tiled_launch(const Plan& p, const GemmArgs& a, const Launch& L) {
  if (p.tch == 256 && p.mt == 8) return launch_tiled<8, 1, 4, 256>(p, a, L);  // 128 x 256, four waves of 128 tokens x 64 channels
  if (p.tch == 256) return launch_tiled<4, 2, 4, 256>(p, a, L);    // 64 tokens x 256 channels, 4 channel tiles per wave
  if (p.mt == 4 && p.wn2) return launch_tiled<4, 4, 2>(p, a, L);  // 2 waves along N x 4 along K, 64 channels per wave
  if (p.mt == 2) return launch_tiled<2, 2>(p, a, L);
  if (p.mt == 8) return launch_tiled<8, 2>(p, a, L);
  if (p.waves == 8) return launch_tiled<4, 2>(p, a, L);
  return launch_tiled<4, 4>(p, a, L);
}

}  // namespace quick_amd
