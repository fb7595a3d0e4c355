// W4A16 GEMM for MI355X (gfx950): y[M,N] = x[M,K] @ fp16((w - z) * s).  The dispatcher: validation, the plan, the workspace, one launch
// through the family's launcher, and every C entry point (include/quick_amd.h).  The kernels live with their families: w4a16_skinny.hip
// (the design), w4a16_tiled.hip, w4a16_wide.hip, w4a16_lean*.hip, w4a16_xm.hip, w4a16_xw.hip, w4a16_xk.hip; the planner in w4a16_plan.hip.
#include "w4a16_common.hpp"
#include "../../include/quick_amd.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "w4a16_args.hpp"
#include "w4a16_launch.hpp"
#include "w4a16_xk_host.hpp"
#include "w4a16_xw_host.hpp"
#include "w4a16_lean_host.hpp"
#include "w4a16_xm_host.hpp"
#include "w4a16_plan.hpp"
namespace quick_amd {

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

// (the other translation units of the library leave their sentence through this one: w4a16_common.hpp)
int quick_amd::set_last_error(int code, const char* text) { return fail(code, "%s", text); }

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

struct Fusion {
  const void* bias = nullptr;
  const void* residual = nullptr;
  const void* ln_w = nullptr;
  float ln_eps = 0.f;
  int silu_mul = 0;
};


// One function per family: its refusals, the ABL value of its build (0; 32 = in-kernel span stamps; tools builds: timing experiments) and its
// launcher, which says whether a build exists.  A launcher that answers false has launched nothing.
static int no_span_build() { return fail(QUICK_ERR_UNSUPPORTED, "no span-stamped build of the kernel this shape runs"); }

static int run_lean(const Plan& p, const GemmArgs& a, const Launch& L) {
  int abl = a.span ? 32 : 0;
#ifdef QUICK_AMD_TOOLS
  if (p.ablate == 16) abl = 64;  // phase stamps into the workspace (tools/lean_phases.py)
  else if (p.ablate) return fail(QUICK_ERR_INVALID_ARGUMENT, "LEAN: timing-experiment bit 16 (stamps) only");
#endif
  if (!p.lean_tmax || !lean_launch(p.waves, p.lean_tmax, p.mt, abl, a, p.grid_x, (a.M + 15) / 16, L))
    return fail(QUICK_ERR_UNSUPPORTED, "no lean build for K=%d G=%d waves=%d (G %% 128 == 0, waves <= K / 128 <= 16 waves, x + table within 160 KiB of LDS)", a.K, a.G, p.waves);
  return QUICK_OK;
}

static int run_xm(const Plan& p, const GemmArgs& a, const Launch& L) {
  int abl = a.span ? 32 : 0;
#ifdef QUICK_AMD_TOOLS
  if (p.ablate == 16) abl = 64;  // phase stamps into the workspace (tools/xm_phases.py)
  else if (p.ablate) return fail(QUICK_ERR_INVALID_ARGUMENT, "XM: timing-experiment bit 16 (stamps) only");
#endif
  if (!p.lean_tmax || !xm_launch(p.wide_mb, p.wide_pairs, abl, a, p.grid_x, p.ntiles / p.grid_x, L))
    return fail(QUICK_ERR_UNSUPPORTED, "no mid-token build for K=%d G=%d (G a power-of-two multiple of 128, 32-bit offsets)", a.K, a.G);
  return QUICK_OK;
}

static int run_xw(const Plan& p, GemmArgs a, const Launch& L) {
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
  if (!xw_launch(p.wide_mb, p.wide_pairs, p.ksplit, abl, a, p.ntiles * p.ksplit, L))
    return fail(QUICK_ERR_UNSUPPORTED, "no four-wave build for tokens=%d channels=%d slices=%d abl=%d", p.wide_mb * 32, p.tch, p.ksplit, abl);
  return QUICK_OK;
}

static int run_xk(const Plan& p, GemmArgs a, const Launch& L) {
  if (a.silu_mul && !xk_takes_silu(p))
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
  if (!xk_launch(XkConfig{p.wide_mb, p.ksplit, p.xk_nbuf, p.xk_wd, abl, p.xk_kq, p.xk_loader ? 1 : 0}, a, p.ntiles * p.ksplit, L)) {
    if (abl == 32) return no_span_build();
    return fail(QUICK_ERR_UNSUPPORTED, "no exchange-K build for tokens=%d slices=%d ring=%d queue=%d%s", p.wide_mb * 32, p.ksplit, p.xk_nbuf,
                p.xk_wd, abl ? " (timing-experiment bits need a QUICK_AMD_TOOLS build)" : "");
  }
  return QUICK_OK;
}

static int run_wide(const Plan& p, const GemmArgs& a, const Launch& L) {
#ifndef QUICK_AMD_TOOLS
  if (p.wide_mb == 8 && p.wide_pairs == 2)  // r02's hipcc-scheduled 256 x 256 tile: the A/B partner of the generated loop
    return fail(QUICK_ERR_UNSUPPORTED, "the hipcc-scheduled 256 x 256 tile is only in a QUICK_AMD_TOOLS build (the product runs the generated loop, w4a16_xw.hpp, or 128 x 256 tiles)");
#endif
  return wide_launch(p, a, L) ? QUICK_OK : no_span_build();
}

static int run_skinny(const Plan& p, const GemmArgs& a, const Launch& L) {
  if (p.mt == 7 && (p.frag8_t != 8 || p.ksplit != 1))
    return fail(QUICK_ERR_UNSUPPORTED, "skinny: seven channel tiles per workgroup only in the straight-line fragment kernel (K = 8192, one slice), no RMSNorm prologue");
  if (p.mt == 8 && !p.frag8_t)
    return fail(QUICK_ERR_UNSUPPORTED, "skinny: eight channel tiles per workgroup only in the straight-line fragment kernel, no RMSNorm prologue");
  return skinny_launch(p, a, L) ? QUICK_OK : no_span_build();
}

static int run_tiled(const Plan& p, const GemmArgs& a, const Launch& L) { return tiled_launch(p, a, L) ? QUICK_OK : no_span_build(); }

static int run_gemm(const void* x, const void* qweight, const void* scales, const void* qzeros, const Fusion& f, void* y,
                    void* workspace, size_t workspace_bytes, int M, int K, int N, int G, int kernel, int grid_split_k,
                    const Launch& L) {
  // 1. validate
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
  // 2. plan
  const Plan p = plan_for(M, K, N, G, kernel, grid_split_k, f.silu_mul != 0, f.ln_w != nullptr);
  if (f.silu_mul && (f.bias || f.residual)) return fail(QUICK_ERR_INVALID_ARGUMENT, "silu_mul excludes bias and residual");
  if (f.ln_w && !plan_takes_rmsnorm(p))  // (covers every family: only LEAN and some SKINNY plans take the prologue)
    return fail(QUICK_ERR_UNSUPPORTED, "RMSNorm prologue: only on the deferred-zero path (see quick_w4a16_can_fuse_rmsnorm)");
  // 3. arguments
  GemmArgs a{(const half_t*)x, (const u32x4*)qweight, (const half_t*)scales, (const uint32_t*)qzeros, (const half_t*)f.bias,
             (const half_t*)f.residual, f.silu_mul, (half_t*)y, nullptr, nullptr, M, K, N, G, std::max(1, G / 128), p.ksplit, p.kt_per_split, p.xcd_gm, nullptr, (const half_t*)f.ln_w, f.ln_eps};
  // (phase stamps: the LAST 2 MiB of the workspace, behind whatever a K split needs)
  if (p.ablate >= 16 && workspace && workspace_bytes >= (size_t)4096 * 8 * 64 + workspace_need(p))
    a.dbg = (unsigned long long*)((char*)workspace + workspace_bytes - (size_t)4096 * 8 * 64);
  a.span = L.span;
  // 4. workspace
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
  // 5. launch
  int rc;
  switch (p.kernel) {
    case QUICK_KERNEL_LEAN: rc = run_lean(p, a, L); break;
    case QUICK_KERNEL_XM: rc = run_xm(p, a, L); break;
    case QUICK_KERNEL_XW: rc = run_xw(p, a, L); break;
    case QUICK_KERNEL_XK: rc = run_xk(p, a, L); break;
    case QUICK_KERNEL_WIDE: rc = run_wide(p, a, L); break;
    case QUICK_KERNEL_SKINNY: rc = run_skinny(p, a, L); break;
    default: rc = run_tiled(p, a, L); break;
  }
  if (rc != QUICK_OK) return rc;
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
