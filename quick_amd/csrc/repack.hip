// Format bridge between the reference's packed order ("cuda order": what
// WQLinear_QUICK.from_linear writes, quick/awq/modules/linear/quick.py:88-150, and what the CUDA
// kernels index, csrc/gemm_cuda_quick.cu:1257-1277) and the MFMA-fragment order consumed by
// w4a16_gemm.hip ("mi355x order").  One-time, load-side work: gather kernels, one thread per
// output dword.
#include "w4a16_common.hpp"
#include "gate_up_mi355x.hpp"
#include "../../include/quick_amd.h"

#include <cstdio>

namespace quick_amd {

// dword index + nibble of logical weight (k, n) in the reference layout (closed form)
__device__ __forceinline__ void cuda_order_pos(int k, int n, int N, size_t& idx, int& nib) {
  const int kt = k >> 5, half = (k >> 4) & 1, r = k & 15;
  const int l4 = (r & 7) >> 1, hi = r >> 3, odd = r & 1;
  const int bx = n >> 7, ty = (n >> 6) & 1, chunk = (n & 63) >> 4, t = (n & 15) >> 3, j = n & 7;
  idx = (size_t)kt * (4 * N) + (size_t)((2 * ty + (j >> 2)) * (N >> 3) + 16 * bx + 4 * (j & 3) + l4) * 8 + 4 * half + chunk;
  nib = 4 * odd + hi + 2 * t;
}

// slot x(n) of the reference scale / zero permutation
__device__ __forceinline__ int cuda_order_slot(int n, int N) {
  const int bx = n >> 7, ty = (n >> 6) & 1, chunk = (n & 63) >> 4, t = (n & 15) >> 3, j = n & 7;
  return ((2 * ty + (j >> 2)) * (N >> 5) + 4 * bx + (j & 3)) * 8 + 2 * chunk + t;
}

// (k, n) of nibble p of mi355x-order dword d
__device__ __forceinline__ void mi355x_dword_coord(size_t d, int K, int& k0, int& n) {
  const int KT = K >> 7;
  const int t = (int)(d & 3), lane = (int)((d >> 2) & 63);
  const size_t tile = d >> 8;
  const int kt = (int)(tile % KT), nt = (int)(tile / KT);
  n = nt * 16 + (lane & 15);
  k0 = kt * 128 + t * 32 + 8 * (lane >> 4);
}

// K = rows of the OUTPUT (a multiple of 128); rows >= K_in (a multiple of 32: a dword is all inside or all outside) are padding
__global__ __launch_bounds__(256) void repack_weight_cuda_to_mi355x(const uint32_t* __restrict__ in,
                                                                    uint32_t* __restrict__ out, int K, int N, int K_in) {
  const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= (size_t)K * N / 8) return;
  int k0, n;
  mi355x_dword_coord(d, K, k0, n);
  uint32_t v = 0;
  if (k0 >= K_in) {
    out[d] = 0u;
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    size_t idx;
    int nib;
    cuda_order_pos(k0 + j, n, N, idx, nib);
    v |= ((in[idx] >> (4 * nib)) & 15u) << (4 * (4 * (j & 1) + (j >> 1)));
  }
  out[d] = v;
}

__global__ __launch_bounds__(256) void repack_weight_mi355x_to_cuda(const uint32_t* __restrict__ in,
                                                                    uint32_t* __restrict__ out, int K, int N) {
  // one thread per (k, n); scatter with atomicOr into a zeroed buffer
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)K * N) return;
  const int k = (int)(i / N), n = (int)(i % N);
  const int KT = K >> 7;
  const int lane = (n & 15) + 16 * ((k & 31) >> 3), j = k & 7;
  const size_t d = (((size_t)(n >> 4) * KT + (k >> 7)) * 64 + lane) * 4 + ((k & 127) >> 5);
  const uint32_t w = (in[d] >> (4 * (4 * (j & 1) + (j >> 1)))) & 15u;
  size_t idx;
  int nib;
  cuda_order_pos(k, n, N, idx, nib);
  atomicOr(out + idx, w << (4 * nib));
}

// scales / zeros: one thread per (g, n).  MI355X order: the scales tensor holds one 32-bit word per (g, n) -- fp16 scale |
// zero point << 16 -- at word ((n/16) * NG + g) * 16 + n%16 (group_word_index, w4a16_common.hpp); qzeros keeps a plain
// copy of the zero points (nibble n%8 of dword n/8) that the GEMM kernels do not read.
__global__ __launch_bounds__(256) void repack_sz_cuda_to_mi355x(const half_t* __restrict__ s_in,
                                                                const uint32_t* __restrict__ z_in,
                                                                uint32_t* __restrict__ sz_out, uint32_t* __restrict__ z_out,
                                                                int NG, int N, int NG_in) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)NG * N) return;
  const int g = (int)(i / N), n = (int)(i % N);
  if (g >= NG_in) {  // a padding group: scale 0, zero point 0 (z_out was zeroed)
    sz_out[group_word_index(g, n, NG)] = 0u;
    return;
  }
  const int x = cuda_order_slot(n, N);
  const uint32_t z = (z_in[(size_t)g * (N >> 2) + (x >> 2)] >> (4 * (x & 3))) & 15u;
  const uint32_t sbits = __builtin_bit_cast(unsigned short, s_in[(size_t)g * 2 * N + 2 * x]);
  sz_out[group_word_index(g, n, NG)] = sbits | (z << 16);
  atomicOr(z_out + (size_t)g * (N >> 2) + (n >> 3), z << (4 * (n & 7)));
}

__global__ __launch_bounds__(256) void repack_sz_mi355x_to_cuda(const uint32_t* __restrict__ sz_in,
                                                                half_t* __restrict__ s_out, uint32_t* __restrict__ z_out,
                                                                int NG, int N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)NG * N) return;
  const int g = (int)(i / N), n = (int)(i % N);
  const int x = cuda_order_slot(n, N);
  const uint32_t w = sz_in[group_word_index(g, n, NG)];
  const half_t s = __builtin_bit_cast(half_t, (unsigned short)(w & 0xffffu));
  s_out[(size_t)g * 2 * N + 2 * x] = s;
  s_out[(size_t)g * 2 * N + 2 * x + 1] = s;
  const uint32_t z = (w >> 16) & 15u;
  atomicOr(z_out + (size_t)g * (N >> 2) + (x >> 2), (z << (4 * (x & 3))) | (z << (4 * (x & 3) + 16)));
}

// ------------------------------------------------------------------------------------------------
// AWQ "GEMM packing" (WQLinear_GEMM checkpoints) <-> mi355x order.  GEMM packing, closed form: qweight int32 [K, N/8], nibble i of
// dword c of row k = iw[k, 8c + order[i]], order = {0, 2, 4, 6, 1, 3, 5, 7}; qzeros int32 [K/G, N/8], the same packing of z[g, n];
// scales fp16 [K/G, N] plain.  Channel 8c + m therefore sits at nibble awq_nibble(m) = {0, 4, 1, 5, 2, 6, 3, 7}[m] = (m >> 1) + 4 * (m & 1).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int awq_nibble(int m) { return (m >> 1) + 4 * (m & 1); }
__device__ __forceinline__ int awq_channel(int i) { return 2 * (i & 3) + (i >> 2); }   // order[i]

constexpr int kAwqTileK = 128;    // rows of a staged block = one k tile of the mi355x order
constexpr int kAwqTileN = 256;    // channels of a staged block (the last block of a row of blocks holds 128 when N % 256 == 128)
constexpr int kAwqRowPad = 1;     // LDS row stride 33 / 17 dwords: the rows k0 + j, k0 + 8 + j, ... a wave gathers from fall on distinct banks

// Weights: every mi355x dword is an 8 x 8 nibble transpose of eight GEMM-packing dwords from eight consecutive rows.  A workgroup stages
// 128 k x 256 (128) channels through LDS -- each input dword read once, in 16-byte pieces of whole 128- (64-) byte row segments -- and
// writes the 16 (8) output tiles of 1 KiB as one 16-byte piece per lane.  Grid: (ceil(N / 256), Kp / 128); rows >= K_in are padding (0).
__global__ __launch_bounds__(256) void repack_weight_awq_gemm_to_mi355x(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                         int Kp, int N, int K_in) {
  __shared__ uint32_t tile[kAwqTileK * (kAwqTileN / 8 + kAwqRowPad)];
  const int n0 = blockIdx.x * kAwqTileN, kt = blockIdx.y;
  const int nc = min(kAwqTileN, N - n0);          // 256 or 128
  const int W = nc >> 3, W4 = nc >> 5;            // dwords / 16-byte pieces per staged row
  const int stride = W + kAwqRowPad;
  const size_t ND = (size_t)(N >> 3);             // dwords per input row
  for (int p = threadIdx.x; p < kAwqTileK * W4; p += 256) {
    const int r = p / W4, c4 = p % W4;
    const int k = kt * kAwqTileK + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (k < K_in) v = *(const u32x4*)(in + (size_t)k * ND + (size_t)(n0 >> 3) + 4 * c4);
    uint32_t* dst = tile + r * stride + 4 * c4;
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
  }
  __syncthreads();
  const int KT = Kp >> 7;
  for (int p = threadIdx.x; p < (nc >> 4) * 64; p += 256) {     // one 16-byte piece of an output tile: lane `lane` of tile (n / 16, kt)
    const int ntl = p >> 6, lane = p & 63;
    const int nl = ntl * 16 + (lane & 15);
    const int col = nl >> 3, sh = 4 * awq_nibble(nl & 7);
    u32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t* src = tile + (t * 32 + 8 * (lane >> 4)) * stride + col;
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) v |= ((src[j * stride] >> sh) & 15u) << (4 * (4 * (j & 1) + (j >> 1)));
      o[t] = v;
    }
    const size_t tileidx = (size_t)((n0 >> 4) + ntl) * KT + kt;
    *(u32x4*)(out + (tileidx * 64 + lane) * 4) = o;
  }
}

// scales / zeros, GEMM packing -> mi355x order: one thread per (g, n) writes the (scale | zero point << 16) word; groups >= NG_in are padding
__global__ __launch_bounds__(256) void repack_sz_awq_gemm_to_mi355x(const half_t* __restrict__ s_in, const uint32_t* __restrict__ z_in,
                                                                     uint32_t* __restrict__ sz_out, int NG, int N, int NG_in) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)NG * N) return;
  const int g = (int)(i / N), n = (int)(i % N);
  uint32_t w = 0u;
  if (g < NG_in) {
    const uint32_t z = (z_in[(size_t)g * (N >> 3) + (n >> 3)] >> (4 * awq_nibble(n & 7))) & 15u;
    w = (uint32_t)__builtin_bit_cast(unsigned short, s_in[(size_t)g * N + n]) | (z << 16);
  }
  sz_out[group_word_index(g, n, NG)] = w;
}

// the plain copy of the zero points (nibble n % 8 of dword n / 8 of a row of N / 4 dwords, whose second half stays 0): one thread per output
// dword puts the eight nibbles of the same input dword in channel order, or writes the 0
__global__ __launch_bounds__(256) void repack_z_awq_gemm_to_mi355x(const uint32_t* __restrict__ z_in, uint32_t* __restrict__ z_out,
                                                                    int NG, int N, int NG_in) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t ND = (size_t)(N >> 3), row = (size_t)(N >> 2);
  if (i >= (size_t)NG * row) return;
  const size_t g = i / row, c = i % row;
  uint32_t v = 0u;
  if (g < (size_t)NG_in && c < ND) {
    const uint32_t q = z_in[g * ND + c];
#pragma unroll
    for (int m = 0; m < 8; ++m) v |= ((q >> (4 * awq_nibble(m))) & 15u) << (4 * m);
  }
  z_out[i] = v;
}

// mi355x order -> GEMM packing (state_dict(), saving): gathers, one thread per output dword.  K % 128 == 0.
__global__ __launch_bounds__(256) void repack_weight_mi355x_to_awq_gemm(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                         int K, int N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t ND = (size_t)(N >> 3);
  if (i >= (size_t)K * ND) return;
  const int k = (int)(i / ND), c = (int)(i % ND);
  const int KT = K >> 7, j = k & 7;
  const int sh = 4 * (4 * (j & 1) + (j >> 1));
  uint32_t v = 0u;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int n = 8 * c + awq_channel(b);
    const int lane = (n & 15) + 16 * ((k & 31) >> 3);
    const size_t d = (((size_t)(n >> 4) * KT + (k >> 7)) * 64 + lane) * 4 + ((k & 127) >> 5);
    v |= ((in[d] >> sh) & 15u) << (4 * b);
  }
  out[i] = v;
}

// one thread per (g, n / 8): eight scale words -> eight fp16 scales (one 16-byte store) and one dword of zero points (read from the words)
__global__ __launch_bounds__(256) void repack_sz_mi355x_to_awq_gemm(const uint32_t* __restrict__ sz_in, half_t* __restrict__ s_out,
                                                                     uint32_t* __restrict__ z_out, int NG, int N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t ND = (size_t)(N >> 3);
  if (i >= (size_t)NG * ND) return;
  const int g = (int)(i / ND), c = (int)(i % ND);
  const uint32_t* w = sz_in + group_word_index(g, 8 * c, NG);    // 8c .. 8c + 7 lie in one 16-channel block: consecutive words
  uint32_t z = 0u;
  u32x4 s;
#pragma unroll
  for (int m = 0; m < 8; m += 2) {
    const uint32_t a = w[m], b = w[m + 1];
    s[m >> 1] = (a & 0xffffu) | (b << 16);
    z |= (((a >> 16) & 15u) << (4 * awq_nibble(m))) | (((b >> 16) & 15u) << (4 * awq_nibble(m + 1)));
  }
  *(u32x4*)(s_out + (size_t)g * N + 8 * (size_t)c) = s;
  z_out[i] = z;
}

// ------------------------------------------------------------------------------------------------
// gate_proj / up_proj <-> the fused layer of the silu_mul epilogue (output channels: gate and up interleaved in blocks of 8), all in mi355x
// order.  In this order the interleave moves whole 16-byte pieces: with the weights viewed as pieces
// [channel tile of 16][k tile][quarter q = (k % 32) / 8][c = n % 16], fused piece (T, kt, q, c) is piece (T / 2, kt, q, 8 * (T % 2) + c % 8) of
// gate (c < 8) or up (c >= 8); the scale words [channel tile][group][16] follow the same rule, four words to a piece; the plain zero-point
// copy interleaves dwords (eight channels each) in the first half of a row and is 0 in the second.  One lane per fused piece, the same
// index in both directions -- kSplit only turns the copy round -- and one launch for the three tensors: workgroups [0, wblocks) move weights,
// [wblocks, wblocks + sblocks) scale words, the rest zero points.  The lane's work is gate_up_mi355x_lane (gate_up_mi355x.hpp), which a host
// program can run too (tools/gate_up_host_check.py: every index under the address sanitizer).
// ------------------------------------------------------------------------------------------------
template <bool kSplit>
__global__ __launch_bounds__(256) void gate_up_mi355x(u32x4* __restrict__ gate_qw, u32x4* __restrict__ gate_sc, u32x4* __restrict__ gate_qz,
                                                      u32x4* __restrict__ up_qw, u32x4* __restrict__ up_sc, u32x4* __restrict__ up_qz,
                                                      u32x4* __restrict__ fused_qw, u32x4* __restrict__ fused_sc, u32x4* __restrict__ fused_qz,
                                                      int K, int I, int NG, unsigned wblocks, unsigned sblocks) {
  gate_up_mi355x_lane<kSplit>(gate_qw, gate_sc, gate_qz, up_qw, up_sc, up_qz, fused_qw, fused_sc, fused_qz, K, I, NG, wblocks, sblocks,
                              blockIdx.x, threadIdx.x);
}

static int check(int K, int N, int G) {
  if (K <= 0 || N <= 0 || G <= 0 || N % 128 != 0 || G % 32 != 0 || K % G != 0) return QUICK_ERR_INVALID_ARGUMENT;
  if (K % 128 != 0) return QUICK_ERR_UNSUPPORTED;
  return QUICK_OK;
}

}  // namespace quick_amd

using namespace quick_amd;

extern "C" {

static int repack_to_mi355x(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                            void* scales_out, void* qzeros_out, int K_in, int K, int N, int group_size, hipStream_t st) {
  const int NG = K / group_size;
  const size_t nd = (size_t)K * N / 8;
  if (hipMemsetAsync(qzeros_out, 0, (size_t)NG * (N / 4) * 4, st) != hipSuccess) return QUICK_ERR_LAUNCH;
  hipLaunchKernelGGL(repack_weight_cuda_to_mi355x, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)qweight_in, (uint32_t*)qweight_out, K, N, K_in);
  hipLaunchKernelGGL(repack_sz_cuda_to_mi355x, dim3((unsigned)(((size_t)NG * N + 255) / 256)), dim3(256), 0, st,
                     (const half_t*)scales_in, (const uint32_t*)qzeros_in, (uint32_t*)scales_out, (uint32_t*)qzeros_out, NG, N,
                     K_in / group_size);
  return hipGetLastError() == hipSuccess ? QUICK_OK : QUICK_ERR_LAUNCH;
}

int quick_repack_cuda_to_mi355x(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                                void* scales_out, void* qzeros_out, int K, int N, int group_size, void* hip_stream) {
  if (int rc = check(K, N, group_size)) return rc;
  return repack_to_mi355x(qweight_in, scales_in, qzeros_in, qweight_out, scales_out, qzeros_out, K, K, N, group_size, (hipStream_t)hip_stream);
}

int quick_padded_in_features(int K, int group_size) {
  if (K <= 0 || group_size <= 0 || group_size % 32 != 0 || K % 32 != 0 || K % group_size != 0) return 0;
  int a = 128, b = group_size;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  const long unit = 128L * group_size / a;  // lcm(128, group_size)
  return (int)(((long)K + unit - 1) / unit * unit);
}

int quick_repack_cuda_to_mi355x_padded(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                                       void* scales_out, void* qzeros_out, int K, int N, int group_size, void* hip_stream) {
  const int Kp = quick_padded_in_features(K, group_size);
  if (Kp == 0 || N <= 0 || N % 128 != 0) return QUICK_ERR_INVALID_ARGUMENT;
  return repack_to_mi355x(qweight_in, scales_in, qzeros_in, qweight_out, scales_out, qzeros_out, K, Kp, N, group_size, (hipStream_t)hip_stream);
}

int quick_repack_mi355x_to_cuda(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                                void* scales_out, void* qzeros_out, int K, int N, int group_size, void* hip_stream) {
  if (int rc = check(K, N, group_size)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  const int NG = K / group_size;
  if (hipMemsetAsync(qweight_out, 0, (size_t)K * N / 2, st) != hipSuccess) return QUICK_ERR_LAUNCH;
  if (hipMemsetAsync(qzeros_out, 0, (size_t)NG * (N / 4) * 4, st) != hipSuccess) return QUICK_ERR_LAUNCH;
  hipLaunchKernelGGL(repack_weight_mi355x_to_cuda, dim3((unsigned)(((size_t)K * N + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)qweight_in, (uint32_t*)qweight_out, K, N);
  (void)qzeros_in;  // the zero points travel in the scales tensor's words
  hipLaunchKernelGGL(repack_sz_mi355x_to_cuda, dim3((unsigned)(((size_t)NG * N + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)scales_in, (half_t*)scales_out, (uint32_t*)qzeros_out, NG, N);
  return hipGetLastError() == hipSuccess ? QUICK_OK : QUICK_ERR_LAUNCH;
}

// shape rules of the GEMM-packing bridge, answered before any GPU work (include/quick_amd.h)
static int check_awq_gemm(const char* fn, int K, int N, int G, bool need_k128) {
  char text[256];
  const char* why = nullptr;
  int code = QUICK_ERR_INVALID_ARGUMENT;
  if (K <= 0 || N <= 0 || G <= 0) why = "non-positive dimension";
  else if (N % 8 != 0) why = "OC is not multiple of pack_num = 8";
  else if (G % 32 != 0) why = "Group size should be a multiple of 32";
  else if (K % G != 0) why = "in_features is not a multiple of the group size";
  else if (K % 32 != 0) why = "in_features must be a multiple of 32";
  else {
    code = QUICK_ERR_UNSUPPORTED;
    if (N % 128 != 0) why = "OC must be a multiple of 128 for the MI355X GEMM kernels";
    else if (need_k128 && K % 128 != 0) why = "in_features must be a multiple of 128: a padded MI355X copy is never turned back";
  }
  if (!why) return QUICK_OK;
  snprintf(text, sizeof(text), "%s: %s (K=%d N=%d G=%d)", fn, why, K, N, G);
  return set_last_error(code, text);
}

int quick_repack_awq_gemm_to_mi355x(const void* qweight_in, const void* qzeros_in, const void* scales_in, void* qweight_out,
                                    void* scales_out, void* qzeros_out, int K, int N, int group_size, void* hip_stream) {
  if (int rc = check_awq_gemm("quick_repack_awq_gemm_to_mi355x", K, N, group_size, false)) return rc;
  if (!qweight_in || !qzeros_in || !scales_in || !qweight_out || !scales_out || !qzeros_out)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "quick_repack_awq_gemm_to_mi355x: null tensor pointer");
  hipStream_t st = (hipStream_t)hip_stream;
  const int Kp = quick_padded_in_features(K, group_size);
  const int NG = Kp / group_size, NG_in = K / group_size;
  hipLaunchKernelGGL(repack_weight_awq_gemm_to_mi355x, dim3((unsigned)((N + kAwqTileN - 1) / kAwqTileN), (unsigned)(Kp / kAwqTileK)),
                     dim3(256), 0, st, (const uint32_t*)qweight_in, (uint32_t*)qweight_out, Kp, N, K);
  hipLaunchKernelGGL(repack_sz_awq_gemm_to_mi355x, dim3((unsigned)(((size_t)NG * N + 255) / 256)), dim3(256), 0, st,
                     (const half_t*)scales_in, (const uint32_t*)qzeros_in, (uint32_t*)scales_out, NG, N, NG_in);
  hipLaunchKernelGGL(repack_z_awq_gemm_to_mi355x, dim3((unsigned)(((size_t)NG * (N / 4) + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)qzeros_in, (uint32_t*)qzeros_out, NG, N, NG_in);
  return hipGetLastError() == hipSuccess ? QUICK_OK : set_last_error(QUICK_ERR_LAUNCH, "quick_repack_awq_gemm_to_mi355x: launch failed");
}

int quick_repack_mi355x_to_awq_gemm(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                                    void* qzeros_out, void* scales_out, int K, int N, int group_size, void* hip_stream) {
  if (int rc = check_awq_gemm("quick_repack_mi355x_to_awq_gemm", K, N, group_size, true)) return rc;
  if (!qweight_in || !scales_in || !qweight_out || !qzeros_out || !scales_out)
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "quick_repack_mi355x_to_awq_gemm: null tensor pointer");
  hipStream_t st = (hipStream_t)hip_stream;
  const int NG = K / group_size;
  (void)qzeros_in;  // the zero points travel in the scales tensor's words
  hipLaunchKernelGGL(repack_weight_mi355x_to_awq_gemm, dim3((unsigned)(((size_t)K * (N / 8) + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)qweight_in, (uint32_t*)qweight_out, K, N);
  hipLaunchKernelGGL(repack_sz_mi355x_to_awq_gemm, dim3((unsigned)(((size_t)NG * (N / 8) + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)scales_in, (half_t*)scales_out, (uint32_t*)qzeros_out, NG, N);
  return hipGetLastError() == hipSuccess ? QUICK_OK : set_last_error(QUICK_ERR_LAUNCH, "quick_repack_mi355x_to_awq_gemm: launch failed");
}

}  // extern "C"

// shape rules of the gate/up interleave, answered before any GPU work (include/quick_amd.h)
static int check_gate_up(const char* fn, int K, int I, int G) {
  char text[256];
  const char* why = nullptr;
  int code = QUICK_ERR_INVALID_ARGUMENT;
  if (K <= 0 || I <= 0 || G <= 0) why = "non-positive dimension";
  else if (G % 32 != 0) why = "Group size should be a multiple of 32";
  else if (K % G != 0) why = "in_features is not a multiple of the group size";
  else if (I % 8 != 0) why = "intermediate size is not multiple of pack_num = 8";
  else {
    code = QUICK_ERR_UNSUPPORTED;
    if (K % 128 != 0) why = "in_features must be a multiple of 128: gate and up are interleaved in MI355X order, which a padded layer does not have";
    else if (I % 64 != 0) why = "intermediate size must be a multiple of 64: the fused layer's 2 * I channels must be a multiple of 128 for the MI355X GEMM kernels";
  }
  if (!why) return QUICK_OK;
  snprintf(text, sizeof(text), "%s: %s (K=%d I=%d G=%d)", fn, why, K, I, G);
  return set_last_error(code, text);
}

template <bool kSplit>
static int launch_gate_up(const char* fn, void* const (&t)[9], int K, int I, int G, void* hip_stream) {
  if (int rc = check_gate_up(fn, K, I, G)) return rc;
  char text[128];
  for (void* p : t) {
    if (p && ((uintptr_t)p & 15) == 0) continue;
    snprintf(text, sizeof(text), "%s: %s", fn, p ? "tensor pointers must be 16-byte aligned" : "null tensor pointer");
    return set_last_error(QUICK_ERR_INVALID_ARGUMENT, text);
  }
  const int NG = K / G;
  if (((size_t)K * I / 16 + (size_t)NG * I / 2 + (size_t)NG * (I / 16)) / 256 + 3 > 0x7fffffffu) {     // (Llama-2-70B: 57.8 k workgroups)
    snprintf(text, sizeof(text), "%s: the layer needs more workgroups than one grid dimension holds", fn);
    return set_last_error(QUICK_ERR_UNSUPPORTED, text);
  }
  const unsigned wblocks = (unsigned)(((size_t)K * I / 16 + 255) / 256), sblocks = (unsigned)(((size_t)NG * I / 2 + 255) / 256);
  const unsigned zblocks = (unsigned)(((size_t)NG * (I / 16) + 255) / 256);
  hipLaunchKernelGGL(gate_up_mi355x<kSplit>, dim3(wblocks + sblocks + zblocks), dim3(256), 0, (hipStream_t)hip_stream, (u32x4*)t[0], (u32x4*)t[1],
                     (u32x4*)t[2], (u32x4*)t[3], (u32x4*)t[4], (u32x4*)t[5], (u32x4*)t[6], (u32x4*)t[7], (u32x4*)t[8], K, I, NG, wblocks, sblocks);
  if (hipGetLastError() == hipSuccess) return QUICK_OK;
  snprintf(text, sizeof(text), "%s: launch failed", fn);
  return set_last_error(QUICK_ERR_LAUNCH, text);
}

extern "C" {

int quick_interleave_gate_up_mi355x(const void* gate_qweight, const void* gate_scales, const void* gate_qzeros, const void* up_qweight,
                                    const void* up_scales, const void* up_qzeros, void* qweight_out, void* scales_out, void* qzeros_out,
                                    int K, int I, int group_size, void* hip_stream) {
  void* const t[9] = {(void*)gate_qweight, (void*)gate_scales, (void*)gate_qzeros, (void*)up_qweight, (void*)up_scales, (void*)up_qzeros,
                      qweight_out, scales_out, qzeros_out};
  return launch_gate_up<false>("quick_interleave_gate_up_mi355x", t, K, I, group_size, hip_stream);
}

int quick_split_gate_up_mi355x(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* gate_qweight, void* gate_scales,
                               void* gate_qzeros, void* up_qweight, void* up_scales, void* up_qzeros, int K, int I, int group_size,
                               void* hip_stream) {
  void* const t[9] = {gate_qweight, gate_scales, gate_qzeros, up_qweight, up_scales, up_qzeros,
                      (void*)qweight_in, (void*)scales_in, (void*)qzeros_in};
  return launch_gate_up<true>("quick_split_gate_up_mi355x", t, K, I, group_size, hip_stream);
}

}  // extern "C"
