/*
 * quick_amd.h -- C ABI of libquick_amd.so: the MI355X (gfx950) W4A16 GEMM behind the
 * SqueezeBits/QUICK operator `quick_kernels.gemm_forward_cuda_quick`.
 *
 * Plain pointers and sizes only: no torch types, no C++ in the signatures.  All pointers are
 * DEVICE pointers unless stated otherwise; `hip_stream` is a hipStream_t passed as void*
 * (NULL = the null stream).  Every entry point is asynchronous with respect to the host and
 * returns a status code; the text of the last error on the calling thread is available through
 * quick_amd_last_error().
 *
 * Reference interfaces replaced (paths relative to the reference repository root):
 *   quick_w4a16_gemm_f16          <- torch::Tensor gemm_forward_cuda_quick(Tensor, Tensor, Tensor,
 *                                    Tensor, int)           csrc/gemm_cuda_quick.h:3-8,
 *                                    host function          csrc/gemm_cuda_quick.cu:1456-1517,
 *                                    exported by            csrc/pybind.cpp:5-8
 *   quick_w4a16_workspace_bytes   <- the `torch::empty({split_k_iters, M, N})` scratch
 *                                                            csrc/gemm_cuda_quick.cu:1468
 *   quick_repack_cuda_to_mi355x   <- the offline interleave of WQLinear_QUICK.from_linear
 *   quick_repack_mi355x_to_cuda      quick/awq/modules/linear/quick.py:88-150 (format bridge:
 *                                    the reference's packed order <-> the MFMA-fragment order)
 */
#ifndef QUICK_AMD_H
#define QUICK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QUICK_AMD_ABI_VERSION 1

/* status codes */
#define QUICK_OK 0
#define QUICK_ERR_INVALID_ARGUMENT 1 /* shape rule violated: the reference throws std::invalid_argument
                                        (csrc/gemm_cuda_quick.cu:1479-1484) -> Python ValueError */
#define QUICK_ERR_WORKSPACE 2        /* workspace missing or too small */
#define QUICK_ERR_LAUNCH 3           /* HIP launch error */
#define QUICK_ERR_UNSUPPORTED 4      /* valid for the reference but outside this library's envelope */

/* kernel selection for quick_w4a16_gemm_f16_ex (tests / bench); 0 = library heuristic */
#define QUICK_KERNEL_AUTO 0
#define QUICK_KERNEL_SKINNY 1 /* M-tiles straight from L2 to VGPRs, k split over the waves of a workgroup */
#define QUICK_KERNEL_TILED 2  /* activations staged through LDS, MFMA-bound regime */
#define QUICK_KERNEL_WIDE 3   /* large M: 32x32x16 MFMA, one wave per SIMD, operands by LDS-DMA (G % 128 == 0; else TILED runs) */
#define QUICK_KERNEL_XK 4     /* 64- / 128-token tiles, eight waves, the K slices of a tile on different CUs exchange partial tiles
                                 (G % 128 == 0; else TILED runs) */
#define QUICK_KERNEL_XW 5     /* 256 x 256 / 128 x 256 / 128 x 128 / 64 x 128 tiles, four waves (one per SIMD) each owning all tokens and a quarter
                                 of the channels, generated hand-placed K loop; 1 / 2 / 4 K slices of a tile on different CUs exchange fp16
                                 parts and give up on partners that are not there (256 x 256: one slice)
                                 (G / 128 a power of two, N % 256 == 0 for the 256-channel tiles; else TILED runs) */

#define QUICK_KERNEL_LEAN 6   /* [r05] 1..16 tokens: one workgroup per 16 tokens x 16 channels, its waves split K; x by LDS-DMA FIRST in the
                                 memory queue, every weight tile of a wave requested up front, unit sums computed under the weights'
                                 flight (G % 128 == 0, K / 128 between waves and 16 * waves; else QUICK_ERR_UNSUPPORTED when forced) */
#define QUICK_KERNEL_XM 7     /* [r06] 17..128 tokens: one workgroup per 32 / 64 tokens x 32..96 channels for all of K, eight waves splitting K, each
                                 with its own x ring (LDS-DMA) and weight queue in a generated loop without barriers; every dequantised
                                 fragment feeds all token blocks (G a power-of-two multiple of 128, K / 128 >= 8) */

int quick_amd_abi_version(void);
const char* quick_amd_last_error(void);

/*
 * y[M, N] (fp16, row-major) = x[M, K] (fp16, row-major, contiguous) @ dequant(qweight, scales, qzeros)
 *
 *   qweight  int32 [K/4, N/2]   4-bit weights, MI355X order (DESIGN.md "Data layout")
 *   scales   fp16  [K/G, 2N]    as uint32 [K/G * N]: word ((n/16) * (K/G) + g) * 16 + n%16 = fp16 scale | zero point << 16
 *   qzeros   int32 [K/G, N/4]   plain copy of the zero points (nibble n%8 of dword n/8 of row g); not read by the GEMM
 *
 * Pointers: every tensor base 16-byte aligned (rows then are, N and K being multiples of 128); torch allocations are
 * 256-byte aligned.  The kernels move x, y, bias and the residual in 16-byte pieces.
 *
 * Dequantised weight = fp16((w - z) * s) exactly as the reference computes it
 * (csrc/dequantize_quick.cuh:15-63 + sub/mul.rn.f16x2 in csrc/gemm_cuda_quick.cu:52-60);
 * accumulation in fp32, one rounding to fp16 at the end.
 *
 * split_k_iters keeps the reference's argument (number of K slices, >= 1).  The reference uses it
 * as a tuning knob for NVIDIA parts; here it is validated and otherwise treated as a hint -- the
 * library picks its own K partitioning and always returns the fully reduced [M, N] result.
 *
 * Errors (mirroring csrc/gemm_cuda_quick.cu:1479-1484): N % 128 != 0 or N % 8 != 0 or
 * G % 32 != 0 -> QUICK_ERR_INVALID_ARGUMENT.  Additional envelope of this library:
 * K % 128 == 0 and K % G == 0 (every shape in BASELINE.json satisfies it) -> else QUICK_ERR_UNSUPPORTED.
 *
 * workspace: device scratch of at least quick_w4a16_workspace_bytes(...) bytes (may be NULL when
 * that function returns 0).  It must stay valid until the work enqueued on `hip_stream` completes,
 * must be ZERO-FILLED before its first use, and is handed back zero-filled where it matters -- layout:
 * [64 KiB arrival counters of the last-arriver split-K reduction, which reset themselves][16 MiB exchange
 * zone: the mailboxes through which the K slices of an exchange-K tile swap partial sums; every consumer
 * zeroes what it has read][fp32 partial tiles of the last-arriver kernels, overwritten before they are read]
 * -- so one zeroed buffer can be reused by every later call on the same stream, whatever its shape.  Do
 * not share it between streams that run concurrently.  (A launch that is aborted -- device reset --
 * may leave the first two regions dirty: zero the buffer again before reusing it.)
 * The K slices of a tile that meet through the exchange zone (QUICK_KERNEL_XK / QUICK_KERNEL_XW launches with more than
 * one slice) need NOT be co-resident since r04: a wave that has polled for a partner longer than the poll limit (41 us)
 * gives its part up -- own share to its self box, a flag bit in the part's state word in the counter region -- and leaves;
 * the partner whose shares reach memory last finds the flag, claims the part (the protocol's only atomic, a compare-and-swap) and
 * finishes it from the boxes.  The fast path writes no state word.  No kernel of the library spins without bound or traps.
 */
int quick_w4a16_gemm_f16(const void* x, const void* qweight, const void* scales, const void* qzeros,
                         void* y, void* workspace, size_t workspace_bytes,
                         int M, int K, int N, int group_size, int split_k_iters, void* hip_stream);

size_t quick_w4a16_workspace_bytes(int M, int K, int N, int group_size, int split_k_iters);

/* Is the workspace in the state every launch expects -- arrival counters, part state words and the exchange zone all-zero?  One pass
 * over the guarded regions (64 KiB + 16 MiB, or the whole buffer if smaller) on `hip_stream`, then a stream synchronise: QUICK_OK, or
 * QUICK_ERR_WORKSPACE with the first dirty byte offset in quick_amd_last_error().  Why it exists: the K slices of an exchange launch
 * hand their partial tiles over in 16-byte granules that are their own arrival flags (no dword of a payload granule is ever 0), and the
 * payload -- eight fp16 partial sums -- has no spare bits for a launch epoch; a separate epoch word per box would need the sender's
 * stores acknowledged before it may be written, the round trip the protocol exists to avoid.  So a granule left behind by an aborted
 * launch cannot be told from a partner's, and the contract is "zero between launches": the library keeps it on every path (also when
 * waves give up), this call verifies it, and QUICK_AMD_CHECK_WORKSPACE=1 in the environment runs it in front of every
 * launch that uses the regions (debugging: it synchronises).  Python: quick_amd.kernels zeroes its per-stream workspace again
 * whenever a launch returns an error.  The reference's split-K scratch + `.sum(0)` (csrc/gemm_cuda_quick.cu:1468,1515) holds no state
 * between launches; this is the price of reducing inside the launch. */
int quick_w4a16_workspace_check(const void* workspace, size_t workspace_bytes, void* hip_stream);

/* Same as quick_w4a16_gemm_f16 with an explicit kernel choice, an optional fp16 bias[N] added in the
 * epilogue (NULL = none; replaces the separate torch add of quick/awq/modules/linear/quick.py:165), and a
 * forced K split across workgroups (0 = heuristic).
 *
 * `kernel`: 0 = the library's planner (what every product path passes).  Otherwise, for tests and tuning, a
 * bit field -- every field 0 = "planner's choice within the family":
 *   bits 0-3    family, QUICK_KERNEL_*
 *   bits 4-7    SKINNY: channel tiles of 16 per workgroup (1, 2, 4; 8 = [r05] the straight-line eight-tile fragment kernel where it is built --
 *               9..16 tokens, G = 128, K / 128 = 8 waves x slices x {2, 4, 7, 8} k tiles, no RMSNorm prologue -- else 4; 7 = [r06] the same kernel with seven tiles per
 *               workgroup: K = 8192, one slice, N % 112 == 0 -- else 4); TILED: token tiles of 16 per workgroup (2, 4, 8);
 *               WIDE / XK / XW: token tiles of 32 per workgroup (WIDE 2, 4, 8; XK 2, 4; XW 2, 4, 8 -- 0 = 4; 8 = the 256 x 256 tile; [r06] WIDE 8 x 2 pairs runs
 *               128 x 256 tiles: r02's hipcc-scheduled 256 x 256 tile spilled registers and lives on in tools builds only);
 *               XM: 32-channel pairs per workgroup (1..3; 0 = the fewest that cover the layer in one round)
 *   bits 8-11   SKINNY / TILED / LEAN: waves per workgroup / 4 ([r06] SKINNY: sixteen waves only with one channel tile per workgroup); XM (bits 8-9): 1 = 32-token tiles, 2 = 64-token tiles; WIDE: 32-channel pairs per wave (1, 2); XK: K slices per tile (1, 2, 4, 8; 15 = half
 *               the planner's count); XW: K slices per tile (1, 2, 4 <= token tiles)
 *   bit 12      SKINNY: no LDS copy of x; WIDE: the double-buffered kernel at every tile size (no ring); XW: 128-channel tiles (implied by 2 token tiles)
 *   bit 13      TILED: retired in r06 (r01's 32x32x16 flavour: QUICK_ERR_INVALID_ARGUMENT)         bit 14  TILED / WIDE / XK: plain (not XCD-aware) tile order
 *   bit 15      TILED: 2 x 4 wave grid; WIDE: eight waves per workgroup (ring kernel)
 *   bits 16-20  timing experiments (wrong results on purpose, phase stamps): only in a QUICK_AMD_TOOLS build of the library
 *               (`python -m quick_amd.build --tools`); the product library answers QUICK_ERR_INVALID_ARGUMENT
 *   bit 21      SKINNY: flip the persistence default
 *   bits 22-24  SKINNY: persistent slots per CU; WIDE: LDS ring slots; XK: x ring slots; XW (bits 22-26): log2 of the exchange poll limit in
 *               ticks of 10 ns (0 = default 2^12; tests pass 1: every wave gives its part up at once)
 *   bit 25      SKINNY: exact per-weight dequantisation (no deferred zero point)
 *   bits 26-28  SKINNY: 26 force the table deferred-zero path, 28 no fragment deferred-zero path; TILED: 27 force 128 x 256
 *               four-wave tiles; XK: weight queue depth in stages (3..6)
 *               XW (bits 27-28): staggered K ranges of the two-slice 128 x 128 launch, d = 1..3 stages of 128 k -- each slice finishes the
 *               blocks it does not own 2 d stages early and mails them while it multiplies on for its own; needs G = 128,
 *               an even K / 128 and K / 256 - d >= 4, anything else is planned without it (plan_describe says `stagger=<d>` when taken)
 *   bits 29-30  TILED: force / forbid 256-channel tiles
 * Environment: QUICK_AMD_EXCHANGE_CUS=<n> -- a SPEED hint since r04: the K slices of an XK launch exchange fastest when tiles x slices
 * workgroups are co-resident, and the planner sizes the slice count for the device's CU count; a process whose queues see fewer CUs (a
 * CU mask) may say so (0: never split K this way).  Correctness does not depend on it: slices that are not there in time are given up
 * on and finished by the last arriver (see "workspace").  QUICK_AMD_EXCHANGE_POLL_LOG2=<n> overrides the poll limit (2^n ticks of 10 ns).
 * QUICK_AMD_XW256=0 -- the planner keeps r02's hipcc-scheduled kernel for the 256 x 256 tile (bit-identical results; the A/B switch).
 * A combination the library has no build for returns QUICK_ERR_UNSUPPORTED; results never depend on the field
 * beyond fp32 summation order (and bit 25's rounding). */
int quick_w4a16_gemm_f16_ex(const void* x, const void* qweight, const void* scales, const void* qzeros,
                            const void* bias, void* y, void* workspace, size_t workspace_bytes,
                            int M, int K, int N, int group_size, int kernel, int grid_split_k,
                            void* hip_stream);
size_t quick_w4a16_workspace_bytes_ex(int M, int K, int N, int group_size, int kernel, int grid_split_k);

/* What may be fused around the GEMM (all optional; zero-initialise the struct):
 *   rmsnorm_weight  fp16 [K]: the GEMM consumes RMSNorm(x) * weight (eps = rmsnorm_eps).  Where the kernel holds x whole
 *                   in LDS it normalises there with quick_rmsnorm_f16's rounding points (fp16(fp16(x * rstd) * weight));
 *                   where it takes x fragments straight from L2 (or from a per-wave LDS copy) it sums the rows' squares in
 *                   a pass in front of the K loop and normalises with the same rounding points (so no product of a massive
 *                   activation overflows and no row of tiny ones goes subnormal, as x * weight, raw, would).  Only where quick_w4a16_can_fuse_rmsnorm() says so (small-M kernels, K not
 *                   split across workgroups) -- QUICK_ERR_UNSUPPORTED otherwise (run quick_rmsnorm_f16 first).
 *   bias            fp16 [N]      (replaces the torch add of quick/awq/modules/linear/quick.py:165)
 *   residual        fp16 [M, N], may alias y: the decoder block's `hidden + proj(...)`
 *   silu_mul        output channels are gate/up interleaved in blocks of 8 (16t+i gate, 16t+8+i up, i < 8) and the
 *                   epilogue writes y[M, N/2] with y[m, 8t+i] = silu(gate) * up -- the intent of the reference's unused
 *                   QuantFusedMLP (quick/awq/modules/fused/mlp.py:52-71).  Excludes bias and residual.
 * The product (+ bias) is accumulated in fp32 and rounded to fp16 once; the residual is added to that rounded product and the sum
 * rounded again -- what GEMM-then-add computes, in every kernel family (silu_mul rounds gate, up and silu as torch does). */
typedef struct quick_gemm_fusion {
  const void* bias;
  const void* residual;
  const void* rmsnorm_weight;
  float rmsnorm_eps;
  int silu_mul;
} quick_gemm_fusion;
int quick_w4a16_gemm_f16_fused(const void* x, const void* qweight, const void* scales, const void* qzeros,
                               const quick_gemm_fusion* fusion, void* y, void* workspace, size_t workspace_bytes,
                               int M, int K, int N, int group_size, int kernel, int grid_split_k, void* hip_stream);
int quick_w4a16_can_fuse_rmsnorm(int M, int K, int N, int group_size);

/* What a launch of this shape will run, as one line of text (host-only, no GPU needed): kernel family, tile shape,
 * grid, K split and workspace, e.g. "tiled tokens=64 channels=128 waves=8 grid=256x1 ksplit=1 xcd_rows=2 workspace=0" or
 * "skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table grid=256x1x1 ksplit=1 workspace=0".  For logs and for tests of
 * the shape heuristics; the wording may grow fields, the leading family word will not change.  `kernel` and
 * `grid_split_k` as in quick_w4a16_gemm_f16_ex (0 = auto).  (No counterpart in the reference: its kernel has one shape.) */
int quick_w4a16_plan_describe(int M, int K, int N, int group_size, int kernel, int grid_split_k, char* text, size_t text_bytes);

/*
 * Measurement aid (bench.py): enqueue the GEMM `iters` times on `hip_stream`, cycling through `n_sets`
 * weight sets (host arrays of device pointers) so that consecutive launches do not hit in the 256 MiB
 * Infinity Cache, with a hipEvent pair bound to each main-kernel dispatch (hipExtLaunchKernelGGL);
 * synchronise, and write each dispatch's own duration in microseconds to the HOST array
 * kernel_us[iters].  Blocking; not part of the reference interface.
 */
int quick_w4a16_gemm_profile(const void* x, const void* const* qweights, const void* const* scales,
                             const void* const* qzeros, int n_sets, void* y, void* workspace,
                             size_t workspace_bytes, int M, int K, int N, int group_size, int kernel,
                             int grid_split_k, int iters, float* kernel_us, void* hip_stream);

/* Measurement aid: the IN-KERNEL wall-clock span of each of `iters` launches -- first wave's start to last wave's end on the
 * constant 100 MHz counter (s_memrealtime), written by the kernels themselves -- in microseconds to the HOST array
 * span_us[iters]; weight sets cycled as in quick_w4a16_gemm_profile.  The dispatch-duration clock reads ~4.2 us for an
 * EMPTY kernel, so launches of a few microseconds (small M) are only visible on this one.  Blocking. */
int quick_w4a16_gemm_span(const void* x, const void* const* qweights, const void* const* scales, const void* const* qzeros,
                          int n_sets, void* y, void* workspace, size_t workspace_bytes, int M, int K, int N, int group_size,
                          int kernel, int grid_split_k, int iters, float* span_us, void* hip_stream);

/* Measurement aid: the same event-pair clock on `iters` dispatches of an EMPTY kernel with the GEMM's launch
 * shape (256 workgroups x 512 threads): the fixed part of every "kernel duration" reading on this stack. */
int quick_amd_dispatch_floor(int iters, float* kernel_us, void* hip_stream);

/*
 * Decode-step glue around the GEMMs (callers of the hot path; counterparts of the out-of-tree kernels the
 * reference's fused runtime uses: awq_ext.layernorm_forward_cuda, quick/awq/modules/fused/norm.py:18;
 * awq_ft_ext.single_query_attention, quick/awq/modules/fused/attn.py:217).  fp16 tensors, fp32 arithmetic.
 *   quick_rmsnorm_f16          y[r,:] = x[r,:] * rsqrt(mean(x[r,:]^2) + eps) * weight
 *   quick_rope_kv_append_f16   one new token per sequence: rotate q, k of qkv[B, (nh+2nkv)*D] by table row *pos
 *                              (rotate-half convention), q -> q_out[B, nh, D], k/v -> caches [B, nkv, L, D] at *pos
 *   quick_decode_attention_f16 single-query attention over cache positions 0..*pos, GQA aware, D == 128
 *   quick_silu_mul_f16         y[m, 8t+i] = silu(gate_up[m, 16t+i]) * gate_up[m, 16t+8+i]  (gate/up interleaved by 8)
 * `pos` is a DEVICE pointer to one int64 (so a captured hipGraph can advance it); the caller keeps 0 <= *pos < cache_len
 * (a device value: the library cannot check it) and batch <= 65535.
 */
int quick_rmsnorm_f16(const void* x, const void* weight, void* y, int rows, int hidden, float eps, void* hip_stream);
int quick_rope_kv_append_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos,
                             void* q_out, void* k_cache, void* v_cache, int batch, int n_heads, int n_kv_heads,
                             int head_dim, int cache_len, void* hip_stream);
/* prefill form: `tokens` consecutive positions *pos0 .. per sequence; qkv [batch * tokens, (nh + 2 nkv) * D];
 * q_out [batch, nh, tokens, D] */
int quick_rope_kv_write_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out,
                            void* k_cache, void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                            int cache_len, void* hip_stream);
/* per-sequence form: pos0 is a DEVICE pointer to int64 [batch]; token t of sequence b sits at position pos0[b] + t.  A sequence with
 * pos0[b] outside 0 .. cache_len - tokens is SKIPPED: its rows of q_out and of the caches are left untouched and no address outside the
 * buffers is formed (an idle slot of a serving loop).  The same checks and error codes as quick_rope_kv_write_f16. */
int quick_rope_kv_write_seq_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out,
                                void* k_cache, void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                                int cache_len, void* hip_stream);
int quick_decode_attention_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos, void* out,
                               int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale,
                               void* hip_stream);
/* quick_rope_kv_append_f16 + quick_decode_attention_f16 in one launch, reading the qkv GEMM output directly.  One online-softmax sweep
 * over the cache, software-pipelined (r05); rows at or behind *pos may hold anything (they are never read into a sum).  Grouped-query
 * models with >= 256 (sequence, KV head) pairs and 4 or 8 query heads per KV head take their scores from the matrix core
 * (v_mfma_f32_16x16x32_f16 on 16 cache rows x the heads of the group); QUICK_AMD_ATTN_MFMA=0 keeps the vector-ALU sweep (A/B switch,
 * same results within fp32 summation order). */
int quick_decode_rope_attention_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos,
                                    void* k_cache, void* v_cache, void* out, int batch, int n_heads, int n_kv_heads,
                                    int head_dim, int cache_len, float scale, void* hip_stream);
/* per-sequence form: pos is a DEVICE pointer to int64 [batch].  Sequence b rotates with table row pos[b], appends k and v at cache row
 * pos[b] and attends rows 0 .. pos[b]; its workgroups sweep its own length only, so a mixed batch costs its own rows, not batch times
 * the longest.  The kernel is chosen as for the shared form (by batch, head counts and cache_len, never by a position), and a
 * workgroup's arithmetic is the shared launch's at *pos = pos[b], bit for bit.  A sequence with pos[b] outside 0 .. cache_len - 1 is
 * SKIPPED: its cache rows and its row of out are left untouched (an idle slot).  The same checks and error codes as the shared form;
 * quick_decode_rope_attention_describe serves both. */
int quick_decode_rope_attention_seq_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos,
                                        void* k_cache, void* v_cache, void* out, int batch, int n_heads, int n_kv_heads,
                                        int head_dim, int cache_len, float scale, void* hip_stream);
/* Which kernel quick_decode_rope_attention_f16 launches for this shape, as one line of text (host-only, no GPU needed): the kernel
 * ("flash", "gqa" = the vector-ALU grouped-query sweep, "gqa-mfma"), query heads per workgroup, workgroups per KV head, waves per
 * workgroup, cache rows per register set and the grid, e.g. "gqa-mfma heads=8 gsplit=1 waves=4 set_rows=64 grid=8x32".  The same
 * refusals as the launch.  For logs and for tests of the dispatch; the wording may grow fields, the leading kernel word will not change. */
int quick_decode_rope_attention_describe(int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len, char* text,
                                         size_t text_bytes);
/* Causal attention of `tokens` new tokens per sequence over the KV cache (prefill from any position: first prompt, second chat turn,
 * chunked prefill, speculative verify), D == 128, GQA aware, one launch.
 *   q        [batch, n_heads, tokens, D]: what quick_rope_kv_write_f16 writes to q_out
 *   caches   [batch, n_kv_heads, cache_len, D]; rows *pos0 .. *pos0 + tokens - 1 already written (by that same call).  Read, never written.
 *   pos0     DEVICE pointer to one int64 (no host read: the launch can be captured); the caller keeps 0 <= *pos0, *pos0 + tokens <= cache_len
 *   out      [batch * tokens, n_heads * D], row b * tokens + t: the matrix o_proj's GEMM consumes
 * Query t attends cache rows 0 .. *pos0 + t and nothing else.  Rows at or behind *pos0 + tokens may hold anything (NaN, +-Inf): they are
 * never read.  Online softmax, no score matrix in memory, no workspace, no atomics.  Both products run on the matrix core
 * (v_mfma_f32_16x16x32_f16) with fp32 accumulation; scores, running max and running sum in fp32; THE WEIGHTS P ARE ROUNDED TO FP16 as the
 * operand of the second product; one fp32 division and one rounding to fp16 at the end.
 * Answered before any GPU work, with a sentence in quick_amd_last_error():
 *   a null pointer; batch, tokens, n_heads, n_kv_heads or cache_len <= 0; tokens > cache_len     QUICK_ERR_INVALID_ARGUMENT
 *   head_dim != 128; n_heads % n_kv_heads != 0; n_heads or batch > 65535 (grid dimensions)        QUICK_ERR_UNSUPPORTED */
int quick_prefill_attention_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, void* hip_stream);
/* per-sequence form: pos0 is a DEVICE pointer to int64 [batch]; query t of sequence b attends cache rows 0 .. pos0[b] + t, and rows at or
 * behind pos0[b] + tokens of THAT sequence are never read.  A sequence with pos0[b] outside 0 .. cache_len - tokens is SKIPPED: its rows
 * of out are left untouched (the shared form pulls such a value inside instead).  The same refusals and error codes as
 * quick_prefill_attention_f16; quick_prefill_attention_describe serves both. */
int quick_prefill_attention_seq_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                    int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, void* hip_stream);
/* The launch of quick_prefill_attention_f16 for this shape as one line of text (host-only, no GPU needed): the kernel word, query rows
 * per workgroup, cache rows per tile, waves and the grid, e.g. "prefill-mfma q_rows=64 kv_rows=32 waves=4 grid=2x32x64".  The same
 * refusals as the launch (the pointers aside).  The wording may grow fields, the leading kernel word will not change. */
int quick_prefill_attention_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, char* text,
                                     size_t text_bytes);
/*
 * One-byte KV cache (opt-in; the fp16 entry points above are unchanged).  k_cache, v_cache: [batch, n_kv_heads, cache_len, 128], one byte
 * per element, OCP e4m3fn (never the fnuz encoding).  One scale per cache, k_scale and v_scale: HOST floats, finite and > 0, constants
 * of a captured graph.
 *   stored byte        rne_e4m3(clamp(float(h) * inv, -448, 448)): h is the fp16 value the fp16 launch stores at that place (rotated K
 *                      rounded to fp16 exactly as there, V copied), inv = 1.0f / scale computed once on the host in fp32.  The clamp is
 *                      explicit (no conversion mode is relied on); NaN stays NaN (a NaN code).
 *   dequantised value  float(byte) * scale.  The kernels fold the scales out of their sweeps: k_scale into the fp32 score factor
 *                      scale * log2 e * k_scale, v_scale into the one fp32 multiply at the final division.  Inside the loops a byte
 *                      becomes its exact fp16 value and nothing else; both MFMA products keep fp16 operands.
 *   rows outside       rows at or behind a sequence's position may hold ANY byte (the NaN codes 0x7F / 0xFF included): they reach neither
 *                      scores nor the value sum.
 * per_sequence (the last int of each launch; one symbol serves both forms): 0 -- pos / pos0 is a DEVICE pointer to one int64 shared by
 * the batch; non-zero -- to int64 [batch], with the skip rule of the _seq_f16 launches (a sequence whose position lies outside the valid
 * range is left untouched: caches, q_out and out).
 * Every entry point answers before any GPU work, with a sentence in quick_amd_last_error() -- shape rules first, then the scales, then
 * the pointers:
 *   quick_rope_kv_write_fp8           sizes <= 0, n_heads % n_kv_heads != 0                      QUICK_ERR_INVALID_ARGUMENT
 *                                     head_dim != 128, batch * tokens > 65535                    QUICK_ERR_UNSUPPORTED
 *   quick_decode_rope_attention_fp8   sizes <= 0, head_dim != 128, n_heads % n_kv_heads != 0,
 *                                     a group other than 1, 2, 4, 8, batch > 65535              QUICK_ERR_UNSUPPORTED
 *   quick_prefill_attention_fp8       sizes <= 0, tokens > cache_len                             QUICK_ERR_INVALID_ARGUMENT
 *                                     head_dim != 128, n_heads % n_kv_heads != 0, grid limits    QUICK_ERR_UNSUPPORTED
 *   all three                         a scale that is not finite and positive; a null pointer or one that is not 16-byte aligned
 *                                     (pos / pos0: 8-byte)                                       QUICK_ERR_INVALID_ARGUMENT
 * (the codes of the fp16 siblings, which accept other head dims in the write and do not look at pointers).
 */
/* quick_rope_kv_write_f16 for byte caches: RoPE on q and k of tokens >= 1 tokens per sequence; q_out [batch, n_heads, tokens, 128] in
 * fp16, bit for bit what the fp16 launch writes; K and V rows stored as bytes in 8-byte pieces. */
int quick_rope_kv_write_fp8(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_cache,
                            void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float k_scale,
                            float v_scale, int per_sequence, void* hip_stream);
/* quick_decode_rope_attention_f16 for byte caches: RoPE, append of the new token's K and V bytes at row *pos, single-query attention over
 * rows 0 .. *pos.  1, 2, 4 or 8 query heads per KV head, a KV head's whole group served from ONE sweep of its rows (scores on
 * v_mfma_f32_16x16x32_f16, 16 elements per 16-byte request, software-pipelined).  The new token takes part in its own step with its
 * QUANTISED-then-dequantised K and V: step p attends exactly what step p + 1 reads from the cache. */
int quick_decode_rope_attention_fp8(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_cache,
                                    void* v_cache, void* out, int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len,
                                    float scale, float k_scale, float v_scale, int per_sequence, void* hip_stream);
/* The launch of quick_decode_rope_attention_fp8 for this shape as one line (host-only), e.g. "gqa-mfma-fp8 heads=4 gsplit=1 waves=4
 * set_rows=64 grid=8x64": the build is chosen by the group alone.  The same shape refusals as the launch. */
int quick_decode_rope_attention_fp8_describe(int batch, int n_heads, int n_kv_heads, int head_dim, int cache_len, char* text,
                                             size_t text_bytes);
/* quick_prefill_attention_f16 over byte caches: the same tiling, masking, online softmax, rounding points and way out; only the staging
 * differs (half the bytes per request, converted to fp16 on the way into the same LDS images).  One build: no describe of its own,
 * quick_prefill_attention_describe gives the grid. */
int quick_prefill_attention_fp8(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch, int tokens,
                                int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, float k_scale, float v_scale,
                                int per_sequence, void* hip_stream);
/*
 * Sliding-window attention over a RING KV cache, fp16 (opt-in; every entry point above is unchanged).  The query at position p attends
 * positions max(0, p - window + 1) .. p.  k_cache, v_cache: [batch, n_kv_heads, ring_rows, 128] fp16; position j lives in cache row
 * j % ring_rows, so cache memory and the decode sweep are bounded by the window, not by the context.  Keys keep the RoPE of their own
 * ABSOLUTE position: nothing is re-labelled when the window moves.
 *   R = ring_rows   rows of the cache tensors
 *   W = window      W <= R
 *   table_rows      rows of the cos / sin tables: the exclusive bound on positions
 * Ring rule.  A chunk of T tokens is written before it is attended and overwrites the rows of positions <= pos0 + T - 1 - R.  With
 * W + T - 1 <= R the oldest position any query of the chunk attends, pos0 - W + 1, lies in front of that: no attended row has been
 * overwritten.  A ring that can never wrap, R >= table_rows, takes any T <= R.
 * Never read.  Every cache row that holds no position inside [window start of the launch's first query, last written position] -- rows
 * not yet written before the first wrap, stale rows of positions in front of the window after it -- may hold anything, NaN keys and
 * +-Inf values included.  Positions inside that span but outside a given query's own window are requested (they are finite) and masked
 * by the row index before the max and the exp, as the causal diagonal is.  The prefill launch never writes a cache; the decode launch
 * writes row *pos % R and nothing else.
 * Rounding points: those of quick_decode_rope_attention_f16's grouped MFMA sweep (fp32 scores, max, sum and P V; one division and one
 * rounding at the end) and of quick_prefill_attention_f16 (P rounded to fp16 as the operand of the second product).
 * per_sequence, as in the fp8 launches: 0 -- pos / pos0 is a DEVICE pointer to one int64 shared by the batch (a value outside the valid
 * range is pulled inside); non-zero -- to int64 [batch], and a sequence whose position lies outside the valid range is skipped and left
 * untouched: caches, q_out and out.  Valid: pos0 in 0 .. table_rows - tokens, *pos in 0 .. table_rows - 1.
 * The prefill launch and the describe take table_rows too: the ring rule and the skip rule cannot be stated without it.
 * Every entry point answers before any GPU work, with a sentence in quick_amd_last_error(), in this order:
 *   a size <= 0, window < 1, window > ring_rows, tokens > ring_rows, tokens > table_rows                 QUICK_ERR_INVALID_ARGUMENT
 *   window + tokens - 1 > ring_rows while ring_rows < table_rows (attention launches and the describe)    QUICK_ERR_INVALID_ARGUMENT
 *   head_dim != 128, n_heads % n_kv_heads != 0, decode: a group other than 1, 2, 4, 8                     QUICK_ERR_UNSUPPORTED
 *   a grid limit (write: batch * tokens > 65535; attention: batch or n_heads > 65535)                     QUICK_ERR_UNSUPPORTED
 *   a null pointer                                                                                        QUICK_ERR_INVALID_ARGUMENT
 */
/* quick_rope_kv_write_f16 into the ring: token t is rotated with table row pos0 + t and its K and V are stored at cache row
 * (pos0 + t) % ring_rows.  q_out and the stored rows are bit for bit what quick_rope_kv_write_f16 writes (at row pos0 + t of a linear
 * cache) for the same qkv and position. */
int quick_rope_kv_write_win_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_cache,
                                void* v_cache, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows,
                                int table_rows, int per_sequence, void* hip_stream);
/* One launch: RoPE at *pos, append at cache row *pos % ring_rows, single-query attention over positions max(0, *pos - window + 1) ..
 * *pos; the new token comes from registers.  1, 2, 4 or 8 query heads per KV head, a KV head's whole group served from ONE sweep with
 * the scores on v_mfma_f32_16x16x32_f16.  The sweep runs over logical positions: the window start is reduced modulo ring_rows once per
 * workgroup, every further row is a compare and a subtract. */
int quick_decode_rope_attention_win_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_cache,
                                        void* v_cache, void* out, int batch, int n_heads, int n_kv_heads, int head_dim, int ring_rows,
                                        int window, int table_rows, float scale, int per_sequence, void* hip_stream);
/* quick_prefill_attention_f16 with a window over the ring: query t attends positions max(0, pos0 + t - window + 1) .. pos0 + t, whose
 * rows quick_rope_kv_write_win_f16 has written.  Tiling, LDS images, online softmax, rounding points and the way out are that kernel's;
 * a workgroup starts at the tile that holds the window start of its first query, and the lower diagonal is masked like the upper one.
 * out: [batch * tokens, n_heads * 128]. */
int quick_prefill_attention_win_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                    int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows, int window, int table_rows,
                                    float scale, int per_sequence, void* hip_stream);
/* The windowed attention launch for this shape as one line (host-only): tokens == 1 describes the decode launch ("decode-win-mfma
 * heads=4 waves=4 set_rows=64 ring_rows=4607 window=4096 grid=8x64"), more tokens the prefill launch ("prefill-win-mfma q_rows=64
 * kv_rows=32 waves=4 ...").  The same shape refusals as the launches. */
int quick_attention_win_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int ring_rows, int window,
                                 int table_rows, char* text, size_t text_bytes);
/*
 * Attention over a PAGED KV cache, fp16 (opt-in; every entry point above is unchanged).  Cache memory is a pool of fixed-size pages and a
 * block table per sequence, so a batch is charged for the tokens alive, not for batch * the longest context.
 *   k_pool, v_pool  [num_pages, n_kv_heads, page_size, 128] fp16: a page holds page_size consecutive positions of ONE sequence, for all
 *                   KV heads
 *   P = page_size   32, 64, 128 or 256: whole multiples of the decode sweep's 16-row chunk and of the prefill kernel's 32-row tile, so
 *                   a chunk or a tile never straddles a page and the table is read once per chunk or tile, wave-uniform
 *   block_table     DEVICE int32 [batch, max_pages]: block_table[b][i] is the pool page of positions i P .. i P + P - 1 of sequence b;
 *                   position j of sequence b, KV head h, lives at pool row (block_table[b][j / P], h, j % P)
 *   table_rows      rows of the cos / sin tables; positions are bounded (exclusive) by min(table_rows, max_pages * P)
 * Keys keep the RoPE of their absolute position; the rounding points are those of the linear launches, operation for operation: on the
 * gathered linear cache the results are bit for bit those of quick_rope_kv_write_f16, of the grouped MFMA decode sweep
 * (quick_decode_rope_attention_win_f16 with ring_rows = window = table_rows) and of quick_prefill_attention_f16.
 * Never read.  Every request is clamped, as a logical position, to [0, last written position] before it is mapped: table columns behind
 * the last written position's page and pool pages named by no needed column are never read and may hold anything (-1; NaN keys, +-Inf
 * values).  The prefill launch never writes the pool; the decode launch writes this token's row and nothing else.
 * A needed entry outside 0 .. num_pages - 1: a write (the write launch, the decode launch's append) drops that row; a read stays inside
 * the pool (decode: the id is pulled inside; prefill: the tile is taken as zeros and nothing is requested).  No address ever leaves the
 * pool and no other sequence's page is written, whatever the table holds; that sequence's output is unspecified.  The same page id may
 * stand in several sequences' rows (a shared prefix); keeping writers apart is the caller's business.
 * per_sequence, as in the window launches: 0 -- pos / pos0 is a DEVICE pointer to one int64 shared by the batch (a value outside the
 * valid range is pulled inside); non-zero -- to int64 [batch], and a sequence whose position lies outside the valid range is skipped and
 * left untouched: pool, q_out and out.  Valid: pos0 in 0 .. bound - tokens, *pos in 0 .. bound - 1, bound = min(table_rows, max_pages * P).
 * Every entry point answers before any GPU work, with a sentence in quick_amd_last_error(), in this order:
 *   a size <= 0 (batch, tokens, n_heads, n_kv_heads, num_pages, page_size, max_pages, table_rows)         QUICK_ERR_INVALID_ARGUMENT
 *   page_size not 32, 64, 128 or 256; tokens > table_rows; max_pages * page_size < tokens                  QUICK_ERR_INVALID_ARGUMENT
 *   head_dim != 128, n_heads % n_kv_heads != 0, decode: a group other than 1, 2, 4, 8                     QUICK_ERR_UNSUPPORTED
 *   a grid limit (write: batch * tokens > 65535; attention: batch or n_heads > 65535)                     QUICK_ERR_UNSUPPORTED
 *   a null pointer                                                                                        QUICK_ERR_INVALID_ARGUMENT
 */
/* quick_rope_kv_write_f16 into the pool: token t is rotated with table row pos0 + t and its K and V are stored at pool row
 * (block_table[b][(pos0 + t) / P], kvh, (pos0 + t) % P).  q_out and the stored rows are bit for bit what quick_rope_kv_write_f16 writes
 * (at row pos0 + t of a linear cache) for the same qkv and position. */
int quick_rope_kv_write_paged_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos0, void* q_out, void* k_pool,
                                  void* v_pool, const void* block_table, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                                  int num_pages, int page_size, int max_pages, int table_rows, int per_sequence, void* hip_stream);
/* One launch: RoPE at *pos, append at this token's page and row, single-query attention over positions 0 .. *pos; the new token comes
 * from registers.  1, 2, 4 or 8 query heads per KV head, a KV head's whole group served from ONE sweep with the scores on
 * v_mfma_f32_16x16x32_f16: one workgroup per (sequence, KV head), 16-row chunks per wave, one table read per chunk. */
int quick_decode_rope_attention_paged_f16(const void* qkv, const void* cos_table, const void* sin_table, const void* pos, void* k_pool,
                                          void* v_pool, void* out, const void* block_table, int batch, int n_heads, int n_kv_heads,
                                          int head_dim, int num_pages, int page_size, int max_pages, int table_rows, float scale,
                                          int per_sequence, void* hip_stream);
/* quick_prefill_attention_f16 over the pool: query t attends positions 0 .. pos0 + t, whose rows quick_rope_kv_write_paged_f16 has
 * written.  Tiling, LDS images, online softmax, rounding points and the way out are that kernel's; each 32-row tile is fetched through
 * the table.  out: [batch * tokens, n_heads * 128]. */
int quick_prefill_attention_paged_f16(const void* q, const void* k_pool, const void* v_pool, const void* pos0, void* out,
                                      const void* block_table, int batch, int tokens, int n_heads, int n_kv_heads, int head_dim,
                                      int num_pages, int page_size, int max_pages, int table_rows, float scale, int per_sequence,
                                      void* hip_stream);
/* The paged attention launch for this shape as one line (host-only): tokens == 1 describes the decode launch ("decode-paged-mfma heads=4
 * waves=4 set_rows=64 page_size=64 max_pages=64 grid=8x16"), more tokens the prefill launch ("prefill-paged-mfma q_rows=64 kv_rows=32
 * waves=4 page_size=64 max_pages=64 grid=2x32x16").  The same shape refusals as the launches. */
int quick_attention_paged_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int num_pages, int page_size,
                                   int max_pages, int table_rows, char* text, size_t text_bytes);
int quick_silu_mul_f16(const void* gate_up, void* y, int rows, int intermediate, void* hip_stream);

/* lm_head of a decode step with the greedy arg-max folded in (the reference: torch linear + max on the fp16 layer AWQ leaves
 * unquantised, examples/benchmark.py:54-57): h = RMSNorm(x[batch, hidden]) * norm_weight (quick_rmsnorm_f16's rounding; norm_weight
 * may be null: h = x), logits[b, v] = h[b, :] . weight[v, :] (fp16 [vocab, hidden], fp32 sums, rounded to fp16),
 * next_token[b] (int64) = the lowest index among the largest fp16 logits.  hidden_out [batch, hidden] and logits [batch, vocab]
 * are optional outputs (null: not written).  batch <= 4, hidden % 512 == 0, batch * hidden <= 36864; QUICK_ERR_UNSUPPORTED
 * otherwise (the caller falls back to its GEMM library).  workspace: quick_lm_head_workspace_bytes(batch), any content. */
size_t quick_lm_head_workspace_bytes(int batch);
int quick_lm_head_argmax_f16(const void* x, const void* norm_weight, float eps, const void* weight, void* hidden_out, void* logits,
                             void* next_token, void* workspace, size_t workspace_bytes, int batch, int vocab, int hidden,
                             void* hip_stream);

#ifdef QUICK_AMD_TOOLS /* only in `python -m quick_amd.build --tools` libraries (libquick_amd_tools.so) */
/* Measurement aid (tools/prefetch_probe.py): pull [ptr, ptr + bytes) through HBM into the memory-side cache -- one
 * dword read per 128-byte line, results unused -- with `workgroups` (low 16 bits; 0 = 64) workgroups of 256 threads; bits 16..
 * choose the touch density (0 / 1: one dword per line, 2, 4, 32 = every byte).  No library path calls it. */
int quick_prefetch(const void* ptr, size_t bytes, int workgroups, void* hip_stream);
#endif

/*
 * Format bridge.  "cuda order" is byte-for-byte what the reference's WQLinear_QUICK.from_linear
 * writes (quick/awq/modules/linear/quick.py:88-150) and what its checkpoints hold; "mi355x order"
 * is what quick_w4a16_gemm_f16 consumes.  All six buffers have the reference's shapes; in and out
 * must not alias.
 */
int quick_repack_cuda_to_mi355x(const void* qweight_in, const void* scales_in, const void* qzeros_in,
                                void* qweight_out, void* scales_out, void* qzeros_out,
                                int K, int N, int group_size, void* hip_stream);
int quick_repack_mi355x_to_cuda(const void* qweight_in, const void* scales_in, const void* qzeros_in,
                                void* qweight_out, void* scales_out, void* qzeros_out,
                                int K, int N, int group_size, void* hip_stream);

/* in_features that the MI355X weight order cannot tile (K % 128 != 0; the reference accepts K % 32 == 0,
 * csrc/gemm_cuda_quick.cu:1479-1484 -- only possible with a group size that is not a multiple of 128): the layer runs on a copy
 * padded along K to quick_padded_in_features(K, G) = the next multiple of lcm(128, G), with weights 0, zero points 0 and
 * scales 0 in the added rows / groups (they contribute exactly 0), and on activations zero-padded to that width by the
 * caller.  quick_repack_cuda_to_mi355x_padded writes that copy: outputs are sized for the padded K
 * (qweight [Kp/4, N/2], scales [Kp/G, 2N], qzeros [Kp/G, N/4]).  quick_padded_in_features returns 0 for shapes the
 * reference rejects too. */
int quick_padded_in_features(int K, int group_size);
int quick_repack_cuda_to_mi355x_padded(const void* qweight_in, const void* scales_in, const void* qzeros_in, void* qweight_out,
                                       void* scales_out, void* qzeros_out, int K, int N, int group_size, void* hip_stream);

/*
 * GEMM-format bridge: AWQ checkpoints in the packing of WQLinear_GEMM (quick/awq/modules/linear/gemm.py:29-63, 108-143) <-> mi355x
 * order.  Both hold the same (iw[K, N], z[K/G, N], s[K/G, N]); the conversion is a permutation of bits, lossless in both directions.
 * The GEMM packing in closed form, order = {0, 2, 4, 6, 1, 3, 5, 7}:
 *   qweight  int32 [K, N/8]     nibble i of dword c of row k = iw[k, 8c + order[i]]
 *   qzeros   int32 [K/G, N/8]   nibble i of dword c of row g = z[g, 8c + order[i]]
 *   scales   fp16  [K/G, N]     plain, not duplicated
 * quick_repack_awq_gemm_to_mi355x always writes Kp = quick_padded_in_features(K, G) rows (Kp == K when K % 128 == 0): outputs are
 * qweight [Kp/4, N/2], scales [Kp/G, 2N], qzeros [Kp/G, N/4]; rows at or beyond K hold weight 0, groups at or beyond K/G scale 0 and
 * zero point 0.  quick_repack_mi355x_to_awq_gemm is the inverse for K % 128 == 0 (a padded copy is never turned back); it reads the
 * zero points from the scale words (qzeros_in is not read).  Inputs and outputs must not alias.
 * Answered before any GPU work, with a sentence in quick_amd_last_error():
 *   K, N or G <= 0, N % 8 != 0, G % 32 != 0, K % G != 0, K % 32 != 0, a null pointer   QUICK_ERR_INVALID_ARGUMENT
 *   N % 128 != 0 (the GEMM kernels' envelope)                                            QUICK_ERR_UNSUPPORTED
 *   K % 128 != 0, mi355x -> GEMM packing only                                            QUICK_ERR_UNSUPPORTED
 */
int quick_repack_awq_gemm_to_mi355x(const void* qweight_in, const void* qzeros_in, const void* scales_in,
                                    void* qweight_out, void* scales_out, void* qzeros_out,
                                    int K, int N, int group_size, void* hip_stream);
int quick_repack_mi355x_to_awq_gemm(const void* qweight_in, const void* scales_in, const void* qzeros_in,
                                    void* qweight_out, void* qzeros_out, void* scales_out,
                                    int K, int N, int group_size, void* hip_stream);

/*
 * gate_proj and up_proj of an MLP <-> the one layer the silu_mul epilogue of quick_w4a16_gemm_f16_fused reads, whose 2 * I output
 * channels interleave gate and up in blocks of 8: fused channel 16t + i = gate channel 8t + i, fused channel 16t + 8 + i = up channel
 * 8t + i (i < 8).  Everything is in mi355x order, where the interleave moves whole 16-byte pieces and no nibble changes place:
 *   per projection   qweight [K/4, I/2]   scales [K/G, 2I]   qzeros [K/G, I/4]
 *   fused            qweight [K/4, I]     scales [K/G, 4I]   qzeros [K/G, I/2]
 * quick_split_gate_up_mi355x is the exact inverse (saving).  One launch each, 16-byte loads and stores, every output byte written
 * once -- the second half of every qzeros row, which holds no channels, as 0 -- with no atomics, memset or LDS.  Inputs and outputs
 * must not alias; every pointer must be 16-byte aligned.  Answered before any GPU work, with a sentence in quick_amd_last_error():
 *   K, I or G <= 0, G % 32 != 0, K % G != 0, I % 8 != 0, a null or misaligned pointer    QUICK_ERR_INVALID_ARGUMENT
 *   K % 128 != 0 (a padded layer has no mi355x order of its own), I % 64 != 0            QUICK_ERR_UNSUPPORTED
 * (2 * I % 128 == 0 is the GEMM kernels' rule for the fused layer's width; the shape rules are answered before the pointers are looked at).
 */
int quick_interleave_gate_up_mi355x(const void* gate_qweight, const void* gate_scales, const void* gate_qzeros,
                                    const void* up_qweight, const void* up_scales, const void* up_qzeros,
                                    void* qweight_out, void* scales_out, void* qzeros_out,
                                    int K, int I, int group_size, void* hip_stream);
int quick_split_gate_up_mi355x(const void* qweight_in, const void* scales_in, const void* qzeros_in,
                               void* gate_qweight, void* gate_scales, void* gate_qzeros,
                               void* up_qweight, void* up_scales, void* up_qzeros,
                               int K, int I, int group_size, void* hip_stream);

/* Dequantise an MI355X-order layer to a dense fp16 [K, N] row-major matrix (debug / parity aid;
 * counterpart of the reference CPU path quick/awq/utils/packing_utils.py:82-97). */
int quick_dequantize_mi355x_f16(const void* qweight, const void* scales, const void* qzeros,
                                void* w_out, int K, int N, int group_size, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* QUICK_AMD_H */
