// GEMM planner (host code only): what every W4A16 launch runs.  make_plan is a sequence of steps in the order they decide -- the small-M
// families (lean, mid-token), AUTO's family pick (rules, launch-time models, corrections), the limits of the picked kernel, then the
// family's own geometry.
#include "w4a16_plan.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "w4a16_lean_host.hpp"
#include "w4a16_xm_host.hpp"

namespace quick_amd {

// compute units of the current device (256 on MI355X); 256 when there is no device to ask (plan_describe on a CPU-only host)
static int cu_count() {
  static thread_local int cached_dev = -2, cached = 256;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 256;
  }
  if (dev != cached_dev) {
    int n = 0;
    cached = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    (void)hipGetLastError();
    cached_dev = dev;
  }
  return cached;
}
// CUs the K slices of an exchange-K launch may count on being CO-RESIDENT.  The slices of a tile poll each other's mailboxes: a launch
// whose workgroups cannot all run at once (a CU mask on the queue, CUs reserved by the runtime) would spin until the poll limit traps.
// The device attribute does not see such masks; QUICK_AMD_EXCHANGE_CUS=<n> tells the planner (0: never split K across CUs that way).
static int exchange_cus() {
  static const int env = [] {
    const char* e = getenv("QUICK_AMD_EXCHANGE_CUS");
    return e && *e ? std::max(0, atoi(e)) : -1;
  }();
  return env >= 0 ? std::min(env, cu_count()) : cu_count();
}

// One planning request: the shape, the decoded kernel id, and the byte counts the 32-bit buffer offsets limit
struct Req {
  int M, K, N, G, KT, grid_split_k;
  KernelId id;
  bool bare;  // AUTO with no field set (kernel id 0)
  bool allow_xk, with_ln;
  size_t x_bytes, y_bytes, w_bytes;
};

// Whether ceil-dividing K into s slices gives exactly s non-empty ones
static bool splits_evenly(int KT, int s) { return (KT + (KT + s - 1) / s - 1) / ((KT + s - 1) / s) == s; }
// 32-bit buffer offsets: the lean / mid-token kernels (< 2 GiB of weights and of x) and the wide / exchange-K / four-wave kernels (< 4 GiB of x and of y)
static bool offsets31(const Req& r) { return r.w_bytes < ((size_t)1 << 31) && r.x_bytes < ((size_t)1 << 31); }
static bool offsets32(const Req& r) { return r.x_bytes < ((size_t)1 << 32) && r.y_bytes < ((size_t)1 << 32); }
// G a power-of-two multiple of 128 (the loops shift the k tile by log2(G / 128))
static bool pow2_groups(int G) { return G % 128 == 0 && ((G / 128) & (G / 128 - 1)) == 0; }
// XCD-aware tile order: the rows gm of a gm x (groups / gm) grid of XCDs over the MBk x NBk tiles that minimises what each XCD's L2 has to
// fetch, (MBk / gm) token blocks of x_cost plus (NBk * gm / groups) channel blocks of w_cost; 0 = plain order
static int xcd_rows(const Req& r, long workgroups, int MBk, int NBk, int groups, long x_cost, long w_cost) {
  int rows = 0;
  long best = -1;
  if (r.id.plain_order || workgroups % 8 != 0) return 0;
  for (int gm = 1; gm <= groups; gm *= 2) {
    if (MBk % gm != 0 || NBk % (groups / gm) != 0) continue;
    const long cost = (long)(MBk / gm) * x_cost + (long)(NBk * gm / groups) * w_cost;
    if (best < 0 || cost < best) {
      best = cost;
      rows = gm;
    }
  }
  return rows;
}
// K slices of a wide launch: as many as keep the workgroups within one round of 256 and the slices >= 4 stages -- any count,
// not only powers of two (80 tiles run 3 slices = 240 workgroups; Llama-2-13B's N = 5120 is 40 / 80 tiles wide)
static int wide_split(int KT, long tiles) { return (int)std::max<long>(1, std::min<long>(256 / std::max<long>(1, tiles), KT / 4)); }

// [r05] lean small-M kernels (w4a16_lean.hpp): one workgroup per 16 tokens x (ntw x 16) channels, `waves` waves split K and request all
// their k tiles up front.  Forced: family LEAN, bits 8-11 waves / 4 (1, 2, 4; 0 = choose), bits 4-7 channel tiles per workgroup (1, 2;
// 0 = choose).  AUTO takes them for 1..4 tokens wherever a build exists, and up to 16 tokens on layers of <= 512 channel blocks -- each
// workgroup fetches its own copy of x, which at 8..16 tokens on a wide layer is more L2 -> LDS traffic than the weights
// [profiles/r05_lean_sweep.txt: in-kernel spans against the r01-r04 skinny kernels, one session: 1 x 4096 x 4096 4.81 -> 3.65 us, 8 x: 5.28 ->
// 4.08, 16 x: 6.48 -> 4.58; 1 x 4096 x 12288 7.83 -> 6.77, 1 x 4096 x 22016 11.56 -> 10.64, 1 x 11008 x 4096 8.13 -> 7.00, 1 x 8192 x 8192 9.65 -> 8.36;
// 8 x 4096 x 22016 13.6 -> 15.1 and 16 x 4096 x 12288 9.9 -> 10.7 stay with the old kernels].
static bool plan_lean(const Req& r, Plan& p) {
  static const int builds[7][3] = {{8, 4, 1}, {8, 4, 2}, {8, 8, 1}, {8, 12, 1}, {16, 4, 1}, {16, 4, 2}, {16, 8, 1}};
  const int M = r.M, K = r.K, N = r.N, G = r.G, KT = r.KT;
  const int mblocks = (M + 15) / 16;
  const bool forced = r.id.family == QUICK_KERNEL_LEAN;
  const bool envelope = G % 128 == 0 && offsets31(r);
  const bool auto_ok = r.bare && r.grid_split_k <= 1 && envelope;
  if (!forced && !(auto_ok && M <= 16)) return false;
  // [r06 audit, profiles/r06_lean_rule_audit.txt] 5 / 6 tokens on the 768 blocks of 4096 x 12288: 8.5 -> 6.9 / 7.6 us
  const bool one_block_ok = forced || M <= 4 || N / 16 <= 512 || (M <= 6 && N / 16 <= 768 && KT <= 32);
  int bw = 0, bt = 0, bn = 0;
  double bcost = 0;
  for (const auto& b : builds) {
    if (!one_block_ok) break;
    const int waves = b[0], tmax = b[1], ntw = b[2];
    if (forced && ((r.id.waves && waves != r.id.waves) || (r.id.mt && ntw != r.id.mt))) continue;
    if (KT < waves || (KT + waves - 1) / waves > tmax || (N / 16) % ntw != 0) continue;
    if (lean_lds_need(M, K, waves, ntw, true) > kLdsPerCu) continue;
    // [r06 audit of this rule for K > 4096 (tools/lean_rule_audit.py, profiles/r06_lean_rule_audit.txt)] from five tokens a long K makes x
    // most of a workgroup's LDS (115-140 KB: one workgroup per CU): a launch that needs a second round of such workgroups loses to the
    // r01-r04 fragment kernels (12 x 5120 x 5120 10.1 against 8.1 us, 8 x 8192 x 8192 12.0 / 10.0, 6 x 11008 x 8192 15.5 / 13.5), one that fits
    // a single round wins (5..8 x 8192 x 4096 5.9-6.5 / 7.0-7.6, 5..8 x 5120 x 5120 5.4-5.8 / 7.3-7.6) -- so: all workgroups co-resident
    if (!forced && M >= 5 && KT > 32 && (long)(N / 16 / ntw) * mblocks > (long)std::max(1u, (unsigned)kLdsPerCu / lean_lds_need(M, K, waves, ntw, true)) * cu_count()) continue;
    // what the fullest CU streams: rounds of workgroups x bytes per workgroup; two tiles per workgroup share the head (0.85, measured);
    // sixteen waves with <= 4 tiles each and twelve tiles per wave cost
    const long wgs = (long)(N / 16 / ntw) * mblocks;
    double cost = (double)((wgs + 255) / 256) * ntw * (ntw == 2 ? 0.85 : 1.0);
    if (waves == 16 && tmax <= 4) cost *= 1.13;
    if (tmax >= 12) cost *= 1.12;
    cost *= 1.0 + 0.001 * tmax;  // (ties: the smallest register ring)
    if (bw == 0 || cost < bcost) {
      bcost = cost;
      bw = waves;
      bt = tmax;
      bn = ntw;
    }
  }
  if (forced || bw) {
    p.kernel = QUICK_KERNEL_LEAN;
    p.ksplit = 1;
    p.kt_per_split = KT;
    p.mt = bn ? bn : (r.id.mt == 2 ? 2 : 1);
    p.waves = bw ? bw : (r.id.waves ? r.id.waves : 8);
    p.lean_tmax = envelope ? bt : 0;
    p.ntiles = (N / 16) * mblocks;
    p.grid_x = N / 16 / p.mt;
    // persistent launches (fewer workgroups than channel blocks; builds of <= 4 tiles per wave, G = 128, one token block): forced by
    // kernel bits 22-24 = workgroups per CU
    if (forced && r.id.slots && bt && bt <= 4 && p.waves == 8 && G == 128 && mblocks == 1 && lean_lds_need(M, K, p.waves, p.mt, true, true) <= kLdsPerCu)
      p.grid_x = std::min(p.grid_x, cu_count() * r.id.slots);
    return true;
  }
  // 8..16 tokens on a wide layer: every one-block workgroup would fetch its own copy of x (more L2 -> LDS bytes than weights) -- one
  // persistent workgroup per CU instead, x staged once, the next block's weights requested under this block's tiles [profiles/r05_lean_persist.txt,
  // in-kernel spans against the r01-r04 picks: 16 x 4096 x 22016 18.0 -> 14.4 us, 16 x 4096 x 12288 10.2 -> 9.0, 8 x 4096 x 22016 13.7 -> 12.4]
  if (auto_ok && G == 128 && M >= 8 && M <= 16 && N / 16 > 512 && KT >= 8 && KT <= 32) {
    const int ntw = ((N / 16) % 2 == 0 && M <= 12 && N / 16 >= 1024 && lean_lds_need(M, K, 8, 2, true, true) <= kLdsPerCu) ? 2 : 1;
    if (lean_lds_need(M, K, 8, ntw, true, true) <= kLdsPerCu) {
      p.kernel = QUICK_KERNEL_LEAN;
      p.ksplit = 1;
      p.kt_per_split = KT;
      p.mt = ntw;
      p.waves = 8;
      p.lean_tmax = 4;
      p.ntiles = (N / 16) * mblocks;
      p.grid_x = std::min(N / 16 / ntw, cu_count());
      return true;
    }
  }
  return false;
}

// [r06] mid-token kernels (w4a16_xm.hpp): one workgroup = 32 or 64 tokens x pr x 32 channels for all of K, eight waves splitting K, each with its
// own x ring and weight queue; x is fetched once per workgroup, in whole cache lines.  Forced: family XM, bits 4-7 = channel pairs per workgroup
// (1..3; 0 = choose), bits 8-9 = 1 / 2: 32- / 64-token tiles whatever the count.  A launch of these is launch ramp + the workgroup's x and
// weight streams one behind the other + the dequantisation + the waves' reduction, with little overlap (profiles/r06_xm_anatomy.txt),
// so what counts is ONE round of workgroups, few bytes of x per CU and every CU busy.  The rule, from the audit of every selection against
// the other families on 15 layer shapes x 8 token counts, three boxes (profiles/r06_xm_audit.txt: pick / best geomean 1.0006-1.005, worst 1.04 on two boxes; QUICK_AMD_XM=0
// switches the family off for A/B; tools/xm_rule_eval.py restates the rule and replays it against an audit file):
//   * K >= 4096 (the audit's layers), and only layers that ONE round of workgroups covers with <= 3 channel pairs each (N = 27648 .. 57344: the
//     exchange-K kernels stay);
//   * 17..32 tokens, K <= 8192: the fewest pairs per workgroup that make one round (0.72-0.97 of the others' time; longer K: the fragment kernels,
//     whose x is 16 tokens deep, stay ahead by 7-35 %);
//   * 33..64 tokens on layers of <= 128 pairs (N <= 4096): two 32-token tiles x one pair -- every CU busy beats the halved dequantisation -- up to
//     K = 8192, and up to 48 tokens at K = 11008 (0.83-1.0 of the exchange launch it replaces, whose time follows the box: three boxes,
//     profiles/r06_xm_audit.txt; 56 / 64 tokens there and K = 14336 were ahead on one box and 4-16 % behind on two: not taken);
//   * 65..128 tokens: the rule and its audit sit at the branch below;
//   * 33..64 tokens, wider layers, K <= 8192: two 32-token tiles x <= 2 pairs where that is one round (N = 5120 .. 8192: 0.82-0.93; layers that
//     leave > 30 % of the CUs idle only from 56 tokens), else 64-token tiles x the fewest pairs that make one round (N = 10240 .. 22016: 0.87-1.0).
static bool plan_xm(const Req& r, Plan& p) {
  const int M = r.M, N = r.N, KT = r.KT;
  const bool forced = r.id.family == QUICK_KERNEL_XM;
  static const bool xm_on = [] {
    const char* e = getenv("QUICK_AMD_XM");
    return !(e && *e && atoi(e) == 0);
  }();
  const bool envelope = pow2_groups(r.G) && offsets31(r);   // (a wave without a k tile adds zeros)
  const int pairs = N / 32, cus = cu_count();
  const auto one_round = [&](int mtiles) {   // fewest channel pairs per workgroup (1..3) that cover the layer in one round, or 0
    for (int c = 1; c <= 3; ++c)
      if ((pairs + c - 1) / c * mtiles <= cus) return c;
    return 0;
  };
  int mb = 0, pr = 0;
  if (forced) {
    mb = r.id.xm_tile ? r.id.xm_tile : (M <= 32 ? 1 : 2);
    pr = r.id.mt ? std::max(1, std::min(3, r.id.mt)) : 1;
    if (!r.id.mt)
      while (pr < 3 && (long)((pairs + pr - 1) / pr) * ((M + mb * 32 - 1) / (mb * 32)) > cus) ++pr;
  } else if (r.bare && xm_on && !r.with_ln && r.grid_split_k <= 1 && envelope && M > 16 && M <= 128 && KT >= 32) {   // (K >= 4096: what the audit measured)
    if (M > 64) {
      // [r06, profiles/r06_xm_audit_65_128.txt (three boxes) and r06_planner_audit.txt, third section (two more, every family forced)] 65..128 tokens against the
      // four-slice 128 x 128 four-wave tile:
      //   * three or four 32-token tiles x the fewest pairs that make ONE round where that is <= 2 pairs (N <= 5120; K <= 8192: 80 x 4096 x 4096 10.7-11.8 -> 8.4-8.9 us,
      //     128 x: 11.0 -> 9.0-10.6, 96 x 5120 x 5120 12.7 -> 11.0; K = 11008 up to 80 tokens: 19.4 -> 18.6-19.3) or, up to 96 tokens, 3 pairs (4096 x 6144: 0.92-1.0);
      //   * else two 64-token tiles x <= 2 pairs that fill >= 80 % of the CUs: K = 4096 up to 128 tokens (4096 x 8192: 20.5 -> 13.6-15.0), K <= 8192 up to 95
      //     (8192 x 8192: 24.4 -> 21.9 on three boxes of four; the four-wave tile follows the box there, 18.8-25.4 us);
      //   * three pairs of 64-token tiles (4096 x 12288, 8192 x 10240) were ahead of the 64-token exchange tiles those counts ran until this audit, but are level with / 12 %
      //     behind the 128 x 128 four-wave tile, which the planner runs from 65 tokens since (below): not taken.  Wider layers, longer K: behind -- they stay.
      const int p1 = one_round((M + 31) / 32), p2 = one_round(2);
      if (p1 && p1 <= 2 && (KT <= 64 || (KT <= 86 && M <= 80))) mb = 1, pr = p1;
      else if (p1 == 3 && M <= 96 && KT <= 64) mb = 1, pr = 3;
      // [r06, end of round: 96 / 128 x 8192 x 8192 on three more boxes (profiles/r06_planner_audit.txt)] ... and up to 128 tokens with K <= 8192 as well: the four-slice 128 x 128 launch these
      // counts ran reads 19.6-32.8 us by box there (all 256 CUs in a four-way exchange), the two 64-token tiles 21.2-23.4: ahead by 9-11 % on three boxes of five, level on one, 2-4 % behind on one.
      else if (p2 && 10 * ((pairs + p2 - 1) / p2 * 2) >= 8 * cus && p2 <= 2 && KT <= 64) mb = 2, pr = p2;
    } else if (M <= 32) {
      if (KT <= 64 && (pr = one_round(1))) mb = 1;
    } else if (2 * pairs <= cus) {
      if (KT <= 64 || (KT <= 86 && M <= 48)) mb = 1, pr = 1;   // (K = 11008 at 56 / 64 tokens: 4-7 % behind the exchange launch on two boxes of three, 13 % ahead on the third; K = 14336: ahead on the audit's first box only, 7-16 % behind the eight-slice exchange launch on two more -- not taken)
    } else if (KT <= 64) {
      const int p1 = one_round(2), p2 = one_round(1);
      if (p1 && p1 <= 2) {
        const int wgs = (pairs + p1 - 1) / p1 * 2;
        if (10 * wgs >= 7 * cus || M >= 56) mb = 1, pr = p1;
      } else if (p2) {
        // [r06, three boxes, profiles/r06_xm_audit.txt] ... except 57..64 tokens on a long K (> 4096) where the 64-token tiles leave > 30 % of the CUs idle: 64 x 8192 x 10240
        // (160 workgroups) 21.6-22.0 us against 20.3-21.2 for the 64 x 128 four-wave tile on every box (level at 56 tokens, 3-8 % ahead up to 48)
        if (!(KT > 32 && M > 56 && 10 * ((pairs + p2 - 1) / p2) < 7 * cus)) mb = 2, pr = p2;
      }
    }
    if (!mb) pr = 0;
  }
  if (!forced && !pr) return false;
  const int mtiles = (M + mb * 32 - 1) / (mb * 32);
  p.kernel = QUICK_KERNEL_XM;
  p.ksplit = 1;
  p.kt_per_split = KT;
  p.wide_mb = mb;
  p.wide_pairs = pr;
  p.grid_x = (pairs + pr - 1) / pr;
  p.ntiles = p.grid_x * mtiles;
  p.waves = 8;
  p.lean_tmax = envelope ? 1 : 0;   // (0 = no build for this shape: the launch answers UNSUPPORTED)
  return true;
}

// What the family pick decided: the family, and the tiles its rules and models chose (0 = the family's own choice)
struct Pick {
  int family;
  int wide_mb, wide_pairs;  // the r02 model's wide tile (0: not a wide pick)
  bool wide_ring;           // ... run by the ring kernel
  int tiled_mt;             // the r02 model's tiled tile, token tiles of 16 (0: not a model pick)
  int xk_mb;                // exchange-K: token tiles of 32
  int xw_mb, xw_pairs, xw_s;  // four-wave: token tiles of 32, channel pairs, K slices
  bool exact32;             // 32-token tiles fit the token count exactly (the tiled kernel's tile rule)
  double est_us, est_xw_us;
};

static Pick pick_family(const Req& r) {
  const int M = r.M, K = r.K, N = r.N, G = r.G, KT = r.KT, family = r.id.family;
  const bool no_req = !r.id.mt && !r.id.waves;
  Pick k{};
  // skinny: one workgroup per 16 tokens x 16..64 channels for all of K (x re-read per channel block, no cross-workgroup
  // reduction); tiled: 32..64 tokens x 128 channels through LDS.  Measured crossover [r01]: the tiled kernel wins from
  // M = 65, and from M = 17 once there are >= 64 tiles of 128 channels (N >= 8192) so that it needs no K split.
  // [r02] ... and at M = 57..64 on a small layer with a long K: 32-token tiles with a 4-way K split (64 x 11008 x 4096 17.7-18.9 ->
  // 17.0-17.3 us, 64 x 14336 x 4096 22.2 -> 19.8, 64 x 16384 x 4096 24.8 -> 21.0; a tie at M = 49..56, and up to K = 8192 the
  // skinny kernel stays ahead: 64 x 8192 x 4096 13.9 against 14.5 us, 64 x 4096 x 4096 8.3 against 10.9)
  const int tiled_tiles = (N / 128) * ((M + 63) / 64);
  // [r02 audit, profiles/r02_planner_audit*.jsonl] 48 tiles are enough (4096 x 6144, M = 24..64: 10.4-12.8 against the skinny
  // kernel's 11.4-14.2 us); and the long-K rule starts at M = 33 from K = 12288 (48 x 14336 x 4096: 22.2 -> 19.2)
  // (the 48-tile rule with G % 128 == 0 only: at G = 64 / 32 the four-tile exact skinny kernel is ahead there, 32 x 4096 x 6144 9.4 /
  // 10.0 against 11.1 / 11.5 us)
  bool want_tiled = M > 64 || (M > 16 && tiled_tiles >= (G % 128 == 0 ? 48 : 64)) || (M > 56 && K >= 10240) || (M > 32 && K >= 12288);
  // [r02, third audit: 21 layer shapes incl. Llama-2-13B / Qwen2 / Yi ones the rules above were not tuned on, M = 20..64,
  // scripts/gpu_planner_sweep_17_64.sh]  With G % 128 == 0 the rule is the four-tile skinny kernel's own geometry instead: it wins where
  // its workgroups (64 channels x 16 tokens each, K split in powers of two down to 8 stages) fit one round of 256 AND a workgroup's K
  // slice is at most 64 stages (4096 x 6144 M = 20..32: 7.6 against the tiled kernel's 10.3 us, 5120 x 5120 M <= 48: 8.6-9.2 against
  // 10.8-12.8, 8192 x 8192 M <= 32: 13.3 against 14.2); two rounds (5120 x 5120 M = 64: 16.0 against 13.0) or long slices
  // (13824 x 5120 M <= 32: 19.3-21.3 against 16.2, 20480 x 7168: 28.4 against 23.7) go to the tiled kernel.
  if (G % 128 == 0 && M > 16 && M <= 64 && N % 64 == 0) {
    const long wg = (long)(N / 64) * ((M + 15) / 16);
    int sk = 1;
    while (wg * sk * 2 <= 256 && KT / (sk * 2) >= 8) sk *= 2;
    want_tiled = !(wg <= 256 && (KT + sk - 1) / sk <= 64);
  }
  k.family = family == QUICK_KERNEL_AUTO ? (want_tiled ? QUICK_KERNEL_TILED : QUICK_KERNEL_SKINNY) : family;
  // Wide kernels (32x32x16 MFMA, one wave per SIMD, LDS-DMA) from 256 tokens, and from 64 tokens once there are enough
  // 64 x 128 tiles to cover the chip (large N): 13 % ahead of the r01 kernels on average over 45 (M, K, N) shapes between
  // 64 x 4096 x 12288 and 8192 x 4096 x 22016, never behind by more than 3 % [r02 probes, profiles/r02_planner_probe*.jsonl].
  // The tile (mb x 32 tokens, pairs x 128 channels) minimises a fitted launch-time model, see below.
  // [r02] ... or, with fewer tiles, once the K slices that fill the chip are still >= 32 stages long (64 x 28672 x 8192: 64 tiles
  // x 4 slices of 56 stages, 46.6 us against the tiled kernel's 54.6-58; M = 80 / 96 / 128 / 200 there: 70.6 / 72.4 / 73.8 / 126.9
  // against 78.4 / 80.0 / 79.3 / 150.8; at 16-22 stages per slice the r01 kernels stay ahead)
  const long wide_tiles64 = (long)((M + 63) / 64) * (N / 128);
  // (audit: from 24 stages -- 96 / 128 x 14336 x 4096, 4 slices of 28: 27.3 / 28.0 against 29.0 / 29.3 us; at 21 stages it is a toss-up,
  // 96 x 11008 x 4096 22.8 against 23.6 but 48 x 8192 x 10240 25.2 against 22.3 -- and from M = 33: 48 x 28672 x 8192 54.6 -> 45.5)
  // (after the store-path change [r02, second audit]: from 21 stages above 64 tokens -- 96 / 128 x 11008 x 4096 22.8 / 24.3 against 24.4 / 25.6)
  // (third audit, with any-count K splits: one token tile, M = 33..64, from 16 stages per slice while the tiles fit one round -- 8192 x
  // 8192 18.0 against 19.0 us, 18944 x 3584 20.6 against 22.3, 28672 x 8192 41.6 against 53, 4096 x 22016 21.3 against 22.2; at 4-11
  // stages per slice the reduction makes it lose 2-8 %, and so do two rounds of tiles, 8192 x 57344 82 against 74)
  const bool wide_long_k = M <= 64 ? (wide_tiles64 <= 256 && KT / std::max<long>(1, 256 / wide_tiles64) >= 16)
                                   : (wide_tiles64 <= 128 && KT / std::max<long>(1, 256 / wide_tiles64) >= 21);
  // ... except where 32-token tiles fit the token count exactly, fill one round and the 64- / 128-token tiles would run a quarter
  // empty (M = 65..96 on Llama-2-70B's qkv: 96 x 8192 x 10240 = 240 tiles of 32 x 128, 30.2 us against 38.6 [r02 audit])
  const long tiles32 = (long)((M + 31) / 32) * (N / 128);
  k.exact32 = M < 128 && ((M + 63) / 64) * 64 - M >= 32 && tiles32 >= 208 && tiles32 <= 256 && !wide_long_k;
  // 65..256 tokens: the r01 tiled kernel's 32 x 128 and 64 x 128 tiles compete in the same model (its own K-split rule, coefficients
  // from all five audits); over the 152 audited shapes of that range the minimum is 1.2 % behind the best measured kernel on average,
  // 12 % at worst, where the separate rules were 2.1 % / 22 % (160 x 4096 x 6144: five exact 32-token tile rows, 17.7 against 21.4 us)
  const bool unified = family == QUICK_KERNEL_AUTO && G % 128 == 0 && M > 64 && M <= 256 && no_req;
  if (family == QUICK_KERNEL_AUTO && G % 128 == 0 &&
      (unified || (!k.exact32 && ((M >= 64 && (M >= 256 || wide_tiles64 >= 96)) || (M > 32 && wide_long_k))))) {
    // (96 tiles of 64 x 128 [second audit]: 64 x 4096 x 12288 17.3 against 18.0 us, 96 / 128 x 4096 x 6144 16.8 / 17.2 against 17.4 / 18.0,
    // 192 x 4096 x 4096 16.9 against 17.9, 192 x 4096 x 6144 22.2 against 24.5; at 64-80 tiles the r01 kernels are level or ahead)
    // Launch-time model per kernel, fitted (relative least squares) to 198 shapes x 10 kernels, 64..8192 tokens on the model
    // layers [r02, scripts/gpu_planner_sweep_large.sh, two sessions averaged; residual 2.5-3.4 % rms = the session noise]:
    //   us = c + a n + stages (b_ceil n + b_frac f) [+ split0 + split1 * slices * tile MB],  n = ceil(f), f = workgroups / 256
    // -- a round of tiles costs what its fullest CU runs (b_ceil), and a partly filled chip runs its tiles faster (b_frac: clocks,
    // HBM share).  Picking the minimum is within 0.6 % of the best measured kernel on average over the 182 shapes routed here,
    // 7.5 % at worst (the r01 cost model after the store-path change: 4.4 % / 26 %).  The ring kernel only at 64 x 128 (one
    // workgroup per CU); 64 x 256 / 128-token ring variants and the 256 x 128 tile never won a shape in the sweep.
    struct WideCand { int mb, pairs; double c, a, b_ceil, b_frac, split0, split1; };
    static const WideCand cand[5] = {{2, 1, 1.31, 2.61, 0.3806, 0.2214, 2.03, 19.6},   // (fitted on four waves, 0.3985 / 0.2318; eight waves: x 0.955, the median over 337 rows)
                                      {2, 2, 6.34, -0.46, 0.4908, 0.5177, 2.13, 13.5},
                                     {4, 1, 6.08, -0.99, 0.4298, 0.5297, 2.54, 13.1}, {4, 2, -1.68, 7.41, 0.6715, 1.0087, 3.53, 10.6},
                                     {8, 2, -7.23, 15.76, 1.2716, 1.7451, 2.48, 58.9}};
    double best = 0;
    for (int c = 0; c < 5; ++c) {
      const int mb = cand[c].mb, pairs = cand[c].pairs;
      if (N % (pairs * 128) != 0) continue;
      const long T = (long)((M + mb * 32 - 1) / (mb * 32)) * (N / (pairs * 128));
      const int s = wide_split(KT, T);
      const double f = (double)(T * s) / 256.0, n = (double)((T * s + 255) / 256), stages = (double)((KT + s - 1) / s);
      // (64 x 128 tiles in more than one round: the double-buffered kernel, 2-4 workgroups per CU, instead of the ring's one --
      // 256 x 4096 x 12288 33.8 against 42.3 us; its own fit over the 219 such rows of the audits, 2.1 % rms)
      const bool rounds64 = mb == 2 && pairs == 1 && T * s > 256;
      double cost = rounds64 ? 5.25 - 0.05 * n + stages * (0.2382 * n + 0.3242 * f)
                                   : cand[c].c + cand[c].a * n + stages * (cand[c].b_ceil * n + cand[c].b_frac * f) +
                                         (s > 1 ? cand[c].split0 + cand[c].split1 * s * (mb * 32.0 * pairs * 128 * 4 / 1e6) : 0.0) -
                                         (s == 2 && mb * pairs <= 8 ? 1.2 : 0.0);   // (two slices: the own partial stays in registers, measured after the fit)
      // [r03 audit, profiles/archive/r03_xk_audit.jsonl] tiles of <= 128 x 128 in SEVERAL rounds run 10-20 % behind this fit on the r03 boxes
      // (measured / predicted, medians: 64 x 128 1.13-1.21, 64 x 256 1.14-1.21, 128 x 128 1.22 against 1.12 in one round; 128 x 256
      // 1.04-1.10 and 256 x 256 1.01-1.05 as fitted): 640 x 5120 x 13824 121 us on 540 tiles against 101 on 162 of 256 x 256
      static const double several_rounds[5] = {1.2, 1.2, 1.2, 1.0, 1.0};  // (replayed on the audit's rows, tools/audit_replay.py: mean gap 0.95 -> 0.37 %, worst 19 -> 7 %)
      if (n >= 2.0) cost *= several_rounds[c];
      if (k.wide_mb == 0 || cost < best) {
        best = cost;
        k.wide_mb = mb;
        k.wide_pairs = pairs;
        k.wide_ring = mb == 2 && pairs == 1 && !rounds64;
      }
    }
    if (unified) {
      static const double tc[2][6] = {{5.968, -0.491, 0.263, 0.145, 0.697, 0.421}, {4.645, 1.535, 0.432, 0.195, 1.204, 0.711}};  // 32 / 64 tokens
      for (int c = 0; c < 2; ++c) {
        const int mt = c == 0 ? 2 : 4;
        const long T = (long)(N / 128) * ((M + mt * 16 - 1) / (mt * 16));
        const int nstage = (KT + 1) / 2;  // (eight waves: stages of 256 k)
        int s = 1;
        while (T * s * 2 <= 256 && nstage / (s * 2) >= 2) s *= 2;
        if (256 / T > s && nstage / (256 / T) >= 2) s = (int)(256 / T);
        s = std::max(1, std::min(s, nstage));
        const int kps = ((nstage + s - 1) / s) * 2, slices = (KT + kps - 1) / kps;
        const double f = (double)(T * slices) / 256.0, n = (double)((T * slices + 255) / 256);
        const double cost = tc[c][0] + tc[c][1] * n + kps * (tc[c][2] * n + tc[c][3] * f) + (slices > 1 ? tc[c][4] + tc[c][5] * slices : 0.0);
        if (cost < best) {
          best = cost;
          k.tiled_mt = mt;
        }
      }
      if (k.tiled_mt) k.wide_mb = 0;
    }
    // [r03] the exchange-K kernels (w4a16_xk.hpp) compete in the same model where their workgroups -- tiles x K slices, slices = the
    // largest power of two that still fits one round -- are co-resident.  Fitted (relative least squares, 246 / 336 rows of
    // scripts/gpu_xk_sweep.sh: 15 layer shapes x 24..1024 tokens, 4.4 / 3.7 % rms) and brought to this model's scale with the same
    // session's measurements of the planner's own wide picks (194 rows, predicted / measured = 0.945):
    //   us = c + stages (b0 + b1 f) + [s > 1] (s0 + s1 s) + d f,   f = workgroups / 256
    // 64-token tiles: the r02 ring tile with the weights in an AGPR queue and five x slots, 3-6 % ahead of it wherever both run
    // (512 x 4096 x 4096 22.6 against 23.8 us); 128-token tiles with 2 / 4 slices: 384 x 11008 x 4096 1.16x, 640 x 4096 x 4096 1.12x.
    if (best > 0 && r.allow_xk) {
      static const double xc[2][6] = {{1.728, 0.3869, 0.1572, 2.320, 0.1693, 2.064}, {3.422, 0.4881, 0.3847, 1.214, 0.4284, 2.382}};
      const int cus = exchange_cus();
      for (int c = 0; c < 2; ++c) {
        const int mb = c == 0 ? 2 : 4;
        const long T = (long)((M + mb * 32 - 1) / (mb * 32)) * (N / 128);
        int sx = 1;
        while (sx < 8 && T * sx * 2 <= cus && KT / (sx * 2) >= 4) sx *= 2;
        while (sx > 1 && (T * sx > cus || !splits_evenly(KT, sx))) sx /= 2;
        if (T * sx > 256) continue;  // (several rounds: the 128 x 256 / 256 x 256 tiles of the wide family are ahead, 0.8x in the sweep)
        const double f = (double)(T * sx) / 256.0, stages = (double)((KT + sx - 1) / sx);
        // (128-token tiles + 4 %: where the two are close the 64-token tile was the better pick in the audit that followed,
        // 128 x 7168 x 7168 22.2 -> 21.0 us, 160 x 14336 x 4096 35.2 -> 32.7 [scripts/gpu_xk_audit.sh])
        const double cost = (xc[c][0] + stages * (xc[c][1] + xc[c][2] * f) + (sx > 1 ? xc[c][3] + xc[c][4] * sx : 0.0) + xc[c][5] * f) * (c == 1 ? 1.04 : 1.0);
        if (cost < best) {
          best = cost;
          k.xk_mb = mb;
          k.wide_mb = 0;
          k.tiled_mt = 0;
        }
      }
    }
    // [r04] the four-wave kernels with generated hand-placed loops (w4a16_xw.hpp) -- 128 x 256, 128 x 128 and 64 x 128 tiles, 1 / 2 / 4 K
    // slices per tile.  Their own launch-time model (same form as above; fitted, relative least squares, to scripts/archive/r04_gpu_xw_sweep.sh:
    // 9 layer shapes x 12 token counts x 6 forced variants, 4.3 / 4.7 / 1.7 % rms) picks the tile and the slice count; WHETHER one of them
    // runs is decided on the sweep's own rows, against the pick of the rules above (profiles/r04_xw_sweep.jsonl, tools/xw_sweep_report.py):
    // they replace the 64- / 128-token wide tiles, the tiled kernel and the exchange-K tiles (6 % faster on the geometric mean of the 108
    // shapes, 13-24 % where the r02 128-token wide tile ran), not the 256 x 256 tile (level within 5 %, behind at 8192 tokens), and below
    // 160 tokens only from 96 tokens on wide layers (N >= 10240: 96 / 128 x 4096 x 11008 20.7 / 21.0 -> 17.8 / 18.6 us; at N = 4096 the 64-token
    // exchange-K tile stays 5-7 % ahead).
    // (where the 256 x 256 tile is the pick they compete only if it runs with a K split: 1024 x 28672 x 8192, 128 tiles x 2 slices, 419 us
    // against 379 on 256 tiles of 128 x 256 -- profiles/r04_xw256.txt)
    if (best > 0 && r.allow_xk && (k.wide_mb != 8 || (N % 256 == 0 && wide_split(KT, (long)((M + 255) / 256) * (N / 256)) > 1)) && pow2_groups(G) &&
        M >= 65 &&   // [r06 audit at 80 tokens, profiles/r06_planner_audit.txt: from 65 tokens -- the 128 x 128 tile with its upper rows empty is 10-32 % ahead of the 64-token
                     // exchange tiles these counts fell to: 80 x 4096 x 22016 29.8 -> 25.4 us, x 13824 x 5120 31.6 -> 23.4, x 28672 x 8192 66.0 -> 55.8]   [r05 sweep, profiles/r05_mid_sweep.txt: from 96 tokens on the narrow layers as well -- 96 / 128 x 4096 x 4096 12.4 / 12.6 -> 11.4 / 11.6 us, x 5120 x 5120 14.8 / 16.9 -> 13.6 / 13.9, x 8192 x 8192 27.9 / 29.1 -> 25.0 / 26.0, x 13824 x 5120 29.5 -> 25.4; at 33..64 tokens no four-wave tile beats the r03 picks by more than the session noise]
        offsets32(r)) {
      struct XwCand { int mb, pairs; double c, a, b_ceil, b_frac, s0, s1, d; };
      static const XwCand xwc[3] = {{4, 2, -2.8632, 5.8843, 0.8799, 0.6018, -0.6402, 1.2461, 5.8244},
                                    {4, 1, -0.3015, 1.9468, 0.5116, 0.3473, -0.0715, 1.0316, 4.3280},
                                    {2, 1, 1.8009, 3.7953, 0.3277, 0.2559, 0.1770, 0.3541, 0.0325}};
      double xbest = 0;
      for (int c = 0; c < 3; ++c) {
        const int mb = xwc[c].mb, pairs = xwc[c].pairs;
        if (N % (pairs * 128) != 0) continue;
        const long T = (long)((M + mb * 32 - 1) / (mb * 32)) * (N / (pairs * 128));
        for (int sx = 1; sx <= mb && sx <= 4; sx *= 2) {
          if (sx > 1 && (T * sx > std::min(256, exchange_cus()) || KT / sx < 4 || !splits_evenly(KT, sx))) continue;
          const double f = (double)(T * sx) / 256.0, n = (double)((T * sx + 255) / 256), stages = (double)((KT + sx - 1) / sx);
          // (- 0.5 us with slices: the exchange lost its atomics after the fit -- 512 x 4096 x 4096 22.0 -> 21.5 / 24.2 -> 23.3 us on two / four
          // slices, profiles/r04_ab_exchange.txt)
          const double cost = xwc[c].c + xwc[c].a * n + stages * (xwc[c].b_ceil * n + xwc[c].b_frac * f) + (sx > 1 ? xwc[c].s0 + xwc[c].s1 * sx - 0.5 : 0.0) + xwc[c].d * f;
          if (k.xw_mb == 0 || cost < xbest) {
            xbest = cost;
            k.est_xw_us = cost;
            k.xw_mb = mb;
            k.xw_pairs = pairs;
            k.xw_s = sx;
          }
        }
      }
      // [r06, three-box audit of the final tree, profiles/r06_planner_audit.txt] 129..256 tokens on layers where FOUR slices of the 128 x 128 tile are exactly one round
      // (N = 4096: 2 x 32 tiles x 4): the fit prefers two slices of the 64 x 128 tile there, and every box measured the 128 x 128 tile ahead -- 160 / 192 / 256 x 4096 x 4096
      // 13.5-15.2 -> 12.6-14.0 us (4-7 %), 160 / 192 x 11008 x 4096 27.2-28.5 -> 24.1-26.7 (7-10 %).  (N = 5120: 320 workgroups, the 64-token tile stays ahead.)
      if (k.xw_mb == 2 && k.xw_pairs == 1 && k.xw_s == 2 && M > 128 && M <= 256 && N % 128 == 0) {
        const long T41 = (long)((M + 127) / 128) * (N / 128);
        if (T41 * 4 <= std::min(256, exchange_cus()) && KT / 4 >= 4 && splits_evenly(KT, 4)) {
          k.xw_mb = 4, k.xw_pairs = 1, k.xw_s = 4;
        }
      }
    }
    // [r04] where the r02 model's pick is the 256 x 256 tile with ONE K slice, the four-wave kernel with the generated 256 x 256 loop runs it
    // instead: 0.935-0.965 of the hipcc-scheduled kernel's time on 28 prefill shapes of 1024..8192 tokens in one session, bit-identical
    // results (scripts/archive/r04_gpu_xw82.sh, profiles/r04_xw256_sweep.jsonl; 4096^3 117.3 -> 111.6 us, 8192 x 4096 x 22016 1232 -> 1170).
    // QUICK_AMD_XW256=0 keeps r02's kernel (the A/B switch; since r06 that kernel is only in QUICK_AMD_TOOLS builds -- it spills 92 bytes per lane --
    // and the product answers the switch with 128 x 256 tiles).
    if (best > 0 && k.wide_mb == 8 && !k.xw_mb && !k.xk_mb && N % 256 == 0 && pow2_groups(G) && KT >= 2 &&
        wide_split(KT, (long)((M + 255) / 256) * (N / 256)) == 1 && offsets32(r)) {
      const char* e = getenv("QUICK_AMD_XW256");
      if (!e || atoi(e) != 0) {
        k.xw_mb = 8, k.xw_pairs = 2, k.xw_s = 1;
        k.est_xw_us = 0.95 * best;
      }
    }
    k.est_us = best;
    // ... unless the models say the r02 / r03 candidate is clearly ahead: on the audit's 133 four-wave picks (scripts/archive/r04_gpu_audit_vs_r03.sh, this
    // tree against r03's library in one session) the r03 model reads 0.95x and the four-wave model 1.03x the measured time, and "four-wave
    // iff its estimate < 1.10 x the other" is the best threshold (geometric mean 0.904 against 0.905 for always; it returns 320 x 4096 x 12288 /
    // 22016 -- 430 tiles of 64 x 256 against 516 of 128 x 128, a nearly empty third round -- to the r02 ring kernel: 43.5 -> 39.6 us, 82.9 -> 75.0)
    if (k.xw_mb && k.est_xw_us >= 1.10 * best) k.xw_mb = 0;
    if (k.xw_mb) k.family = QUICK_KERNEL_XW;
    else if (k.xk_mb) k.family = QUICK_KERNEL_XK;
    else if (k.wide_mb) k.family = QUICK_KERNEL_WIDE;
    else if (k.tiled_mt) k.family = QUICK_KERNEL_TILED;
  }
  // [r03] 33..64 tokens where the rules above leave the 32-token tiled kernel with a K split: one 64-token exchange-K tile per CU
  // instead, when its slices are long (>= 8 stages) and cover most of the chip -- Mistral's fused GQA qkv, 4096 x 6144, at 48 / 64
  // tokens 12.8 / 13.0 -> 10.6 / 10.8 us, 64 x 5120 x 5120 13.5 -> 11.6; with eight slices, 40..64 x 11008 / 14336 x 4096 (the down
  // projections at batch 40..64): 16.6-19.8 -> 14.6-16.4 us in two sessions of three, 3 % behind in the third
  // [scripts/gpu_xk_sweep.sh, gpu_xk_audit.sh]
  if (r.allow_xk && family == QUICK_KERNEL_AUTO && k.family == QUICK_KERNEL_TILED && G % 128 == 0 && M > 32 && M <= 64 && no_req) {
    const long T = N / 128;
    int sx = 1;
    while (sx < 8 && T * sx * 2 <= std::min(256, exchange_cus()) && KT / (sx * 2) >= 4) sx *= 2;
    while (sx > 1 && !splits_evenly(KT, sx)) sx /= 2;
    if (T * sx >= 160 && T * sx <= cu_count() && KT / sx >= 8) {
      k.family = QUICK_KERNEL_XK;
      k.xk_mb = 2;
    }
  }
  // [r05 audit, profiles/r05_planner_audit.txt / r05_mid_sweep.txt: AUTO against forced launches of every family, 234 + 65 shapes, two sessions]
  // two corrections where a four-wave tile was consistently ahead of the models' pick:
  //  * 33..95 tokens, 160..256 workgroups of 64 x 128 tiles x TWO slices (N = 12288, 13824, 10240): 33 / 48 / 64 x 4096 x 12288 13.8 / 14.9 / 15.1 ->
  //    12.5 / 13.4 / 13.7 us, 48 / 64 x 8192 x 10240 26.6 / 25.4 -> 21.8 / 22.2, 64 x 5120 x 13824 21.0 -> 18.7;
  //  * 96..128 tokens where ONE row of 128 x 128 tiles x FOUR slices fits a round (N <= 8192): 96 / 128 x 4096 x 4096 12.0 / 12.1 -> 11.0 / 11.0,
  //    x 4096 x 6144 13.7 / 14.0 -> 11.7 / 12.0, x 5120 x 5120 14.8 / 16.9 -> 13.6 / 13.9
  // Final tree, two boxes (tools/audit_auto_vs_forced.py): geometric mean AUTO / best forced 1.0013, worst 1.048 (96 x 8192 x 8192, where two
  // token tiles of 64 x 128 x two slices are ahead of the four-slice 128 x 128 tile; a rule for it was tried and lost 18 % at 96 / 128 x
  // 28672 x 8192 -- the 64-token loop is the slower one per MFMA, only its exchange is cheaper -- so it stays a 5 % gap).
  if (r.allow_xk && family == QUICK_KERNEL_AUTO && pow2_groups(G) && no_req && r.grid_split_k <= 1 && offsets32(r)) {
    const long t64 = (long)((M + 63) / 64) * (N / 128), t128 = (long)(N / 128);
    const long xcus = std::min(256, exchange_cus());   // (QUICK_AMD_EXCHANGE_CUS: how many CUs the K slices of a tile may count on)
    if (M >= 33 && M <= 64 && t64 * 2 >= 160 && t64 * 2 <= xcus && KT / 2 >= 4 && splits_evenly(KT, 2)) {   // (r06: up to 64 tokens; above, the 128 x 128 tile -- see the four-wave rule)
      k.family = QUICK_KERNEL_XW;
      k.xw_mb = 2, k.xw_pairs = 1, k.xw_s = 2;
    } else if (M >= 65 && M <= 128 && t128 * 4 <= xcus && t128 * 4 >= 96 && KT / 4 >= 4 && splits_evenly(KT, 4)) {
      k.family = QUICK_KERNEL_XW;
      k.xw_mb = 4, k.xw_pairs = 1, k.xw_s = 4;
    }
  }
  return k;
}

// The tile of a four-wave launch, worked out BEFORE the width check: a forced id with bit 12 or two token blocks and a block count of 8 means
// 256-channel tiles all the same, and N % 256 == 128 would leave the last 128 channels unwritten -- ADVICE r04
static void xw_tile(const Req& r, const Pick& k, int& mb, int& pairs) {
  mb = k.xw_mb ? k.xw_mb : (r.id.mt == 2 ? 2 : (r.id.mt == 8 ? 8 : 4));
  pairs = k.xw_mb ? k.xw_pairs : (mb == 8 ? 2 : ((mb == 2 || r.id.b12) ? 1 : 2));
}

// The picked family where its kernel can take the launch, else r01's tiled kernel
static int within_limits(const Req& r, const Pick& k) {
  // small groups: r01's tiled kernel; x travels through a buffer descriptor with 32-bit offsets in the wide / exchange-K kernels: from
  // 4 GiB of activations on, r01's tiled kernel (64-bit pointers) runs instead (exchange-K: y through a buffer descriptor as well)
  if (k.family == QUICK_KERNEL_WIDE && (r.G % 128 != 0 || r.x_bytes >= ((size_t)1 << 32))) return QUICK_KERNEL_TILED;
  if (k.family == QUICK_KERNEL_XK && (r.G % 128 != 0 || !offsets32(r))) return QUICK_KERNEL_TILED;
  if (k.family == QUICK_KERNEL_XW) {
    int mb, pairs;
    xw_tile(r, k, mb, pairs);
    if (!pow2_groups(r.G) || r.N % (pairs * 128) != 0 || !offsets32(r)) return QUICK_KERNEL_TILED;  // (whole channel tiles)
  }
  return k.family;
}

// Four waves, one per SIMD, hand-placed K loops (w4a16_xw.hpp): tiles of 128 x 256, 128 x 128 or 64 x 128; S = 1, 2, 4 K slices per
// tile on S compute units.  Nobody has to be co-resident (a wave that waits too long gives its block up, the last partner finishes it),
// but the exchange zone holds S * S boxes of (a tile's fp16 image / S) per tile: workgroups <= 256 with S > 1.
// bits 4-7: 32-token blocks per tile (2, 4; 0 = 4); bit 12: 128-channel tiles (implied by 2 blocks); bits 8-11: S (0 = as many as fit
// the CUs); bits 22-26: log2 of the poll limit in ticks of 10 ns (tests: 1 = every wave gives up at once).
// (bits 4-7 = 8: the 256 x 256 tile -- waves of 256 tokens x 64 channels, a ring of two 64 KiB slots, one slice only)
// AUTO's rule for the staggered two-slice launch: stages (128 k) per slice and output tiles
constexpr int kXwStaggerAutoD = 1;   // (d = 2 / 3 were the A/B builds)
static bool xw_stagger_auto(int stages_per_slice, int tiles) { return tiles == 128 && stages_per_slice >= 16; }
static void shape_xw(const Req& r, const Pick& k, Plan& p) {
  const int M = r.M, N = r.N, KT = r.KT;
  int mb, pairs;
  xw_tile(r, k, mb, pairs);
  const int MBk = (M + mb * 32 - 1) / (mb * 32), NBk = N / (pairs * 128);
  p.wide_mb = mb;
  p.wide_pairs = pairs;
  p.tch = pairs * 128;
  p.waves = 4;
  p.ntiles = MBk * NBk;
  const int s_req = k.xw_s ? k.xw_s : (r.grid_split_k > 0 ? r.grid_split_k : r.id.n8);
  int s = 1;
  if (mb == 8) s = 1;
  else if (s_req == 1 || s_req == 2 || (s_req == 4 && mb == 4)) s = s_req;
  else
    while (s < mb && s < 4 && (long)p.ntiles * s * 2 <= cu_count() && KT / (s * 2) >= 4) s *= 2;
  while (s > 1 && ((long)p.ntiles * s > 256 || !splits_evenly(KT, s))) s /= 2;
  p.ksplit = s;
  p.kt_per_split = (KT + s - 1) / s;
  p.poll_log2 = r.id.poll_log2;
  if (const char* e = getenv("QUICK_AMD_EXCHANGE_POLL_LOG2")) p.poll_log2 = std::max(0, std::min(31, atoi(e)));
  // Staggered K ranges (bits 27-28 = d): only the two-slice 128 x 128 launch with G = 128, an even number of k tiles and a phase 1 of at
  // least the ring's four stages has the build; anything else is planned WITHOUT it.  AUTO (kernel id 0) takes d = 2 where it was measured
  // ahead (profiles/r07_ab_stagger.txt): one workgroup per CU half of the chip or more, 16 stages per slice or more.
  p.xw_stagger = 0;
  const auto stagger_fits = [&](int d) { return mb == 4 && pairs == 1 && s == 2 && r.G == 128 && KT % 2 == 0 && KT / 2 - d >= 4; };
  if (r.id.xw_stagger) p.xw_stagger = stagger_fits(r.id.xw_stagger) ? r.id.xw_stagger : 0;
  else if (r.bare && xw_stagger_auto(KT / 2, p.ntiles) && stagger_fits(kXwStaggerAutoD)) p.xw_stagger = kXwStaggerAutoD;
  // XCDs per K slice: they form a gm x gn grid over the (token, channel) tiles; bytes per k and XCD: x rows (2 B) + weight columns (1/2 B)
  p.xcd_gm = xcd_rows(r, (long)p.ntiles * s, MBk, NBk, 8 / s, 64L * mb, 64L * pairs);
}

// exchange-K kernels (w4a16_xk.hpp): tile = mb * 32 tokens x 128 channels, eight waves; the S slices of a tile run on S compute
// units at the same time and swap parts of their partial tiles, so S > 1 needs the whole grid co-resident: tiles * S <= CUs.
// bits 4-7: mb (2, 4; 0 = by M), bits 8-11: S (1, 2, 4, 8; 0 = as many as fit), bits 22-24: x ring slots, bits 26-28: weight queue depth
static void shape_xk(const Req& r, const Pick& k, Plan& p) {
  const int M = r.M, N = r.N, KT = r.KT;
  const int mb = k.xk_mb ? k.xk_mb : ((r.id.mt == 2 || r.id.mt == 4) ? r.id.mt : (M > 64 ? 4 : 2));
  const int MBk = (M + mb * 32 - 1) / (mb * 32), NBk = N / 128;
  const int cus = exchange_cus();
  p.wide_mb = mb;
  p.wide_pairs = 1;
  p.tch = 128;
  p.waves = 8;
  p.ntiles = MBk * NBk;
  const int s_req = r.grid_split_k > 0 ? r.grid_split_k : r.id.n8;
  int s = 1;
  if (s_req == 1 || s_req == 2 || s_req == 4 || s_req == 8) s = s_req;
  else {
    while (s < 8 && (long)p.ntiles * s * 2 <= cus && KT / (s * 2) >= 4) s *= 2;
    if (s_req == 15 && s > 1) s /= 2;  // (tuning sweeps: half the count the rule gives)
  }
  // (the slices must fit the chip, and ceil-dividing K must give exactly S non-empty slices)
  // 64-token tiles with K slices need <= 128 registers and 80 KiB of LDS: TWO workgroups are resident per CU (four waves per SIMD)
  // (tools builds, forced slice counts: measured slower than one slice on one CU -- 512 x 4096 x 4096 25.8 against 22.8 us)
#ifdef QUICK_AMD_TOOLS
  const long cap = mb == 2 ? 2L * cus : cus;
#else
  const long cap = cus;
#endif
  while (s > 1 && ((long)p.ntiles * s > ((s_req == 2 || s_req == 4 || s_req == 8) ? cap : (long)cus) || !splits_evenly(KT, s))) s /= 2;
  p.ksplit = s;
  p.kt_per_split = (KT + s - 1) / s;
  p.xk_nbuf = r.id.slots >= 3 ? r.id.slots : 5;
  p.xk_wd = r.id.xk_wd >= 3 ? r.id.xk_wd : 4;
  p.xk_loader = r.id.b12;
  // sixteen waves (bit 13): 64-token tiles with ONE slice whose K range is a whole number of 256-k stages
  p.xk_kq = (r.id.b13 && mb == 2 && s == 1 && KT % 2 == 0 && KT >= 4 && p.xk_nbuf == 5 && p.xk_wd == 4 && !p.xk_loader) ? 4 : 2;
  // XCDs per K slice: they form a gm x gn grid over the (token, channel) tiles; bytes per k and XCD: x rows (2 B) + weight columns (1/2 B)
  p.xcd_gm = xcd_rows(r, (long)p.ntiles * s, MBk, NBk, 8 / s, 64L * mb, 64);
}

// bits 4-7: MB (token tiles of 32 per workgroup: 2, 4, 8), bits 8-11: PAIRS (32-channel pairs per wave: 1, 2); 0 = choose
static void shape_wide(const Req& r, const Pick& k, Plan& p) {
  const int M = r.M, N = r.N, KT = r.KT;
  int mb = k.wide_mb ? k.wide_mb : r.id.mt, pairs = k.wide_mb ? k.wide_pairs : r.id.n8;
  if (mb != 2 && mb != 4 && mb != 8) mb = M > 128 ? 8 : (M > 64 ? 4 : 2);
  if (pairs != 1 && pairs != 2) pairs = 2;
  if (N % (pairs * 128) != 0) pairs = 1;
#ifndef QUICK_AMD_TOOLS
  if (mb == 8 && pairs == 2) mb = 4;   // [r06] no register-spilling kernel in the product: where the generated 256 x 256 loop cannot take a launch (K split, 64-bit offsets,
                                       // G not a power-of-two multiple of 128) 128 x 256 tiles run instead of r02's hipcc-scheduled 256 x 256 tile
#endif
  p.wide_mb = mb;
  p.wide_pairs = pairs;
  // bit 12: no ring (the double-buffered kernel at every tile size); bits 22-24: ring slots (0 = as many as fit, up to 6);
  // bit 15: eight waves per workgroup (two per SIMD, k16 steps split by parity) -- ring kernel, tiles up to 128 x 128 / 64 x 256
  // The planner's own ring launches (64 x 128 tiles) run the eight-wave variant with four slots: since the whole workgroup shares
  // the way out (§5.3 of DESIGN.md) it is 2-5 % ahead of four waves / six slots on every shape probed, warm against warm in one
  // session -- 512 x 4096 x 4096 24.04 against 24.68 us, 128 x 4096 x 12288 21.5 / 22.6, 64 x 4096 x 22016 20.8 / 21.7, 512 x 11008 x 4096
  // 57.8 / 59.2, 448 x 4096 x 4096 22.7 / 23.4; four slots are level with or 1 % ahead of six [r02].
  const bool auto_ring = k.wide_mb && k.wide_ring;
  const bool eight = (r.id.b15 || auto_ring) && mb * pairs <= 4 && !r.id.b12;
  const int nb_req = auto_ring ? 4 : r.id.slots, nb_max = mb == 8 ? 0 : wide_ring_nbuf(mb, pairs, eight ? 2 : 1);
  p.wide_nbuf = (r.id.b12 || nb_max < 3 || (k.wide_mb && !k.wide_ring)) ? 0 : (nb_req >= 3 ? std::min(nb_req, nb_max) : nb_max);
  p.waves = (eight && p.wide_nbuf >= 3) ? 8 : 4;
  p.tch = pairs * 128;
  const int MBk = (M + mb * 32 - 1) / (mb * 32), NBk = N / p.tch;
  p.ntiles = MBk * NBk;
  p.slab_floats = (size_t)mb * 32 * p.tch;
  p.ksplit = std::max(1, std::min(r.grid_split_k > 0 ? r.grid_split_k : wide_split(KT, p.ntiles), KT));
  p.kt_per_split = (KT + p.ksplit - 1) / p.ksplit;
  p.xcd_gm = xcd_rows(r, p.ntiles, MBk, NBk, 8, 64L * mb, p.tch / 2);   // bytes per k: x rows (2 B) + weight columns (1/2 B) per XCD
}

static void shape_skinny(const Req& r, Plan& p) {
  const int M = r.M, K = r.K, N = r.N, G = r.G, KT = r.KT;
  const int mblocks = (M + 15) / 16;
  // channel tiles per workgroup ~ token blocks (weights are re-read per token block, x per channel block)
  // (two token blocks: four tiles as well with G % 128 == 0 -- never behind two in the third audit, 32 x 5120 x 5120 15.8 -> 9.1 us)
  int mt_auto = mblocks <= 1 ? 1 : (mblocks <= 2 && G % 128 != 0 ? 2 : 4);
  // M = 9..16 on a large layer: the fragments-from-L2 path reads x once per 16-channel tile -- 4x the weight bytes at
  // M = 16 -- so share every x fragment among 4 channel tiles (8192 x 57344 at M = 16: 119 -> 78 us, 28672 x 8192:
  // 65 -> 36 us [r01]).  Small layers keep NTW = 1 (more workgroups); from 1024 channel blocks the deferred-zero path
  // (x in LDS) is as fast or faster and stays.
  if (!r.id.mt && M > 8 && M <= 32 && (long)K * N >= 40L * 1000 * 1000) {  // (M = 17..32: 11008 x 4096 16.6 -> 13.5 us)
    // (the table flavour up to M = 12: at M = 16 the 4-tile fragment flavour is ahead, 4096 x 22016 18.3 -> 16.9 us, 4096 x
    // 28672 20.3 -> 19.3 [r02 audit])
    // [r03 audit on the final kernels, scripts/gpu_small_audit2.sh: as a bare GEMM the table flavour is ahead at M = 16 as well up to
    // ~120 M weights -- 4096 x 22016 17.0 -> 14.8 us, 4096 x 28672 18.2 -> 16.8; 8192 x 57344 keeps the four tiles.]
    // Not taken: these layers are the gate_up projections, which carry the RMSNorm prologue in a decode step, and the table flavour
    // normalises its 16 rows one after the other -- Llama-2-7B / Mistral-7B at batch 16 lost 5-8 % tok/s with it [bench_decode.py].
    const bool dz_ok = mblocks == 1 && M <= 12 && !r.id.b12 && !r.id.exact && N / 16 >= 1024 &&
                       skinny_lds_bytes(M, G, 1, 8, KT, true, true, true) <= kLdsPerCu;
    if (!dz_ok) mt_auto = 4;
  } else if (!r.id.mt && M >= 5 && M <= 8 && N >= 8192 && N / 16 < 1024 && (G % 128 == 0 || (M >= 6 && (size_t)M * (K * 2 + 16) > (size_t)64 * 1024))) {
    // (r03: with G % 128 == 0 from M = 5 and at any K -- the four-tile kernel then takes its fragments from L2, below: 4096 x 12288
    // M = 5, 6 8.4-8.6 -> 7.6 us)
    // (only where the 4-tile kernel takes its fragments straight from L2: its LDS-copy flavour is slower, M = 6, 7 at K = 4096)
    mt_auto = 4;  // at M = 8: 4096 x 12288 11.0 -> 10.3 us, 8192 x 10240 18.7 -> 16.6 us, 28672 x 8192 49 -> 34 us; from
  }               // 1024 blocks (4096 x 22016, 8192 x 57344) the deferred-zero path stays ahead, and so it does at M <= 4
  // 257..512 channel blocks (N = 6144, 8192) at M = 4..16: one-tile workgroups come in 1.5 or 2 per CU -- two tiles per
  // workgroup are one round of <= 256 and share every x fragment [r02 audit: 4096 x 6144 M = 4 / 8 / 16 7.6 / 8.2 / 10.9 -> 6.4 /
  // 6.3 / 7.6 us, 8192 x 8192 M = 6 14.7 -> 10.1, 28672 x 8192 M = 3, 4 33.5 -> 25.4]; large layers keep the 4 tiles from M = 9
  if (!r.id.mt && mblocks == 1 && N / 16 > 256 && N / 16 <= 512 && G % 128 == 0) {
    if (KT >= 128) mt_auto = M >= 3 ? 4 : mt_auto;  // (a very long K: four tiles and a 2-way K split, 28672 x 8192 M = 3..8 24.8-25.1 us)
    // [r03 audit, scripts/gpu_small_audit2.sh] up to 320 blocks (N = 5120) four tiles from seven tokens (5120 x 5120 M = 8 .. 16 8.0-9.5 ->
    // 7.6-8.5 us); above, two tiles up to twelve tokens (8192 x 8192 M = 10 11.8 -> 11.0)
    else if (N / 16 <= 320) mt_auto = M >= 7 ? 4 : (M >= 4 ? 2 : mt_auto);
    // (4096 x 6144 keeps two tiles at 13..16 tokens although four with a two-way K split are 2-5 % ahead: the split would cost the
    // RMSNorm prologue of Mistral's fused qkv a launch)
    else if (M >= 4 && (M <= 12 || (long)K * N < 40L * 1000 * 1000)) mt_auto = 2;
  }
  // M = 7, 8 with a long K (>= 10240: the x copy is far beyond the 64 KiB LDS budget) where the exact path would take its fragments
  // from L2 once per 16 channels: two tiles per workgroup share them (8 x 11008 x 4096 10.0 -> 9.2 us, 14336 x 4096 12.2 -> 11.4,
  // 18944 x 3584 14.7 -> 13.1; at M = 6 it is a tie) [audits]
  // (r03 audit: four tiles, 8 x 11008 x 4096 9.3 -> 8.8 us, 8 x 14336 x 4096 11.4 -> 10.3)
  if (!r.id.mt && mt_auto == 1 && M >= 7 && M <= 8 && N / 16 <= 256 && G % 128 == 0 && K >= 10240) mt_auto = 4;
  p.mt = r.id.mt ? r.id.mt : mt_auto;
  if (p.mt != 1 && p.mt != 2) p.mt = 4;
  while (p.mt > 1 && (N / 16) % p.mt != 0) p.mt /= 2;
  p.waves = (r.id.waves == 4 || r.id.waves == 8 || r.id.waves == 16) ? r.id.waves : 8;
  p.ntiles = (N / (16 * p.mt)) * mblocks;
  p.slab_floats = (size_t)p.mt * 256;
  // fill the 256 CUs when N is small: every workgroup should still own >= 8 k-tiles
  int ks = 1;
  while (p.ntiles * ks * 2 <= 256 && KT / (ks * 2) >= 8) ks *= 2;
  p.ksplit = std::max(1, std::min(r.grid_split_k > 0 ? r.grid_split_k : ks, KT));
  p.kt_per_split = (KT + p.ksplit - 1) / p.ksplit;
}

static void shape_tiled(const Req& r, const Pick& k, Plan& p) {
  const int M = r.M, K = r.K, N = r.N, KT = r.KT, mt_req = r.id.mt;
  const bool by_rule = !mt_req && !k.tiled_mt;
  p.mt = mt_req ? (mt_req == 2 ? 2 : (mt_req == 8 ? 8 : 4)) : (k.tiled_mt ? k.tiled_mt : (M <= 32 ? 2 : 4));
  p.waves = r.id.waves == 16 ? 16 : 8;
  int wk = p.wn2 ? 4 : p.waves / 4;
  // 32-token tiles once 64-token tiles would need a 4-way K split to cover the CUs (twice the tiles, half the slices
  // to reduce): M = 65..128 at N = 4096, 15.5 us instead of 16.5 us at M = 128 [r01]
  if (by_rule && p.mt == 4 && (N / 128) * ((M + 63) / 64) * 4 <= 256 && (KT + wk - 1) / wk >= 8) p.mt = 2;
  // ... and at K <= 4096 already where they would need a 2-way split: twice the tiles and nothing to reduce (64 x 4096 x 12288
  // 18.1 -> 17.0 us, 192 x 4096 x 4096 18.2 -> 17.1, 96 / 128 x 4096 x 6144 17.9 -> 16.9 [r02 audit]; with a longer K the split
  // tiles stay ahead: 48 x 8192 x 10240 22.3 against 29.4)
  if (by_rule && p.mt == 4 && k.exact32 && !r.id.force_big && !r.id.force256) p.mt = 2;  // (see exact32 in pick_family)
  if (by_rule && p.mt == 4 && K <= 4096 && !r.id.force_big && !r.id.force256 && (N / 128) * ((M + 63) / 64) * 2 <= 256 &&
      (N / 128) * ((M + 31) / 32) <= 256)
    p.mt = 2;
  // 256-channel tiles (4 channel tiles per wave: one LDS fragment read per four MFMAs instead of two, 2/3 of the L2 -> CU
  // bytes per MAC): M = 1024 at N = 4096 59 -> 50 us, M = 8192 x 22016 772 -> 845 TFLOP/s [r01].  Whether they pay is a
  // matter of how the tiles quantise onto the 256 CUs.  In units of one 128-channel tile alone on its CU: two
  // co-resident 128-channel tiles take ~1.65, a 256-channel tile ~1.5; W wide tiles run in ceil(W / 256) rounds, the
  // 2W narrow ones in full rounds of 512 plus a remainder that runs one or two per CU.  Up to 128 wide tiles they
  // would need a K split and lose (M = 512 at N = 4096: 33.7 against 31.1 us); 129..256 win by 8-10 % (M = 576..960 at
  // N = 4096, 256 x 12288, 128 x 22016, M = 384..512 at K = N = 8192); just above a multiple of 256 the second, nearly
  // empty round loses (192 x 22016: 80 against 70 us; 512 x 11008: 84 against 75) [r01 sweep, one session].
  // Kernel bit 29 forces them, bit 30 forbids them.
  const bool wide_ok = p.mt == 4 && p.waves == 8 && !p.wn2 && !p.ablate && N % 256 == 0 && by_rule;
  const long wtiles = (long)(N / 256) * ((M + 63) / 64);
  const long nfull = 2 * wtiles / 512, nrem = 2 * wtiles % 512;
  const double narrow_cost = 1.65 * nfull + (nrem == 0 ? 0.0 : (nrem <= 256 ? 1.0 : 1.65));
  const double wide_cost = 1.5 * ((wtiles + 255) / 256);
  const bool wide = r.id.force256 || (!r.id.forbid256 && wtiles > 128 && wide_cost < narrow_cost);
  p.tch = wide_ok && wide ? 256 : 128;
  // 128 x 256 tiles run by FOUR waves of 128 tokens x 64 channels each (128 accumulators per lane: at 256 threads hipcc
  // hands out AGPRs, 396 registers, one workgroup per CU): 1.6 VALU and 0.25 LDS fragment reads per MFMA, half the
  // L2 -> CU bytes per MAC of the 64 x 128 tile.  A round of them costs ~1.87 rounds of 64 x 256 tiles for twice the
  // work [r01: M = 2048 at N = 4096 91.6 -> 85.6 us, 8192 x 4096 x 22016 1758 -> 1580 us, 4096 x 8192 x 8192 587 -> 534 us
  // = 1.03 PFLOP/s], so they win where their rounds quantise no worse.  Kernel bit 27 forces them, bit 30 forbids them.
  const long btiles = (long)(N / 256) * ((M + 127) / 128);
  const double big_cost = 1.5 * 1.87 * ((btiles + 255) / 256);
  const bool big = r.id.force_big || (!r.id.forbid256 && !r.id.force256 && btiles > 128 && big_cost < std::min(narrow_cost, wide_cost));
  if (wide_ok && big) {
    p.tch = 256;
    p.mt = 8;
    p.waves = 4;
    wk = 1;  // 4 waves along N, stages of 128 k
  }
  p.ntiles = (N / p.tch) * ((M + p.mt * 16 - 1) / (p.mt * 16));
  p.slab_floats = (size_t)(p.tch / 16) * p.mt * 256;
  // one workgroup per CU: split K until the 256 CUs are covered, keeping >= 2 stages per slice
  const int nstage = (KT + wk - 1) / wk;
  int ks = 1;
  while (p.ntiles * ks * 2 <= 256 && nstage / (ks * 2) >= 2) ks *= 2;
  // ... and not only in powers of two: 80 tiles (Llama-2-70B's qkv, N = 10240) run 3 slices = 240 workgroups,
  // 25.8 us against 29.7 us with 2 at M = 64 [r01]
  if (256 / p.ntiles > ks && nstage / (256 / p.ntiles) >= 2) ks = 256 / p.ntiles;
  p.ksplit = std::max(1, std::min(r.grid_split_k > 0 ? r.grid_split_k : ks, nstage));
  p.kt_per_split = ((nstage + p.ksplit - 1) / p.ksplit) * wk;  // whole stages
  // XCD-aware tile order: (MB/gm) token blocks of 4*BMT*K bytes plus (NB*gm/8) channel blocks of 64*K bytes
  const int MBk = (M + p.mt * 16 - 1) / (p.mt * 16), NBk = N / p.tch;
  p.xcd_gm = xcd_rows(r, (long)MBk * NBk, MBk, NBk, 8, 4L * p.mt, 64);
}

// The skinny launch's x path and dequantisation flavour, once its K split is known
static void skinny_flavour(const Req& r, Plan& p) {
  const int M = r.M, N = r.N, G = r.G, KT = r.KT;
  const int nblocks = N / (16 * p.mt), mblocks = (M + 15) / 16;
  const int cu_req = r.id.slots;  // workgroup slots per CU for a persistent launch, 0 = choose
  p.grid_x = nblocks;
  // Deferred-zero path (M <= 16, one channel tile per workgroup, x and its unit sums in LDS).  It launches PERSISTENT
  // workgroups -- each walks the channel blocks b, b + grid, ... with the chunk pipeline running across blocks -- so
  // that the x copy and the table are paid once per workgroup.  Slots per CU c in {1, 2} (what LDS allows): two
  // co-resident workgroups finish a block each ~1.6x slower than one alone [r01 sweep], so pick the c with the
  // smaller rounds(c) * (c == 1 ? 1 : 1.8).  With M > 2 the copy + table only pay off from two blocks per workgroup
  // [r01: N = 4096, M = 8: 7.1 us against 5.4 us exact]; below that the exact path runs.
  p.dz = false;
  const size_t lds_dz = skinny_lds_bytes(M, G, 1, p.waves, p.kt_per_split, true, true, true);
  const int fit = (int)std::min<size_t>(2, kLdsPerCu / lds_dz);
  if (!r.id.b12 && !r.id.exact && p.mt == 1 && M <= 16 && fit >= 1) {
    int c = 1;
    if (cu_req) c = std::min(cu_req, 8);
    // (r03 audit, scripts/gpu_tiny_audit.sh: 1.8 -- 1792 blocks, 4096 x 28672, run 7 rounds of one per CU in 13.1 us against 4 rounds of
    // two in 13.8 at M = 1 .. 4; 1376 blocks, 4096 x 22016, stay with 3 rounds of two: 10.7 against 11.2)
    else if (fit >= 2 && ((nblocks + 511) / 512) * 1.8 < (double)((nblocks + 255) / 256)) c = 2;
    int rounds = (nblocks + 256 * c - 1) / (256 * c);
    if (!cu_req && M > 2 && rounds < 2 && c == 2) {
      c = 1;
      rounds = (nblocks + 255) / 256;
    }
    // ... and only when the rounds keep the slots busy (384 blocks on 256 slots = 2 rounds at 75 %: Mistral's qkv
    // at M = 16 lost 2 % to the exact path's 384 one-block workgroups [r01])
    const bool balanced = (double)nblocks >= 0.8 * rounds * 256 * c;
    // (M = 3 from 256 blocks as well [third audit: never behind the exact path there, 13824 x 5120 16.3 -> 11.5 us, 4096 x 6144 6.7 -> 6.2,
    // 5120 x 5120 8.0 -> 7.4, 11008 x 4096 8.2 -> 7.9; with 224 blocks, 18944 x 3584, the exact path is ahead 12.8 against 13.9])
    // (r03: M = 4 as well -- with the rows of the x copy / table prologue batched four at a time the table flavour is ahead there too,
    // 4 x 4096 x 4096 4.88 -> 4.60 us, 4 x 11008 x 4096 9.04 -> 8.28 [scripts/gpu_dz.sh]; from 6 tokens the exact path keeps its lead)
    if (M <= 2 || (M <= 4 && nblocks >= 256 && p.ksplit == 1) || r.id.force_table || (rounds >= 2 && balanced && p.ksplit == 1)) {  // bit 26: tests force the path
      p.dz = p.xlds = true;
      if (!r.id.flip && p.ksplit == 1 && rounds >= 2) p.grid_x = std::min(nblocks, ((nblocks + rounds - 1) / rounds + 7) & ~7);
      // One workgroup per CU and a long K: 16 waves instead of 8 -- twice the bytes in flight per CU and half the chain of
      // k-tiles a wave still has to compute after its last load lands.  M = 1, one session [r02]: 11008 x 4096 8.08 -> 7.12 us,
      // 14336 x 4096 8.80 -> 8.44, 28672 x 8192 25.0 -> 23.4 (M = 2: 8.92 -> 7.64); nothing at K = 4096 (4096 x 12288 7.40 ->
      // 7.36), and slower wherever two 8-wave workgroups share a CU (4096 x 22016 10.4 -> 13.0, 8192 x 8192 8.9 -> 11.6).
      // (G = 32: four units per k-tile, 1 x 11008 x 4096 15.1 us with 16 waves against 9.3 -- not there)
      if (!r.id.waves && p.waves == 8 && G >= 64 && p.grid_x <= 256 && p.kt_per_split >= 64 &&
          skinny_lds_bytes(M, G, 1, 16, p.kt_per_split, true, true, true) <= kLdsPerCu)
        p.waves = 16;
    }
  }
  // [r03 audit on the final kernels, 5..16 tokens x 12 layer shapes, scripts/gpu_small_audit2.sh] From five tokens the copy of x into
  // LDS loses to fragments straight from L2 wherever the table flavour above does not run: 5 / 6 x 4096 x 4096 5.1 -> 4.4 / 4.7 us,
  // 5 / 6 x 4096 x 6144 6.6 -> 5.7, 10 x 11008 x 4096 11.9 -> 8.9 (a four-way K split with the copy).  G % 128 == 0 (what was measured).
  const bool l2_frag = G % 128 == 0 && (M >= 5 || (M == 4 && p.mt >= 2));   // (4 x 4096 x 6144, two tiles: 6.2 -> 5.8 us)
  const bool x_fits = (size_t)std::min(M, 16) * (p.kt_per_split * 256 + 16) <= (size_t)64 * 1024;   // (the x copy within 64 KiB)
  if (!p.dz && !r.id.exact && !r.id.no_frag && p.mt >= 2 && G % 128 == 0 &&  // (G < 128: 4 units per tile, spills)
      (r.id.b12 || l2_frag || M > 16 || !x_fits)) {
    // fragment flavour of the deferred-zero path: several channel tiles per workgroup, x fragments straight from L2,
    // the unit sums from one extra MFMA per k-step (kernel bit 28 forbids it)
    p.dz = true;
    p.xlds = false;
  } else if (!p.dz) {
    // exact path: x through LDS while the copy is small (64 KiB), else fragments straight from L2; persistent
    // launches measured within +-5 % of one block per workgroup [r01] and are off unless asked for
    p.xlds = !r.id.b12 && !l2_frag && M <= 16 && x_fits;
    // ... and a one-tile launch with a short K runs sixteen waves (twice the loads in flight per CU; K = 4096: M = 5 .. 16 4.4-5.9 ->
    // 4.3-5.9 us, 3-5 % at 6..12 tokens; at K = 11008 eight waves stay ahead)
    if (l2_frag && !r.id.waves && p.mt == 1 && p.ksplit == 1 && KT <= 32 && mblocks == 1) p.waves = 16;
    const int slots = std::max(1, 256 * (cu_req ? cu_req : 2) / mblocks);
    if (p.xlds && (r.id.flip || cu_req) && p.ksplit == 1 && nblocks > slots) {  // the fragments-from-L2 variants cannot
      const int rounds = (nblocks + slots - 1) / slots;
      p.grid_x = (nblocks + rounds - 1) / rounds;
    }
  }
}

// [r05] 9..16 tokens where the four-tile fragment flavour runs and K / 128 splits into 8 waves x ksplit x T whole k tiles, T in {2, 4, 7, 8}:
// eight tiles per workgroup, straight-line (w4a16_frag8_kernel).  ksplit: one slice from 192 blocks, else the smallest of 2, 4 that gives >= 256 workgroups.
// Forced by kernel id (SKINNY, 8 channel tiles); AUTO takes it where measured ahead (below).
static void skinny_frag8(const Req& r, Plan& p) {
  const int M = r.M, K = r.K, N = r.N, KT = r.KT;
  const bool asked7 = r.id.family == QUICK_KERNEL_SKINNY && r.id.mt == 7;   // (forced: seven tiles per workgroup, T = 8, one slice)
  const bool asked = (r.id.family == QUICK_KERNEL_SKINNY && r.id.mt == 8) || asked7;
  const bool auto_ok = !r.with_ln && r.bare && r.grid_split_k == 0 && p.mt == 4 && p.dz && !p.xlds && (long)K * N >= 60L * 1000 * 1000;
  if (!(asked || auto_ok) || r.G != 128 || M < 9 || M > 16 || N % 128 != 0 || KT % 8 != 0 || r.x_bytes >= ((size_t)1 << 31)) return;
  int best_ks = 0, best_t = 0;
  for (int s2 = 1; s2 <= 4; s2 *= 2) {   // the forced slice count, else the first that gives >= 256 workgroups, else the last one that fits
    if (r.grid_split_k > 0 && s2 != r.grid_split_k) continue;
    if (asked7 && s2 != 1) continue;
    if ((KT / 8) % s2 != 0) continue;
    const int t = KT / 8 / s2;
    if (t != 2 && t != 4 && t != 7 && t != 8) continue;
    best_ks = s2;
    best_t = t;
    if ((N / 128) * s2 >= (s2 == 1 ? 192 : 256)) break;   // (one slice from 192 blocks: a K split costs more than the idle CUs)
  }
  // (AUTO only where measured ahead: 8192 x 57344 one slice 62 -> 54 us, 28672 x 8192 four slices 29.5 -> 27.9, 8192 x 8192 four slices
  // 12.9 -> 11.9; 8192 x 10240 -- 80 blocks -- two slices 17.2 against 15.3: stays with four tiles)
  // ... and 8192 x 28672 -- 224 blocks, one slice -- 28.7 -> 23.5: one slice from 192 blocks, K slices only on whole multiples of 64 blocks)
  // (128 blocks x two slices, 8192 x 16384: 16.4 -> 18.5 us, behind: K slices only where measured ahead, 64 blocks x four)
  if (best_ks && !asked && !((best_ks == 1 && N / 128 >= 192) || (N / 128 == 64 && best_ks == 4))) best_ks = 0;
  if (asked7 && !(best_ks == 1 && best_t == 8 && N % 112 == 0)) best_ks = 0;
  if (!best_ks) return;
  p.mt = 8;
  p.waves = 8;
  p.dz = true;
  p.xlds = false;
  p.frag8_t = best_t;
  p.ksplit = best_ks;
  p.kt_per_split = 8 * best_t;
  p.grid_x = N / 128;
  p.ntiles = (N / 128) * ((M + 15) / 16);
  p.slab_floats = (size_t)8 * 256;
  // [r06, late] seven tiles per workgroup where that makes fewer or fuller rounds of one workgroup per CU (one slice, T = 8 only -- K = 8192): a round costs
  // its weights + its x fragments (x: as many bytes as four tiles' weights), so 7 + 4 against 8 + 4 per round.  16 x 8192 x 57344: 448 blocks = 2 rounds (the
  // second three quarters full) -> 512 blocks = 2 full rounds of less; the forced eight-tile id keeps eight.
  if (best_ks == 1 && best_t == 8 && N % 112 == 0 && (asked7 || !asked)) {
    const int cus = cu_count();
    const long cost8 = (long)((N / 128 + cus - 1) / cus) * 12, cost7 = (long)((N / 112 + cus - 1) / cus) * 11;
    if (asked7 || cost7 < cost8) {
      p.mt = 7;
      p.grid_x = N / 112;
      p.ntiles = (N / 112) * ((M + 15) / 16);
      p.slab_floats = (size_t)7 * 256;
    }
  }
}

// with_ln: the launch carries an RMSNorm prologue -- AUTO keeps to the kernels that have one (no mid-token, no eight-tile fragment launch)
static Plan make_plan(int M, int K, int N, int G, int kernel, int grid_split_k, bool allow_xk = true, bool with_ln = false) {
  const KernelId id = decode_kernel_id(kernel);
  const Req r{M, K, N, G, K / 128, grid_split_k, id, id.family == QUICK_KERNEL_AUTO && !id.mt && !id.waves && !id.high, allow_xk, with_ln,
              (size_t)M * K * 2, (size_t)M * N * 2, (size_t)K * N / 2};
  Plan p{};
  p.ablate = id.ablate;
  p.wn2 = id.b15;
  if (plan_lean(r, p) || plan_xm(r, p)) return p;
  const Pick k = pick_family(r);
  p.est_us = k.est_us;
  p.est_xw_us = k.est_xw_us;
  p.kernel = within_limits(r, k);
  if (p.kernel == QUICK_KERNEL_XW) shape_xw(r, k, p);
  else if (p.kernel == QUICK_KERNEL_XK) shape_xk(r, k, p);
  else if (p.kernel == QUICK_KERNEL_WIDE) shape_wide(r, k, p);
  else if (p.kernel == QUICK_KERNEL_SKINNY) shape_skinny(r, p);
  else shape_tiled(r, k, p);
  p.ksplit = (r.KT + p.kt_per_split - 1) / p.kt_per_split;
  if (p.kernel == QUICK_KERNEL_SKINNY) {
    skinny_flavour(r, p);
    skinny_frag8(r, p);
  }
  // [r06] sixteen waves (128 registers per lane): one-tile workgroups, and the table flavour only with <= 2 units per k tile -- the other builds
  // spilled registers and were never the planner's own pick; a forced request runs eight waves
  if (p.kernel == QUICK_KERNEL_SKINNY && p.waves == 16 && (p.mt != 1 || (p.dz && group_mode(G) > 2))) p.waves = 8;
  return p;
}

// The planner does not see the epilogue: where AUTO picks an exchange-K launch that cannot carry SiLU * mul, a SiLU * mul launch runs the
// plan without those kernels (and without the RMSNorm prologue's restrictions).  The workspace must serve either.
static bool silu_replans(int kernel, const Plan& p) { return decode_kernel_id(kernel).family == QUICK_KERNEL_AUTO && p.kernel == QUICK_KERNEL_XK && !xk_takes_silu(p); }

Plan plan_for(int M, int K, int N, int G, int kernel, int grid_split_k, bool silu, bool with_ln) {
  const Plan p = make_plan(M, K, N, G, kernel, grid_split_k, true, with_ln);
  return silu && silu_replans(kernel, p) ? make_plan(M, K, N, G, kernel, grid_split_k, false) : p;
}

size_t plan_workspace_bytes(int M, int K, int N, int G, int kernel, int grid_split_k) {
  const Plan p = make_plan(M, K, N, G, kernel, grid_split_k);
  const size_t need = workspace_need(p);
  return silu_replans(kernel, p) ? std::max(need, workspace_need(make_plan(M, K, N, G, kernel, grid_split_k, false))) : need;
}

// The RMSNorm prologue: the lean kernels, and the deferred-zero skinny kernels with one K slice (the table flavour, or the fragment flavour
// with eight waves), not the straight-line fragment kernel
bool plan_takes_rmsnorm(const Plan& p) {
  return p.kernel == QUICK_KERNEL_LEAN || (p.kernel == QUICK_KERNEL_SKINNY && p.dz && p.ksplit == 1 && !p.frag8_t && (p.xlds || (p.mt >= 2 && p.waves == 8)));
}

void plan_describe(int M, int K, int N, int G, int kernel, int grid_split_k, char* text, size_t text_bytes) {
  const Plan p = make_plan(M, K, N, G, kernel, grid_split_k);
  if (p.kernel == QUICK_KERNEL_LEAN)
    snprintf(text, text_bytes, "lean ntw=%d waves=%d tiles_per_wave<=%d grid=%dx%d lds=%u workspace=0", p.mt, p.waves, p.lean_tmax, p.grid_x, (M + 15) / 16,
             lean_lds_need(M, K, p.waves, p.mt, false));
  else if (p.kernel == QUICK_KERNEL_XM)
    snprintf(text, text_bytes, "xm tokens=%d channels=%d waves=8 grid=%dx%d lds=%u workspace=0", p.wide_mb * 32, p.wide_pairs * 32, p.grid_x, p.ntiles / p.grid_x,
             xm_lds_need(p.wide_mb, p.wide_pairs));
  else if (p.kernel == QUICK_KERNEL_SKINNY)
    snprintf(text, text_bytes, "skinny ntw=%d waves=%d x=%s dequant=%s grid=%dx%dx%d ksplit=%d workspace=%zu", p.mt, p.waves,
             p.xlds ? "lds" : "l2", p.dz ? (p.xlds ? "deferred-zero-table" : "deferred-zero-fragment") : "exact", p.grid_x,
             (M + 15) / 16, p.ksplit, p.ksplit, workspace_need(p));
  else if (p.kernel == QUICK_KERNEL_XW)
  {
    char stg[16] = "";
    if (p.xw_stagger) snprintf(stg, sizeof stg, " stagger=%d", p.xw_stagger);
    snprintf(text, text_bytes, "xw tokens=%d channels=%d waves=4 ring=%d queue=%d grid=%d slices=%d xcd_rows=%d%s workspace=%zu", p.wide_mb * 32, p.tch,
             p.wide_mb == 2 ? 8 : (p.wide_mb == 8 ? 2 : 4), p.wide_mb == 2 ? 8 : (p.wide_mb == 8 ? 2 : 4), p.ntiles * p.ksplit, p.ksplit, p.xcd_gm, stg, workspace_need(p));
  }
  else if (p.kernel == QUICK_KERNEL_XK)
    snprintf(text, text_bytes, "xk tokens=%d channels=128 waves=%d ring=%d queue=%d grid=%d slices=%d xcd_rows=%d workspace=%zu", p.wide_mb * 32,
             p.xk_loader ? 12 : (p.xk_kq == 4 ? 16 : 8), p.xk_loader ? 3 : p.xk_nbuf, p.xk_loader ? 5 : p.xk_wd, p.ntiles * p.ksplit, p.ksplit, p.xcd_gm, workspace_need(p));
  else if (p.kernel == QUICK_KERNEL_WIDE)
    snprintf(text, text_bytes, "wide tokens=%d channels=%d waves=%d ring=%d grid=%dx%d ksplit=%d xcd_rows=%d workspace=%zu", p.wide_mb * 32,
             p.tch, p.waves, p.wide_nbuf, p.ntiles, p.ksplit, p.ksplit, p.xcd_gm, workspace_need(p));
  else
    snprintf(text, text_bytes, "tiled tokens=%d channels=%d waves=%d grid=%dx%d ksplit=%d xcd_rows=%d workspace=%zu", p.mt * 16,
             p.tch, p.wn2 ? 8 : p.waves, p.ntiles, p.ksplit, p.ksplit, p.xcd_gm, workspace_need(p));
  if ((p.est_us > 0 || p.est_xw_us > 0) && getenv("QUICK_AMD_PLAN_ESTIMATES")) {   // (the launch-time models' estimates, for planner audits)
    const size_t n = strlen(text);
    if (n + 40 < text_bytes) snprintf(text + n, text_bytes - n, " est=%.1f est_xw=%.1f", p.est_us, p.est_xw_us);
  }
}

}  // namespace quick_amd
