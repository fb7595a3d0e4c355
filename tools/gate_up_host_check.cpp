// Host run of the gate / up interleave kernels' lane function (quick_amd/csrc/gate_up_mi355x.hpp) over heap buffers of the exact tensor
// sizes, walking the grid the library launches: built with -fsanitize=address,undefined by tools/gate_up_host_check.py, any index out of
// bounds or misaligned piece ends the run.  Usage: gate_up_host_check K I G in.bin out.bin
//   in.bin  = gate qweight | gate scales | gate qzeros | up qweight | up scales | up qzeros   (mi355x order, raw bytes)
//   out.bin = fused qweight | scales | qzeros, then the six tensors the split makes of them
#include <cstdio>
#include <cstdlib>
#include <cstring>

// the header is HIP source; this program is plain C++
#define __host__
#define __device__
#define __forceinline__ inline
#include "../quick_amd/csrc/gate_up_mi355x.hpp"

using quick_amd::gate_up_piece;

static gate_up_piece* alloc(size_t bytes, int fill) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes) != 0) exit(3);
  memset(p, fill, bytes);
  return (gate_up_piece*)p;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int K = atoi(argv[1]), I = atoi(argv[2]), G = atoi(argv[3]), NG = K / G;
  const size_t bytes[3] = {(size_t)K * I / 2, (size_t)NG * I * 4, (size_t)NG * I};   // of one projection: qweight, scales, qzeros
  gate_up_piece *in[6], *fused[3], *back[6];
  FILE* f = fopen(argv[4], "rb");
  if (!f) return 3;
  for (int t = 0; t < 6; ++t) {
    in[t] = alloc(bytes[t % 3], 0);
    if (fread(in[t], 1, bytes[t % 3], f) != bytes[t % 3]) return 3;
    back[t] = alloc(bytes[t % 3], 0xa5);
  }
  fclose(f);
  for (int t = 0; t < 3; ++t) fused[t] = alloc(2 * bytes[t], 0xa5);
  const unsigned wblocks = (unsigned)(((size_t)K * I / 16 + 255) / 256), sblocks = (unsigned)(((size_t)NG * I / 2 + 255) / 256);
  const unsigned zblocks = (unsigned)(((size_t)NG * (I / 16) + 255) / 256);
  for (unsigned b = 0; b < wblocks + sblocks + zblocks; ++b)
    for (unsigned t = 0; t < 256; ++t)
      quick_amd::gate_up_mi355x_lane<false>(in[0], in[1], in[2], in[3], in[4], in[5], fused[0], fused[1], fused[2], K, I, NG, wblocks, sblocks, b, t);
  for (unsigned b = 0; b < wblocks + sblocks + zblocks; ++b)
    for (unsigned t = 0; t < 256; ++t)
      quick_amd::gate_up_mi355x_lane<true>(back[0], back[1], back[2], back[3], back[4], back[5], fused[0], fused[1], fused[2], K, I, NG, wblocks, sblocks, b, t);
  f = fopen(argv[5], "wb");
  if (!f) return 3;
  for (int t = 0; t < 3; ++t) fwrite(fused[t], 1, 2 * bytes[t], f);
  for (int t = 0; t < 6; ++t) fwrite(back[t], 1, bytes[t % 3], f);
  fclose(f);
  for (int t = 0; t < 6; ++t) free(in[t]), free(back[t]);
  for (int t = 0; t < 3; ++t) free(fused[t]);
  return 0;
}
