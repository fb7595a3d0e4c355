// quick_prefill_attention_seq_f16: the per-sequence form of the kernel in prefill_attention.hpp, in a unit of its own (see there).
#define PA_KERNEL prefill_attention_seq_kernel
#define PA_SEQ true
#include "prefill_attention.hpp"

using namespace quick_amd;

extern "C" {

int quick_prefill_attention_seq_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                    int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, void* hip_stream) {
  return prefill_attention_launch(q, k_cache, v_cache, pos0, out, batch, tokens, n_heads, n_kv_heads, head_dim, cache_len, scale,
                                        hip_stream);
}

}  // extern "C"
