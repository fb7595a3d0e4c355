// quick_prefill_attention_f16 and its describe: the shared-position form of the kernel in prefill_attention.hpp.
#define PA_KERNEL prefill_attention_kernel
#define PA_SEQ false
#include "prefill_attention.hpp"

using namespace quick_amd;

extern "C" {

int quick_prefill_attention_f16(const void* q, const void* k_cache, const void* v_cache, const void* pos0, void* out, int batch,
                                int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, float scale, void* hip_stream) {
  return prefill_attention_launch(q, k_cache, v_cache, pos0, out, batch, tokens, n_heads, n_kv_heads, head_dim, cache_len, scale,
                                         hip_stream);
}

int quick_prefill_attention_describe(int batch, int tokens, int n_heads, int n_kv_heads, int head_dim, int cache_len, char* text,
                                     size_t text_bytes) {
  const int rc = prefill_attention_check(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len);
  if (rc != QUICK_OK) return rc;
  if (!text || text_bytes == 0) return set_last_error(QUICK_ERR_INVALID_ARGUMENT, "prefill attention: no room for the description");
  snprintf(text, text_bytes, "prefill-mfma q_rows=%d kv_rows=%d waves=%d grid=%dx%dx%d", PA_QROWS, PA_KVROWS, PA_WAVES,
           (tokens + PA_QROWS - 1) / PA_QROWS, n_heads, batch);
  return QUICK_OK;
}

}  // extern "C"
