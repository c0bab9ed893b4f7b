// Library-wide state: the calling thread's last error text, the ABI version and the A/B switches (common.h).
#include <stdarg.h>

#include "common.h"

static thread_local char g_err[512] = "";

void igcn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* igcn_last_error(void) { return g_err; }
extern "C" int igcn_version(void) { return IGCN_ABI_VERSION; }

unsigned g_igcn_options = 0;
int g_igcn_gemm_bn_cap = 0;
int g_igcn_attn_chunk_rows = 0;
extern "C" int igcn_configure(unsigned options, int gemm_bn_cap, int attn_chunk_rows) {
  g_igcn_options = options;
  g_igcn_gemm_bn_cap = gemm_bn_cap;
  g_igcn_attn_chunk_rows = attn_chunk_rows;
  return IGCN_OK;
}
