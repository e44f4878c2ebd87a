// capi.hip -- error plumbing and the weight-layout helper shared by every libvadx entry point.
#include "common.h"
#include "pack.h"

#include <stdlib.h>
#include <string.h>

namespace vadx {
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace vadx

extern "C" int vadx_abi_version(void) { return VADX_ABI_VERSION; }      // include/vadx.h is the one place the number lives
extern "C" const char *vadx_last_error(void) { return vadx::g_err; }

extern "C" size_t vadx_frag_major_floats(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)((rows + 15) & ~15) * (size_t)((cols + 15) & ~15);
}

extern "C" int vadx_frag_major_host(const float *src, int rows, int cols, float *dst) {
    VADX_REQUIRE(src && dst && rows > 0 && cols > 0, "vadx_frag_major_host: bad argument");
    const int ldw = (cols + 15) & ~15;
    const size_t n = vadx_frag_major_floats(rows, cols);
    for (size_t e = 0; e < n; ++e) dst[e] = 0.f;
    vadx::pack::f32(dst, ldw, rows, cols, vadx::pack::rowmajor(src, rows, cols));
    return VADX_OK;
}

// fp16 x 2 fragments of a [rows][cols] weight matrix for the entry points that take bare weight pointers (include/vadx.h):
// [rows/16 tiles][cols/32 chunks][2 planes][64 lanes][8 fp16]; lane 16 q + i, slot e holds W[16 tile + i][32 chunk + k(q, e)] with
//   VADX_H2_K_PLAIN    k = 8 q + e                       (operand planes [k / 8][column][8]: layers_split.h)
//   VADX_H2_K_QUARTER  k = 16 (e >> 2) + 4 q + (e & 3)   (the order in which marblenet.hip's kgemm_h reads k-major float32 rows without
//                                                         bank conflicts)
extern "C" size_t vadx_frag_h2_floats(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)((rows + 15) / 16) * (size_t)((cols + 31) / 32) * 2 * vadx::HFRAG;
}

extern "C" int vadx_frag_h2_host(const float *src, int rows, int cols, int k_order, float *dst, float *wmax_out) {
    VADX_REQUIRE(src && dst && rows > 0 && cols > 0, "vadx_frag_h2_host: bad argument");
    VADX_REQUIRE(k_order == VADX_H2_K_PLAIN || k_order == VADX_H2_K_QUARTER, "vadx_frag_h2_host: k_order must be VADX_H2_K_PLAIN or VADX_H2_K_QUARTER");
    const int nch = (cols + 31) / 32;
    float wmax = 0.f;
    const auto w = vadx::pack::rowmajor(src, rows, cols);
    if (k_order == VADX_H2_K_QUARTER)       // fragment position 8 q + e of a chunk holds its k = 16 (e >> 2) + 4 q + (e & 3)
        vadx::pack::split<vadx::SchemeH2>(dst, (rows + 15) / 16, nch, [&](int r, int c) { return w(r, (c & ~31) + 16 * ((c & 7) >> 2) + 4 * ((c & 31) >> 3) + (c & 3)); }, wmax);
    else
        vadx::pack::split<vadx::SchemeH2>(dst, (rows + 15) / 16, nch, w, wmax);
    if (wmax_out) *wmax_out = wmax;
    VADX_REQUIRE(wmax <= vadx::H_MAX, "vadx_frag_h2_host: a weight (|w| = %g) is outside the fp16 range: keep this matrix on VADX_ARITH_F32", (double)wmax);
    return VADX_OK;
}
