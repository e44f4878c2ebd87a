// pack.h -- host only: the one walk "matrix view -> weight fragments" behind every *_pack_host.  The layouts themselves are defined where
// the kernels read them (common.h: frag_index; split3.h: qfrag_put; split2.h: hfrag_put; split_scheme.h: put_host); this header only
// visits the elements.  A matrix view is a callable (row, k) -> float that returns 0 outside the matrix.
#pragma once
#include "split_scheme.h"

namespace vadx {
namespace pack {

// float32, fragment-major: element (r, k) of src for r < rows, k < cols into the [.][ldw] matrix at dst (common.h: frag_index)
template <class Src>
void f32(float *dst, int ldw, int rows, int cols, Src src) {
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) dst[frag_index(ldw, r, k)] = src(r, k);
}

// One (16-row tile, 32-k chunk) of scheme Sch: src(i, k), i < 16, k < 32, into the NP plane fragments at frags; wmax as Sch::put_host
template <class Sch, class Src>
void group(float *frags, Src src, float &wmax) {
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 32; ++k) Sch::put_host(frags, i, k, src(i, k), wmax);
}

// A whole matrix in the plain section order [tiles][chunks][NP planes][QFRAG]
template <class Sch, class Src>
void split(float *dst, int tiles, int chunks, Src src, float &wmax) {
    for (int nt = 0; nt < tiles; ++nt)
        for (int kc = 0; kc < chunks; ++kc)
            group<Sch>(dst + (size_t)((nt * chunks + kc) * Sch::NP) * QFRAG, [&](int i, int k) { return src(16 * nt + i, 32 * kc + k); }, wmax);
}

// ... in the arithmetic a run-time plane count names: np = 3 bf16 x 3, 2 fp16 x 2, 0 none (float32 MFMAs keep no split copy)
template <class Src>
void split(int np, float *dst, int tiles, int chunks, Src src, float &wmax) {
    if (np == SchemeB3::NP) split<SchemeB3>(dst, tiles, chunks, src, wmax);
    else if (np == SchemeH2::NP) split<SchemeH2>(dst, tiles, chunks, src, wmax);
}

// the view of a plain row-major [rows][cols] matrix
inline auto rowmajor(const float *w, int rows, int cols) {
    return [=](int r, int k) { return (r < rows && k < cols) ? w[(size_t)r * cols + k] : 0.f; };
}

// row-major [rows][cols] -> row-major with leading dimension ld (the form frag_major_inplace converts)
inline void rows_ld(float *dst, const float *src, int rows, int cols, int ld) {
    for (int r = 0; r < rows; ++r) memcpy(dst + (size_t)r * ld, src + (size_t)r * cols, cols * sizeof(float));
}

}  // namespace pack
}  // namespace vadx
