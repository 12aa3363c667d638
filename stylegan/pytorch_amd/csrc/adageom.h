// Device side shared by the two bilinear resamples of the geometric group (adageom.hip: zero padding; adageompad.hip: reflection
// padding): the table row, the identity test, THE position and weight expressions, the accumulation step, and the adjoint's candidate
// box and the walk over it.  Both files compute s_p and w through geom_pos / geom_w, so a coefficient is the same fp32 number in the
// forward and the adjoint of either padding, and where no tap leaves the image the two paddings agree bit for bit.
#pragma once
#include "aug.h"

constexpr int DG_BLOCK = 256;
constexpr float DG_MARGIN = 0.03125f;               // slack of the adjoint's candidate box, in pixels (covers T T^-1 != I in fp32)
// The tile kernels: a block owns a DG_TILE x DG_TILE output tile of one image, a wave eight rows of it, and in each of its four trips
// the wave's lanes are an 8 x 8 patch of pixels (lane = 8 row + column).
constexpr int DG_TILE = 32;
static_assert(DG_TILE * DG_TILE == 4 * DG_BLOCK && DG_TILE == 4 * 8 && DG_BLOCK == 4 * WAVE, "four waves of eight rows, four 8 x 8 patches each");

typedef float f32x3u __attribute__((ext_vector_type(3), aligned(4)));   // one 12-byte pixel at a 4-byte aligned address (dwordx3)

struct DgMat { float i00, i01, i10, i11, t00, t01, t10, t11; };

__device__ __forceinline__ DgMat dg_load_mat(const float* __restrict__ m) {
    DgMat q;
    q.i00 = m[0]; q.i01 = m[1]; q.i10 = m[2]; q.i11 = m[3]; q.t00 = m[4]; q.t01 = m[5]; q.t10 = m[6]; q.t11 = m[7];
    return q;
}

__device__ __forceinline__ bool dg_identity(const DgMat& q) {
    return q.i00 == 1.f && q.i01 == 0.f && q.i10 == 0.f && q.i11 == 1.f && q.t00 == 1.f && q.t01 == 0.f && q.t10 == 0.f && q.t11 == 1.f;
}

// s_p = c + T^-1 (p - c) for the output pixel p = (column j, row i): THE position expression of the forward and the adjoint.
__device__ __forceinline__ void geom_pos(const DgMat& q, float cx, float cy, int i, int j, float& sx, float& sy) {
    const float dx = __fsub_rn((float)j, cx), dy = __fsub_rn((float)i, cy);
    sx = __fadd_rn(cx, __fadd_rn(__fmul_rn(q.i00, dx), __fmul_rn(q.i01, dy)));
    sy = __fadd_rn(cy, __fadd_rn(__fmul_rn(q.i10, dx), __fmul_rn(q.i11, dy)));
}

// w(s, t) = max(0, 1 - |s_x - t_x|) max(0, 1 - |s_y - t_y|): THE weight expression of the forward and the adjoint.
__device__ __forceinline__ float geom_w(float sx, float sy, int tx, int ty) {
    const float wx = fmaxf(0.f, __fsub_rn(1.f, fabsf(__fsub_rn(sx, (float)tx))));
    const float wy = fmaxf(0.f, __fsub_rn(1.f, fabsf(__fsub_rn(sy, (float)ty))));
    return __fmul_rn(wx, wy);
}

__device__ __forceinline__ void dg_acc(float (&acc)[3], float w, const float* __restrict__ px) {
    const f32x3u v = *reinterpret_cast<const f32x3u*>(px);
    acc[0] = __fadd_rn(acc[0], __fmul_rn(w, v.x));
    acc[1] = __fadd_rn(acc[1], __fmul_rn(w, v.y));
    acc[2] = __fadd_rn(acc[2], __fmul_rn(w, v.z));
}

struct DgBox { float ex, ey; int nx, ny; };                     // the adjoint's candidate box: half extents (with the slack) and trip counts

template <bool ADJ>
__device__ __forceinline__ DgBox dg_box(const DgMat& q) {
    DgBox bx = {0.f, 0.f, 0, 0};
    if (ADJ) {
        bx.ex = fabsf(q.t00) + fabsf(q.t01) + DG_MARGIN; bx.ey = fabsf(q.t10) + fabsf(q.t11) + DG_MARGIN;
        bx.nx = min((int)floorf(2.f * bx.ex) + 1, 7); bx.ny = min((int)floorf(2.f * bx.ey) + 1, 7);
    }
    return bx;
}

// The adjoint's candidate walk for the tap position q = (row qi, column qj): the candidates p are the integers of the box centre +-
// (extent + margin), centre = c + T (q - c), extent = (|t00| + |t01|, |t10| + |t11|); nx, ny (the trip counts) come from the matrix
// alone.  Candidates are visited row by row, those with a zero weight or outside the image skipped, and added to acc.  q need not be
// a pixel: the reflection padding walks the mirror positions of a pixel, which lie outside the image.
__device__ __forceinline__ void dg_adj_walk(const float* __restrict__ gb, int H, int W, const DgMat& q, float cx, float cy, float ex, float ey,
                                            int nx, int ny, int qi, int qj, float (&acc)[3]) {
    const float dx = (float)qj - cx, dy = (float)qi - cy;
    const float px = cx + (q.t00 * dx + q.t01 * dy), py = cy + (q.t10 * dx + q.t11 * dy);
    if (!(px > -8.f && px < (float)W + 8.f && py > -8.f && py < (float)H + 8.f)) return;      // the whole box is outside
    const int j0 = (int)ceilf(px - ex), i0 = (int)ceilf(py - ey);
    for (int di = 0; di < ny; ++di) {
        const int i = i0 + di;
        if (i < 0 || i >= H) continue;
        for (int dj = 0; dj < nx; ++dj) {
            const int j = j0 + dj;
            if (j < 0 || j >= W) continue;
            float sx, sy;
            geom_pos(q, cx, cy, i, j, sx, sy);
            const float w = geom_w(sx, sy, qj, qi);
            if (w > 0.f) dg_acc(acc, w, gb + ((size_t)i * W + j) * 3);
        }
    }
}
