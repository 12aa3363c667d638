// The general geometric group of the ADA paper (Karras et al., NeurIPS 2020) on the discriminator's fp32 RGB input: isotropic scale,
// arbitrary rotation and anisotropic scale of one image composed into ONE affine map T about the image centre, applied by a single
// bilinear resample (definitions in include/sgx.h):
//   y(p) = sum_t w(s_p, t) x(t)        forward: the four taps t = floor(s_p) + {0,1}^2 inside the image, s_p = c + T^-1 (p - c)
//   z(q) = sum_p w(s_p, q) g(p)        adjoint: the output pixels p whose taps include q, found from the bounding box of T(q + (-1,1)^2)
// Both are gathers (no atomics: bit-reproducible), and both compute the position s_p and the weight w with the SAME expression
// (geom_pos, geom_w: every product and sum rounded to fp32 on its own), so the adjoint's coefficients are the forward's bit for bit.
// sgx_ada_geom_matrix turns one D evaluation's draws (and, under ADA, its gate uniforms against p) into the per-image table
// {T^-1, T} once; the forward, the adjoint and the R1 double backward read the table, never p.  An image with its three ops off gets
// the exact identity row, which IS its flag: both resample kernels copy such an image (a block-uniform branch).
#include "adageom.h"

enum { DG_SCALE = 32, DG_ROTATE = 64, DG_ANISO = 128, DG_OPS = DG_SCALE | DG_ROTATE | DG_ANISO };

// z = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3);  2^(0.2 z)
__device__ __forceinline__ float dg_lognormal(float ua, float ub) {
    const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, ua))));
    const float z = __fmul_rn(r, cosf(__fmul_rn(6.283185307179586f, ub)));
    return exp2f(__fmul_rn(0.2f, fminf(fmaxf(z, -3.f), 3.f)));
}

__global__ __launch_bounds__(DG_BLOCK) void ada_geom_matrix_kernel(const float* __restrict__ u, int u_stride, const float* __restrict__ gu,
                                                                   int gu_stride, const float* __restrict__ state, int policy,
                                                                   float* __restrict__ mat, int B) {
    const int b = blockIdx.x * DG_BLOCK + threadIdx.x;
    if (b >= B) return;
    int on = policy;
    if (gu) {
        const float p = state[0];
        const float* g = gu + (size_t)gu_stride * b;
        on &= (g[0] < p ? DG_SCALE : 0) | (g[1] < p ? DG_ROTATE : 0) | (g[2] < p ? DG_ANISO : 0);
    }
    float* m = mat + 8 * (size_t)b;
    if (!(on & DG_OPS)) {                                        // the identity row: what the resample kernels copy under
        m[0] = 1.f; m[1] = 0.f; m[2] = 0.f; m[3] = 1.f; m[4] = 1.f; m[5] = 0.f; m[6] = 0.f; m[7] = 1.f;
        return;
    }
    const float* ub = u + (size_t)u_stride * b;
    const float s = (on & DG_SCALE) ? dg_lognormal(ub[0], ub[1]) : 1.f;
    const float th = (on & DG_ROTATE) ? __fmul_rn(6.283185307179586f, __fsub_rn(ub[2], 0.5f)) : 0.f;
    const float a = (on & DG_ANISO) ? dg_lognormal(ub[3], ub[4]) : 1.f;
    const float sx = __fmul_rn(s, a), sy = __fdiv_rn(s, a);
    const float c = cosf(th), sn = sinf(th);
    // T = Rot(th) diag(sx, sy) on (column, row);  T^-1 = diag(1/sx, 1/sy) Rot(-th)
    m[0] = __fdiv_rn(c, sx); m[1] = __fdiv_rn(sn, sx); m[2] = __fdiv_rn(-sn, sy); m[3] = __fdiv_rn(c, sy);
    m[4] = __fmul_rn(c, sx); m[5] = __fmul_rn(-sn, sy); m[6] = __fmul_rn(sn, sx); m[7] = __fmul_rn(c, sy);
}

// Forward value of output pixel (i, j): taps in the order (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1), those outside the image
// skipped.  A position far outside (|s| beyond the int range cannot occur: |T^-1| <= 2.3 and the image is < 2^31 / 3 floats).
__device__ __forceinline__ void dg_fwd_px(const float* __restrict__ xb, int H, int W, const DgMat& q, float cx, float cy, int i, int j,
                                          float (&acc)[3]) {
    float sx, sy;
    geom_pos(q, cx, cy, i, j, sx, sy);
    acc[0] = acc[1] = acc[2] = 0.f;
    if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return;     // no tap inside (also: NaN positions of a bad table)
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int tx = x0 + dx, ty = y0 + dy;
            if (tx >= 0 && tx < W && ty >= 0 && ty < H) dg_acc(acc, geom_w(sx, sy, tx, ty), xb + ((size_t)ty * W + tx) * 3);
        }
    }
}

// Adjoint value of pixel q = (row qi, column qj): the candidate walk of dg_adj_walk (adageom.h) from +0.
__device__ __forceinline__ void dg_adj_px(const float* __restrict__ gb, int H, int W, const DgMat& q, float cx, float cy, float ex, float ey,
                                          int nx, int ny, int qi, int qj, float (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.f;
    dg_adj_walk(gb, H, W, q, cx, cy, ex, ey, nx, ny, qi, qj, acc);
}

// Any H, W, any 4-byte aligned base: one pixel per thread in row order, one trip (short-lived blocks).  grid (ceil(H W / DG_BLOCK), B).
template <bool ADJ>
__global__ __launch_bounds__(DG_BLOCK) void ada_geom_px_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                               int H, int W) {
    const int b = blockIdx.y;
    const DgMat q = dg_load_mat(mat + 8 * (size_t)b);
    const int unit = blockIdx.x * DG_BLOCK + threadIdx.x;
    if (unit >= H * W) return;
    const int i = unit / W, j = unit - i * W;
    const size_t at = ((size_t)b * H * W + unit) * 3;
    float acc[3];
    if (dg_identity(q)) {                                        // (block-uniform) a copy, bit for bit
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = x[at + k];
    } else {
        const float* xb = x + (size_t)b * H * W * 3;
        const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
        const DgBox bx = dg_box<ADJ>(q);
        if (ADJ) dg_adj_px(xb, H, W, q, cx, cy, bx.ex, bx.ey, bx.nx, bx.ny, i, j, acc);
        else dg_fwd_px(xb, H, W, q, cx, cy, i, j, acc);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) y[at + k] = acc[k];
}

// W % 4 == 0, 16-byte aligned bases.  A block owns a DG_TILE x DG_TILE output tile of one image, a wave eight rows of it, and in each
// of its four trips the wave's lanes are an 8 x 8 patch of pixels (lane = 8 row + column).  An affine map takes the patch to a small
// parallelogram of the source, so the 64 addresses of one tap load fall on a dozen cache lines; with the lanes of a wave laid along a
// row instead (the first version: four consecutive pixels per lane) a turned image spread them over 64 lines, and the launch cost 6 to
// 11 times the blit tile kernel's.  An identity image is copied in row order, four pixels (three 16-byte loads
// and stores) per thread: the grid's DG_TILE^2-pixel tiles are at least as many as its DG_TILE^2-pixel runs.
// grid (ceil(H / DG_TILE) * ceil(W / DG_TILE), B).
template <bool ADJ>
__global__ __launch_bounds__(DG_BLOCK) void ada_geom_tile_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                                 int H, int W, int tiles_x) {
    const int b = blockIdx.y;
    const DgMat q = dg_load_mat(mat + 8 * (size_t)b);
    const float* xb = x + (size_t)b * H * W * 3;
    float* yb = y + (size_t)b * H * W * 3;
    if (dg_identity(q)) {                                        // (block-uniform) a copy, bit for bit
        const int unit = blockIdx.x * DG_BLOCK + threadIdx.x;
        if (unit >= H * (W / 4)) return;
        const float4* s = reinterpret_cast<const float4*>(xb + (size_t)unit * 12);
        const float4 v0 = s[0], v1 = s[1], v2 = s[2];
        float4* d = reinterpret_cast<float4*>(yb + (size_t)unit * 12);
        d[0] = v0; d[1] = v1; d[2] = v2;
        return;
    }
    const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = ti * DG_TILE + (threadIdx.x / WAVE) * 8 + (lane >> 3);
    if (i >= H) return;
    const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
    const DgBox bx = dg_box<ADJ>(q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = tj * DG_TILE + 8 * k + (lane & 7);
        if (j >= W) continue;
        float acc[3];
        if (ADJ) dg_adj_px(xb, H, W, q, cx, cy, bx.ex, bx.ey, bx.nx, bx.ny, i, j, acc);
        else dg_fwd_px(xb, H, W, q, cx, cy, i, j, acc);
        f32x3u v; v.x = acc[0]; v.y = acc[1]; v.z = acc[2];
        *reinterpret_cast<f32x3u*>(yb + ((size_t)i * W + j) * 3) = v;
    }
}

extern "C" int sgx_ada_geom_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat,
                                   int B, void* stream) {
    if (int rc = aug_check_matrix("ada_geom_matrix", u, u_stride, 5, gu, gu_stride, 3, state, mat, B, policy_bits, DG_OPS, "scale 32, rotate 64, aniso 128"))
        return rc;
    SGX_NOTE(0.0, (20.0 + (gu ? 16.0 : 0.0) + 32.0) * B, "ada_geom_matrix B%d", B);
    hipLaunchKernelGGL(ada_geom_matrix_kernel, dim3((B + DG_BLOCK - 1) / DG_BLOCK), dim3(DG_BLOCK), 0, (hipStream_t)stream, u, u_stride, gu, gu_stride,
                       state, policy_bits, mat, B);
    SGX_LAUNCH_CHECK("ada_geom_matrix");
    return 0;
}

// One launch: the tile path where an identity image can be copied in 16-byte pieces (rows of whole groups of four, 16-byte aligned
// bases), else a pixel per thread.
int dg_plan(bool ptrs_ok, int B, int H, int W, int adjoint, bool aligned, AugPlan* p) {
    if (int rc = aug_check_images("ada_geom", ptrs_ok, B, H, W)) return rc;
    const int tiles_x = (W + DG_TILE - 1) / DG_TILE, tiles_y = (H + DG_TILE - 1) / DG_TILE, adj = adjoint != 0;
    *p = AugPlan{1};
    if (aug_vec4(W, aligned)) p->l[0] = AugLaunch{AUG_K_GEOM_TILE, 0, adj, 0, 0, tiles_x * tiles_y, B, 0, tiles_x};
    else p->l[0] = AugLaunch{AUG_K_GEOM_PX, 0, adj, 0, 0, aug_grid((size_t)H * W), B};
    return 0;
}

extern "C" int sgx_ada_geom(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* stream) {
    AugPlan p;
    if (int rc = dg_plan(x && y && mat, B, H, W, adjoint, aug_aligned(x, y), &p)) return rc;
    if (int rc = aug_check_out_of_place("ada_geom", x, y, " (the passes gather)")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const AugLaunch& l = p.l[0];
    const dim3 grid(l.gx, l.gy), block(DG_BLOCK);
    const bool tile = l.kernel == AUG_K_GEOM_TILE;
    SGX_NOTE(0.0, 24.0 * B * H * W, "ada_geom_%s B%d %dx%d %s", tile ? "tile" : "px", B, H, W, adjoint ? "adj" : "fwd");
    sgx_by_int<0, 1>(l.mode, [&](auto M) {
        if (tile) hipLaunchKernelGGL((ada_geom_tile_kernel<bool(M())>), grid, block, 0, st, x, y, mat, H, W, l.tiles);
        else hipLaunchKernelGGL((ada_geom_px_kernel<bool(M())>), grid, block, 0, st, x, y, mat, H, W);
    });
    SGX_LAUNCH_CHECK("ada_geom");
    return 0;
}
