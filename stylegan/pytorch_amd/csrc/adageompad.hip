// The bilinear resample of the geometric group (adageom.hip) with the ADA paper's REFLECTION padding instead of zeros (definitions in
// include/sgx.h, sgx_ada_geom_reflect).  Per axis of length N >= 2 a tap index t is valid iff -(N-1) <= t <= 2 (N-1) -- one
// reflection period, np.pad(mode="reflect") with pad N-1 -- and reads the pixel r(t) = -t (t < 0), 2 (N-1) - t (t > N-1), t (else);
// the weight is taken at the unreflected t; a tap beyond one period contributes zero (the paper clamps its margin the same way):
//   y(p) = sum over the valid taps t = floor(s_p) + {0,1}^2 of w(s_p, t) x(r(t))                    forward
//   z(q) = sum_p sum over the valid taps t of p with r(t) = q of w(s_p, t) g(p)                       adjoint
// Both are gathers (no atomics: bit-reproducible) over the table of sgx_ada_geom_matrix, with the position, the weight, the
// accumulation step and the candidate walk of adageom.h, so the adjoint's coefficients are the forward's bit for bit, and where no
// tap leaves the image both directions give sgx_ada_geom's bits.  The adjoint enumerates the unreflected positions q' with r(q') = q:
// per axis q itself, -q when q >= 1 and 2 (N-1) - q when q <= N-2 (up to three, distinct, all inside the period), so up to nine
// per pixel, mirrors row-major (the row's three, then the column's three, in that order), and runs the candidate walk for each; most
// leave through the walk's box-outside test at once.  An identity row is copied (a block-uniform branch).
#include "adageom.h"

__device__ __forceinline__ bool dgp_valid(int t, int N) { return t >= -(N - 1) && t <= 2 * (N - 1); }
__device__ __forceinline__ int dgp_reflect(int t, int N) { return t < 0 ? -t : t > N - 1 ? 2 * (N - 1) - t : t; }

// Forward value of output pixel (i, j): taps in the order (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1), those beyond one period
// skipped.  The early return is wider than "no valid tap" by a pixel (and takes the NaN positions of a bad table); inside it
// |s| < 2 max(H, W) + 1 < 2^31, and the per-tap tests are exact.
__device__ __forceinline__ void dgp_fwd_px(const float* __restrict__ xb, int H, int W, const DgMat& q, float cx, float cy, int i, int j,
                                           float (&acc)[3]) {
    float sx, sy;
    geom_pos(q, cx, cy, i, j, sx, sy);
    acc[0] = acc[1] = acc[2] = 0.f;
    if (!(sx > -(float)W - 1.f && sx < 2.f * (float)W && sy > -(float)H - 1.f && sy < 2.f * (float)H)) return;
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int tx = x0 + dx, ty = y0 + dy;
            if (dgp_valid(tx, W) && dgp_valid(ty, H))
                dg_acc(acc, geom_w(sx, sy, tx, ty), xb + ((size_t)dgp_reflect(ty, H) * W + dgp_reflect(tx, W)) * 3);
        }
    }
}

// Mirror m = 0, 1, 2 of the pixel index q on an axis of length N: the position, and whether the axis has it.
__device__ __forceinline__ int dgp_mirror(int m, int q, int N) { return m == 0 ? q : m == 1 ? -q : 2 * (N - 1) - q; }
__device__ __forceinline__ bool dgp_has_mirror(int m, int q, int N) { return m == 0 || (m == 1 ? q >= 1 : q <= N - 2); }

// Adjoint value of pixel q = (row qi, column qj): the candidate walk at each of its up to nine unreflected positions, into one sum.
__device__ __forceinline__ void dgp_adj_px(const float* __restrict__ gb, int H, int W, const DgMat& q, float cx, float cy, const DgBox& bx,
                                           int qi, int qj, float (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.f;
    for (int my = 0; my < 3; ++my) {
        if (!dgp_has_mirror(my, qi, H)) continue;
        const int ti = dgp_mirror(my, qi, H);
        for (int mx = 0; mx < 3; ++mx) {
            if (!dgp_has_mirror(mx, qj, W)) continue;
            dg_adj_walk(gb, H, W, q, cx, cy, bx.ex, bx.ey, bx.nx, bx.ny, ti, dgp_mirror(mx, qj, W), acc);
        }
    }
}

// Any H, W >= 2, any 4-byte aligned base: one pixel per thread in row order, one trip.  grid (ceil(H W / DG_BLOCK), B).
template <bool ADJ>
__global__ __launch_bounds__(DG_BLOCK) void ada_geom_reflect_px_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                       const float* __restrict__ mat, int H, int W) {
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
        if (ADJ) dgp_adj_px(xb, H, W, q, cx, cy, bx, i, j, acc);
        else dgp_fwd_px(xb, H, W, q, cx, cy, i, j, acc);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) y[at + k] = acc[k];
}

// W % 4 == 0, 16-byte aligned bases: the lane layout of ada_geom_tile_kernel (adageom.hip) -- a block owns a
// DG_TILE x DG_TILE output tile, a wave eight rows of it, and in each of its four trips the wave's lanes are an 8 x 8 patch, which
// an affine map (and its reflection, piecewise) takes to a few cache lines of the source.  An identity image is copied in row order,
// four pixels (three 16-byte loads and stores) per thread.  grid (ceil(H / DG_TILE) * ceil(W / DG_TILE), B).
template <bool ADJ>
__global__ __launch_bounds__(DG_BLOCK) void ada_geom_reflect_tile_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                         const float* __restrict__ mat, int H, int W, int tiles_x) {
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
        if (ADJ) dgp_adj_px(xb, H, W, q, cx, cy, bx, i, j, acc);
        else dgp_fwd_px(xb, H, W, q, cx, cy, i, j, acc);
        f32x3u v; v.x = acc[0]; v.y = acc[1]; v.z = acc[2];
        *reinterpret_cast<f32x3u*>(yb + ((size_t)i * W + j) * 3) = v;
    }
}

// One launch, chosen as sgx_ada_geom chooses its own: the tile kernel where an identity image can be copied in 16-byte pieces (rows of
// whole groups of four, 16-byte aligned bases), else a pixel per thread.
enum { DGP_K_PX = 0, DGP_K_TILE = 1 };
struct DgpPlan { int n, kernel, adj, gx, gy, tiles; };
static_assert(SGX_ADA_GEOM_REFLECT_PLAN_INTS == sizeof(DgpPlan) / sizeof(int), "sgx_ada_geom_reflect_plan: the count, then one launch");
static int dgp_plan(bool ptrs_ok, int B, int H, int W, int adjoint, bool aligned, DgpPlan* p) {
    if (int rc = aug_check_images("ada_geom_reflect", ptrs_ok, B, H, W)) return rc;
    SGX_REQUIRE(H >= 2 && W >= 2, SGX_EINVAL, "ada_geom_reflect: the reflection needs H, W >= 2, got %dx%d", H, W);
    const int tiles_x = (W + DG_TILE - 1) / DG_TILE, tiles_y = (H + DG_TILE - 1) / DG_TILE, adj = adjoint != 0;
    if (aug_vec4(W, aligned)) *p = DgpPlan{1, DGP_K_TILE, adj, tiles_x * tiles_y, B, tiles_x};
    else *p = DgpPlan{1, DGP_K_PX, adj, aug_grid((size_t)H * W), B, 0};
    return 0;
}

extern "C" int sgx_ada_geom_reflect_plan(int B, int H, int W, int adjoint, int aligned, int* out) {
    SGX_REQUIRE(out, SGX_EINVAL, "ada_geom_reflect_plan: out is NULL");
    for (int i = 0; i < SGX_ADA_GEOM_REFLECT_PLAN_INTS; ++i) out[i] = 0;
    DgpPlan p;
    if (int rc = dgp_plan(true, B, H, W, adjoint, aligned != 0, &p)) return rc;
    const int v[SGX_ADA_GEOM_REFLECT_PLAN_INTS] = {p.n, p.kernel, p.adj, p.gx, p.gy, p.tiles};
    for (int i = 0; i < SGX_ADA_GEOM_REFLECT_PLAN_INTS; ++i) out[i] = v[i];
    return 0;
}

extern "C" int sgx_ada_geom_reflect(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* stream) {
    DgpPlan p;
    if (int rc = dgp_plan(x && y && mat, B, H, W, adjoint, aug_aligned(x, y), &p)) return rc;
    if (int rc = aug_check_out_of_place("ada_geom_reflect", x, y, " (the passes gather)")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.gx, p.gy), block(DG_BLOCK);
    const bool tile = p.kernel == DGP_K_TILE;
    SGX_NOTE(0.0, 24.0 * B * H * W, "ada_geom_reflect_%s B%d %dx%d %s", tile ? "tile" : "px", B, H, W, p.adj ? "adj" : "fwd");
    sgx_by_int<0, 1>(p.adj, [&](auto M) {
        if (tile) hipLaunchKernelGGL((ada_geom_reflect_tile_kernel<bool(M())>), grid, block, 0, st, x, y, mat, H, W, p.tiles);
        else hipLaunchKernelGGL((ada_geom_reflect_px_kernel<bool(M())>), grid, block, 0, st, x, y, mat, H, W);
    });
    SGX_LAUNCH_CHECK("ada_geom_reflect");
    return 0;
}
