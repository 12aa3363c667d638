// The colour group of the ADA paper (Karras et al., NeurIPS 2020) on the discriminator's fp32 RGB input: brightness, contrast, luma flip,
// hue rotation and saturation of one image composed into ONE affine map of the RGB vector (definitions in include/sgx.h):
//   y = M x + t        forward (with_bias) / linear part (without)
//   z = M^T g          adjoint
// with v = (1,1,1)/sqrt(3), P = v v^T, K the cross-product matrix of v:  M = c [sigma P + s (cos(theta) (I - P) + sin(theta) K)],
// t = c sigma b (1,1,1).  sgx_ada_color_matrix turns one D evaluation's draws (and, under ADA, its gate uniforms against p) into the
// per-image table {M row major, t} once; the forward, the linear part, the adjoint and the R1 double backward read the table, never p.
// The pass is one 24 B/pixel stream (one unit per thread, short-lived blocks); every product and sum is rounded to
// fp32 on its own in the header's order, so a float32 restatement reproduces it bit for bit and the adjoint's coefficients ARE the
// forward's.  A row equal to (I, 0) is the identity flag: both kernels copy such an image (a block-uniform branch), bit for bit.
#include "aug.h"

enum { DC_BRIGHTNESS = 256, DC_CONTRAST = 512, DC_LUMAFLIP = 1024, DC_HUE = 2048, DC_SATURATION = 4096,
       DC_OPS = DC_BRIGHTNESS | DC_CONTRAST | DC_LUMAFLIP | DC_HUE | DC_SATURATION };
constexpr int DC_BLOCK = 256;

// z = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3)
__device__ __forceinline__ float dc_normal(float ua, float ub) {
    const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, ua))));
    const float z = __fmul_rn(r, cosf(__fmul_rn(6.283185307179586f, ub)));
    return fminf(fmaxf(z, -3.f), 3.f);
}

__global__ __launch_bounds__(DC_BLOCK) void ada_color_matrix_kernel(const float* __restrict__ u, int u_stride, const float* __restrict__ gu,
                                                                    int gu_stride, const float* __restrict__ state, int policy,
                                                                    float* __restrict__ mat, int B) {
    const int b = blockIdx.x * DC_BLOCK + threadIdx.x;
    if (b >= B) return;
    int on = policy;
    if (gu) {
        const float p = state[0];
        const float* g = gu + (size_t)gu_stride * b;
        on &= (g[0] < p ? DC_BRIGHTNESS : 0) | (g[1] < p ? DC_CONTRAST : 0) | (g[2] < p ? DC_LUMAFLIP : 0) | (g[3] < p ? DC_HUE : 0) |
              (g[4] < p ? DC_SATURATION : 0);
    }
    float* m = mat + 12 * (size_t)b;
    float dg = 1.f, lo = 0.f, up = 0.f, t = 0.f;                 // M = circulant(dg, lo, up): rows (dg lo up), (up dg lo), (lo up dg)
    if (on & DC_OPS) {                                           // (else: the identity row, what the pass kernels copy under)
        const float* ub = u + (size_t)u_stride * b;
        const float c = (on & DC_CONTRAST) ? exp2f(__fmul_rn(0.5f, dc_normal(ub[2], ub[3]))) : 1.f;
        const bool flip = (on & DC_LUMAFLIP) && fminf(floorf(__fmul_rn(2.f, ub[4])), 1.f) == 1.f;
        const float cf = flip ? -c : c;                                                               // c sigma
        if (on & DC_BRIGHTNESS) t = __fmul_rn(cf, __fmul_rn(0.2f, dc_normal(ub[0], ub[1])));
        if (!flip && !(on & (DC_HUE | DC_SATURATION))) {         // c I exactly (1/3 + 2/3 in fp32 is not to be trusted for this)
            dg = c;
        } else {
            const float cs = (on & DC_SATURATION) ? __fmul_rn(c, exp2f(dc_normal(ub[6], ub[7]))) : c;
            float co = 1.f, sn = 0.f;
            if (on & DC_HUE) {
                const float th = __fmul_rn(6.283185307179586f, __fsub_rn(ub[5], 0.5f));
                co = cosf(th); sn = sinf(th);
            }
            const float a = __fdiv_rn(cf, 3.f), d3 = __fdiv_rn(__fmul_rn(cs, co), 3.f);
            const float e = __fmul_rn(__fmul_rn(cs, sn), 0.5773502691896258f);
            const float base = __fsub_rn(a, d3);
            dg = __fadd_rn(a, __fmul_rn(2.f, d3)); lo = __fsub_rn(base, e); up = __fadd_rn(base, e);
        }
    }
    m[0] = dg; m[1] = lo; m[2] = up; m[3] = up; m[4] = dg; m[5] = lo; m[6] = lo; m[7] = up; m[8] = dg;
    m[9] = t; m[10] = t; m[11] = t;
}

// One image's map as the pass applies it: out_k = ((c[k][0] in_0 + c[k][1] in_1) + c[k][2] in_2) (+ t[k]); the adjoint reads M transposed.
struct DcMap { float c[3][3], t[3]; bool identity; };

template <bool ADJ>
__device__ __forceinline__ DcMap dc_load_map(const float* __restrict__ m) {
    DcMap q;
    bool id = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = m[3 * k + j];
            id = id && v == (k == j ? 1.f : 0.f);
            if (ADJ) q.c[j][k] = v; else q.c[k][j] = v;
        }
        q.t[k] = m[9 + k];
        id = id && q.t[k] == 0.f;
    }
    q.identity = id;
    return q;
}

template <bool BIAS>
__device__ __forceinline__ void dc_pixel(const DcMap& q, float& r, float& g, float& b) {
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = __fadd_rn(__fadd_rn(__fmul_rn(q.c[k][0], r), __fmul_rn(q.c[k][1], g)), __fmul_rn(q.c[k][2], b));
        if (BIAS) o[k] = __fadd_rn(o[k], q.t[k]);
    }
    r = o[0]; g = o[1]; b = o[2];
}

// Any H, W, any 4-byte aligned base: one pixel per thread, one trip.  grid (ceil(H W / DC_BLOCK), B).
template <bool ADJ, bool BIAS>
__global__ __launch_bounds__(DC_BLOCK) void ada_color_px_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                                int HW) {
    const int b = blockIdx.y;
    const DcMap q = dc_load_map<ADJ>(mat + 12 * (size_t)b);
    const int unit = blockIdx.x * DC_BLOCK + threadIdx.x;
    if (unit >= HW) return;
    const size_t at = ((size_t)b * HW + unit) * 3;
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x[at + k];
    if (!q.identity) dc_pixel<BIAS>(q, v[0], v[1], v[2]);        // (block-uniform) else a copy, bit for bit
#pragma unroll
    for (int k = 0; k < 3; ++k) y[at + k] = v[k];
}

// H W % 4 == 0, 16-byte aligned bases (an image is 12 H W bytes, so every image base is aligned as well): four consecutive pixels (three
// 16-byte loads and stores) per thread, one trip, the layout of the apply kernel of diffaug.hip.  grid (ceil(H W / (4 DC_BLOCK)), B).
template <bool ADJ, bool BIAS>
__global__ __launch_bounds__(DC_BLOCK) void ada_color_vec_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                                 int HW) {
    const int b = blockIdx.y;
    const int unit = blockIdx.x * DC_BLOCK + threadIdx.x;
    const bool live = unit < HW / 4;
    const size_t at = ((size_t)b * HW + (size_t)unit * 4) * 3;
    float4 v0, v1, v2;
    if (live) {                                                  // the data loads first: the table's wait falls behind them
        const float4* s = reinterpret_cast<const float4*>(x + at);
        v0 = s[0]; v1 = s[1]; v2 = s[2];
    }
    const DcMap q = dc_load_map<ADJ>(mat + 12 * (size_t)b);
    if (!live) return;
    if (!q.identity) {                                           // (block-uniform) else a copy, bit for bit
        dc_pixel<BIAS>(q, v0.x, v0.y, v0.z);
        dc_pixel<BIAS>(q, v0.w, v1.x, v1.y);
        dc_pixel<BIAS>(q, v1.z, v1.w, v2.x);
        dc_pixel<BIAS>(q, v2.y, v2.z, v2.w);
    }
    float4* d = reinterpret_cast<float4*>(y + at);
    d[0] = v0; d[1] = v1; d[2] = v2;
}

extern "C" int sgx_ada_color_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat,
                                    int B, void* stream) {
    if (int rc = aug_check_matrix("ada_color_matrix", u, u_stride, 8, gu, gu_stride, 5, state, mat, B, policy_bits, DC_OPS,
                                  "brightness 256, contrast 512, lumaflip 1024, hue 2048, saturation 4096"))
        return rc;
    SGX_NOTE(0.0, (32.0 + (gu ? 24.0 : 0.0) + 48.0) * B, "ada_color_matrix B%d", B);
    hipLaunchKernelGGL(ada_color_matrix_kernel, dim3((B + DC_BLOCK - 1) / DC_BLOCK), dim3(DC_BLOCK), 0, (hipStream_t)stream, u, u_stride, gu,
                       gu_stride, state, policy_bits, mat, B);
    SGX_LAUNCH_CHECK("ada_color_matrix");
    return 0;
}

// One launch: four pixels (three 16-byte loads and stores) per lane where an IMAGE splits into whole groups of four (H W % 4 == 0: the
// pass does not know rows) and the bases are aligned, else one.
int dc_plan(bool ptrs_ok, int B, int H, int W, int adjoint, int with_bias, bool aligned, AugPlan* p) {
    if (int rc = aug_check_images("ada_color", ptrs_ok, B, H, W)) return rc;
    SGX_REQUIRE(!(adjoint && with_bias), SGX_EINVAL, "ada_color: the adjoint has no bias");
    const int HW = H * W, vec = aug_vec4(HW, aligned);
    *p = AugPlan{1, {{vec ? AUG_K_COLOR_VEC : AUG_K_COLOR_PX, 0, adjoint != 0, 0, with_bias != 0, aug_grid(vec ? HW / 4 : HW), B, 0, 0, HW}}};
    return 0;
}

extern "C" int sgx_ada_color(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, int with_bias, void* stream) {
    AugPlan p;
    if (int rc = dc_plan(x && y && mat, B, H, W, adjoint, with_bias, aug_aligned(x, y), &p)) return rc;
    if (int rc = aug_check_out_of_place("ada_color", x, y, "")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const AugLaunch& l = p.l[0];
    const dim3 grid(l.gx, l.gy), block(DC_BLOCK);
    const bool vec = l.kernel == AUG_K_COLOR_VEC;
    SGX_NOTE(0.0, 24.0 * B * H * W, "ada_color_%s B%d %dx%d %s", vec ? "vec" : "px", B, H, W, adjoint ? "adj" : with_bias ? "fwd" : "lin");
    sgx_by_int<0, 1, 2>(2 * l.mode + l.bias, [&](auto v) {             // linear part, forward, adjoint: <ADJ, BIAS> = <0, 0>, <0, 1>, <1, 0>
        constexpr bool ADJ = v() == 2, BIAS = v() == 1;
        if (vec) hipLaunchKernelGGL((ada_color_vec_kernel<ADJ, BIAS>), grid, block, 0, st, x, y, mat, l.HW);
        else hipLaunchKernelGGL((ada_color_px_kernel<ADJ, BIAS>), grid, block, 0, st, x, y, mat, l.HW);
    });
    SGX_LAUNCH_CHECK("ada_color");
    return 0;
}
