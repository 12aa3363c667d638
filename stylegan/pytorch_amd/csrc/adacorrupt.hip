// The image-space corruptions of the ADA paper (Karras et al., NeurIPS 2020, App. B) on the discriminator's fp32 RGB input, applied
// last: additive Gaussian noise and ONE cutout rectangle per image (definitions in include/sgx.h):
//   y = M (x + sigma n)    forward (mode 0)       M the diagonal 0/1 mask of the rectangle, n a standard normal field
//   z = M g                linear part (mode 1)   A = A^T = M: also the adjoint, and the R1 double backward
// sgx_ada_corrupt_table turns one D evaluation's draws (and, under ADA, its gate uniforms against p) into the per-image row
// (sigma, k0, k1, x0, x1, y0, y1, 0) once; the passes read the table, never p.  The field is never stored: element e of an image
// takes normal e & 3 of Philox4x32-10 at counter e >> 2 under the image's key (k0, k1), two Box-Muller pairs per call, so the pass is
// one 24 B/pixel stream (one unit per thread, short-lived blocks) and a graph replay gets a fresh field from the
// 24 bytes of draws.  sigma == 0, the empty rectangle and the copy are block-uniform branches: an image or a mode without noise
// executes no Philox round and no transcendental, and both kernels compute a normal by the same function, so they agree bit for bit.
#include "aug.h"

enum { DN_NOISE = 16384, DN_CUTOUT = 32768, DN_OPS = DN_NOISE | DN_CUTOUT };
constexpr int DN_BLOCK = 256, DN_ROW = 8;

// z = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3)
__device__ __forceinline__ float dn_normal(float ua, float ub) {
    const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, ua))));
    const float z = __fmul_rn(r, cosf(__fmul_rn(6.283185307179586f, ub)));
    return fminf(fmaxf(z, -3.f), 3.f);
}

__device__ __forceinline__ float dn_key(float u) { return (float)min((unsigned)__fmul_rn(u, 16777216.f), 16777215u); }

// The cut interval [lo, hi) of an axis of N samples around the centre c: the integers j with |(j + 0.5) / N - c| < 0.25
__device__ __forceinline__ void dn_interval(float c, int N, float& lo, float& hi) {
    const float a = __fmul_rn(c, (float)N), q = __fmul_rn(0.25f, (float)N);
    lo = (float)max(0, (int)floorf(__fsub_rn(__fsub_rn(a, q), 0.5f)) + 1);
    hi = (float)min(N, (int)ceilf(__fsub_rn(__fadd_rn(a, q), 0.5f)));
}

__global__ __launch_bounds__(DN_BLOCK) void ada_corrupt_table_kernel(const float* __restrict__ u, int u_stride, const float* __restrict__ gu,
                                                                     int gu_stride, const float* __restrict__ state, int policy, int H, int W,
                                                                     float* __restrict__ tab, int B) {
    const int b = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (b >= B) return;
    int on = policy;
    if (gu) {
        const float p = state[0];
        const float* g = gu + (size_t)gu_stride * b;
        on &= (g[0] < p ? DN_NOISE : 0) | (g[1] < p ? DN_CUTOUT : 0);
    }
    const float* ub = u + (size_t)u_stride * b;
    float r[DN_ROW] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // both ops off: the all-zero row, what the pass kernels copy under
    if (on & DN_NOISE) {
        r[0] = __fmul_rn(0.1f, fabsf(dn_normal(ub[0], ub[1])));
        r[1] = dn_key(ub[2]);
        r[2] = dn_key(ub[3]);
    }
    if (on & DN_CUTOUT) {
        dn_interval(ub[4], W, r[3], r[4]);
        dn_interval(ub[5], H, r[5], r[6]);
    }
    float* t = tab + DN_ROW * (size_t)b;
#pragma unroll
    for (int k = 0; k < DN_ROW; ++k) t[k] = r[k];
}

// Philox4x32-10 (Salmon et al., SC 2011) at counter (q, 0, 0, 0) under key (k0, k1)
__device__ __forceinline__ void dn_philox(unsigned q, unsigned k0, unsigned k1, unsigned (&o)[4]) {
    unsigned c0 = q, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// The four normals of counter q: two Box-Muller pairs, no clamp.  The one function both kernels take a normal from.
__device__ __forceinline__ void dn_normals(unsigned q, unsigned k0, unsigned k1, float (&n)[4]) {
    unsigned o[4];
    dn_philox(q, k0, k1, o);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float ua = __fmul_rn((float)(o[2 * m] >> 8), 5.9604644775390625e-8f), ub = __fmul_rn((float)(o[2 * m + 1] >> 8), 5.9604644775390625e-8f);
        const float rad = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, ua))));
        float s, c;
        sincospif(__fmul_rn(2.f, ub), &s, &c);
        n[2 * m] = __fmul_rn(rad, c);
        n[2 * m + 1] = __fmul_rn(rad, s);
    }
}

// One image's row as the pass reads it (block-uniform).
struct DnRow { float sigma; unsigned k0, k1; int x0, x1, y0, y1; bool rect; };

__device__ __forceinline__ DnRow dn_load_row(const float* __restrict__ t) {
    DnRow r;
    r.sigma = t[0];
    r.k0 = (unsigned)t[1]; r.k1 = (unsigned)t[2];
    r.x0 = (int)t[3]; r.x1 = (int)t[4]; r.y0 = (int)t[5]; r.y1 = (int)t[6];
    r.rect = r.x0 < r.x1 && r.y0 < r.y1;
    return r;
}

__device__ __forceinline__ bool dn_cut(const DnRow& r, int i, int j) { return i >= r.y0 && i < r.y1 && j >= r.x0 && j < r.x1; }
__device__ __forceinline__ float dn_add(float x, float sigma, float n) { return __fadd_rn(x, __fmul_rn(sigma, n)); }

// Any H, W, any 4-byte aligned base: one pixel per thread, one trip.  Its three elements start at normal (3 unit) & 3 of counter
// (3 unit) >> 2 and may run into the next counter.  grid (ceil(H W / DN_BLOCK), B).
template <int MODE>
__global__ __launch_bounds__(DN_BLOCK) void ada_corrupt_px_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ tab,
                                                                  int HW, int W) {
    const int b = blockIdx.y;
    const DnRow r = dn_load_row(tab + DN_ROW * (size_t)b);
    const int unit = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (unit >= HW) return;
    const size_t at = ((size_t)b * HW + unit) * 3;
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x[at + k];
    const bool noisy = MODE == 0 && r.sigma != 0.f;
    if (noisy || r.rect) {                                       // (block-uniform) else a copy, bit for bit
        const int i = unit / W, j = unit - i * W;
        if (r.rect && dn_cut(r, i, j)) {
            v[0] = v[1] = v[2] = 0.f;
        } else if (noisy) {
            const unsigned e = 3u * (unsigned)unit, q = e >> 2, ph = e & 3u;
            float a[4], c[4] = {0.f, 0.f, 0.f, 0.f};
            dn_normals(q, r.k0, r.k1, a);
            if (ph >= 2u) dn_normals(q + 1u, r.k0, r.k1, c);
            const float n0 = ph == 0u ? a[0] : ph == 1u ? a[1] : ph == 2u ? a[2] : a[3];
            const float n1 = ph == 0u ? a[1] : ph == 1u ? a[2] : ph == 2u ? a[3] : c[0];
            const float n2 = ph == 0u ? a[2] : ph == 1u ? a[3] : ph == 2u ? c[0] : c[1];
            v[0] = dn_add(v[0], r.sigma, n0); v[1] = dn_add(v[1], r.sigma, n1); v[2] = dn_add(v[2], r.sigma, n2);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) y[at + k] = v[k];
}

// Twelve floats as three aligned 16-byte stores.  The empty asm makes each quad one register tuple where the paths of MODE 0 join:
// without it the compiler stored the merged values as 16 + 12 + 16 (at byte 28) + 4 bytes, and the pass ran 7-13 % slower.
__device__ __forceinline__ void dn_store12(float* __restrict__ p, float4 a, float4 b, float4 c) {
    f32x4 o0 = {a.x, a.y, a.z, a.w}, o1 = {b.x, b.y, b.z, b.w}, o2 = {c.x, c.y, c.z, c.w};
    asm volatile("" : "+v"(o0), "+v"(o1), "+v"(o2));
    f32x4* d = reinterpret_cast<f32x4*>(p);
    d[0] = o0; d[1] = o1; d[2] = o2;
}

// H W % 4 == 0, 16-byte aligned bases (an image is 12 H W bytes, so every image base is aligned as well): four consecutive pixels of
// the image's flat pixel order (three 16-byte loads and stores) per thread, one trip; their twelve elements are the normals of the
// counters 3 unit .. 3 unit + 2, three Philox calls.  grid (ceil(H W / (4 DN_BLOCK)), B).
template <int MODE>
__global__ __launch_bounds__(DN_BLOCK) void ada_corrupt_vec_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ tab,
                                                                   int HW, int W) {
    const int b = blockIdx.y;
    const int unit = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (unit >= HW / 4) return;
    const size_t at = ((size_t)b * HW + (size_t)unit * 4) * 3;
    // the data loads first, in ONE region with the table's: the table's wait falls behind them (a region of their own around the
    // loads made the compiler wait for the data before it issued the table's scalar loads in MODE 0: DESIGN 9.7)
    const float4* s = reinterpret_cast<const float4*>(x + at);
    float4 v0 = s[0], v1 = s[1], v2 = s[2];
    const DnRow r = dn_load_row(tab + DN_ROW * (size_t)b);
    const bool noisy = MODE == 0 && r.sigma != 0.f;
    if (noisy || r.rect) {                                       // (block-uniform) else a copy, bit for bit
        bool cut[4] = {false, false, false, false};
        if (r.rect) {
            int i = (4 * unit) / W, j = 4 * unit - i * W;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cut[k] = dn_cut(r, i, j);
                if (++j == W) { j = 0; ++i; }
            }
        }
        if (noisy && !(cut[0] && cut[1] && cut[2] && cut[3])) {
            float n[3][4];
#pragma unroll
            for (int k = 0; k < 3; ++k) dn_normals(3u * (unsigned)unit + k, r.k0, r.k1, n[k]);
            v0.x = dn_add(v0.x, r.sigma, n[0][0]); v0.y = dn_add(v0.y, r.sigma, n[0][1]); v0.z = dn_add(v0.z, r.sigma, n[0][2]);
            v0.w = dn_add(v0.w, r.sigma, n[0][3]); v1.x = dn_add(v1.x, r.sigma, n[1][0]); v1.y = dn_add(v1.y, r.sigma, n[1][1]);
            v1.z = dn_add(v1.z, r.sigma, n[1][2]); v1.w = dn_add(v1.w, r.sigma, n[1][3]); v2.x = dn_add(v2.x, r.sigma, n[2][0]);
            v2.y = dn_add(v2.y, r.sigma, n[2][1]); v2.z = dn_add(v2.z, r.sigma, n[2][2]); v2.w = dn_add(v2.w, r.sigma, n[2][3]);
        }
        if (cut[0]) v0.x = v0.y = v0.z = 0.f;
        if (cut[1]) v0.w = v1.x = v1.y = 0.f;
        if (cut[2]) v1.z = v1.w = v2.x = 0.f;
        if (cut[3]) v2.y = v2.z = v2.w = 0.f;
    }
    dn_store12(y + at, v0, v1, v2);
}

extern "C" int sgx_ada_corrupt_table(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, int H, int W,
                                     float* tab, int B, void* stream) {
    if (int rc = aug_check_matrix("ada_corrupt_table", u, u_stride, 6, gu, gu_stride, 2, state, tab, B, policy_bits, DN_OPS,
                                  "noise 16384, imgcutout 32768"))
        return rc;
    SGX_REQUIRE(H > 0 && W > 0, SGX_EINVAL, "ada_corrupt_table: bad image size %dx%d", H, W);
    SGX_NOTE(0.0, (24.0 + (gu ? 12.0 : 0.0) + 32.0) * B, "ada_corrupt_table B%d", B);
    hipLaunchKernelGGL(ada_corrupt_table_kernel, dim3((B + DN_BLOCK - 1) / DN_BLOCK), dim3(DN_BLOCK), 0, (hipStream_t)stream, u, u_stride, gu,
                       gu_stride, state, policy_bits, H, W, tab, B);
    SGX_LAUNCH_CHECK("ada_corrupt_table");
    return 0;
}

// One launch: four pixels (three 16-byte loads and stores) per lane where an IMAGE splits into whole groups of four (H W % 4 == 0) and
// the bases are aligned, else one.
enum { DN_K_PX = 0, DN_K_VEC = 1 };
struct DnPlan { int n, kernel, mode, gx, gy; };
static_assert(SGX_ADA_CORRUPT_PLAN_INTS == sizeof(DnPlan) / sizeof(int), "sgx_ada_corrupt_plan: the count, then one launch");
static int dn_plan(bool ptrs_ok, int B, int H, int W, int mode, bool aligned, DnPlan* p) {
    if (int rc = aug_check_images("ada_corrupt", ptrs_ok, B, H, W)) return rc;
    SGX_REQUIRE(mode == 0 || mode == 1, SGX_EINVAL, "ada_corrupt: mode %d (0 forward, 1 linear part)", mode);
    const int HW = H * W, vec = aug_vec4(HW, aligned);
    *p = DnPlan{1, vec ? DN_K_VEC : DN_K_PX, mode, aug_grid(vec ? HW / 4 : HW), B};
    return 0;
}

extern "C" int sgx_ada_corrupt_plan(int B, int H, int W, int mode, int aligned, int* out) {
    SGX_REQUIRE(out, SGX_EINVAL, "ada_corrupt_plan: out is NULL");
    for (int i = 0; i < SGX_ADA_CORRUPT_PLAN_INTS; ++i) out[i] = 0;
    DnPlan p;
    if (int rc = dn_plan(true, B, H, W, mode, aligned != 0, &p)) return rc;
    const int v[SGX_ADA_CORRUPT_PLAN_INTS] = {p.n, p.kernel, p.mode, p.gx, p.gy};
    for (int i = 0; i < SGX_ADA_CORRUPT_PLAN_INTS; ++i) out[i] = v[i];
    return 0;
}

extern "C" int sgx_ada_corrupt(const float* x, float* y, const float* tab, int B, int H, int W, int mode, void* stream) {
    DnPlan p;
    if (int rc = dn_plan(x && y && tab, B, H, W, mode, aug_aligned(x, y), &p)) return rc;
    if (int rc = aug_check_out_of_place("ada_corrupt", x, y, "")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.gx, p.gy), block(DN_BLOCK);
    const bool vec = p.kernel == DN_K_VEC;
    SGX_NOTE(0.0, 24.0 * B * H * W, "ada_corrupt_%s B%d %dx%d %s", vec ? "vec" : "px", B, H, W, p.mode ? "lin" : "fwd");
    sgx_by_int<0, 1>(p.mode, [&](auto v) {
        constexpr int MODE = v();
        if (vec) hipLaunchKernelGGL((ada_corrupt_vec_kernel<MODE>), grid, block, 0, st, x, y, tab, H * W, W);
        else hipLaunchKernelGGL((ada_corrupt_px_kernel<MODE>), grid, block, 0, st, x, y, tab, H * W, W);
    });
    SGX_LAUNCH_CHECK("ada_corrupt");
    return 0;
}
