// Host side shared by the augmentation launchers (diffaug.hip, adageom.hip, adacolor.hip): the argument checks of an image pass, the
// rule for four pixels per lane, the per-image grid, and the plan of what a call launches (sgx_aug_plan, include/sgx.h).
#pragma once
#include "common.h"

// fp32 [B][H][W][3] images, one grid row (blockIdx.y) per image: the code is returned with the message set.  ptrs_ok: the call's
// pointers are all there (the query has none and passes true).
static inline int aug_check_images(const char* name, bool ptrs_ok, int B, int H, int W) {
    SGX_REQUIRE(ptrs_ok && B > 0 && H > 0 && W > 0 && B <= 65535, SGX_EINVAL, "%s: bad arguments (B=%d %dx%d)", name, B, H, W);
    SGX_REQUIRE((size_t)H * W * 3 < (size_t)1 << 31, SGX_EUNSUPPORTED, "%s: image of %dx%d too large", name, H, W);
    return 0;
}
static inline int aug_check_out_of_place(const char* name, const void* x, const void* y, const char* why) {
    SGX_REQUIRE(x != y, SGX_EINVAL, "%s: in place is not supported%s", name, why);
    return 0;
}
static inline int aug_check_ws(const char* name, const void* ws, size_t ws_bytes, size_t need) {
    SGX_REQUIRE(ws && ws_bytes >= need, SGX_EWORKSPACE, "%s: workspace %zu < %zu bytes", name, ws_bytes, need);
    return 0;
}
// The arguments of sgx_ada_geom_matrix / sgx_ada_color_matrix: nu draws and, under ADA, ng gate uniforms per image; the ops of `mask`
// (`ops`: their names and bits, for the message).
static inline int aug_check_matrix(const char* name, const void* u, int u_stride, int nu, const void* gu, int gu_stride, int ng, const void* state,
                                   const void* mat, int B, int policy_bits, int mask, const char* ops) {
    SGX_REQUIRE(u && mat && B > 0, SGX_EINVAL, "%s: bad arguments (B=%d)", name, B);
    SGX_REQUIRE(u_stride >= nu, SGX_EINVAL, "%s: draws %d floats apart, need at least %d", name, u_stride, nu);
    SGX_REQUIRE((gu == nullptr) == (state == nullptr), SGX_EINVAL, "%s: gate uniforms and the ADA state come together or not at all", name);
    SGX_REQUIRE(!gu || gu_stride >= ng, SGX_EINVAL, "%s: gate uniforms %d floats apart, need at least %d", name, gu_stride, ng);
    SGX_REQUIRE(policy_bits >= 0 && (policy_bits & ~mask) == 0, SGX_EINVAL, "%s: policy bits %d (%s)", name, policy_bits, ops);
    return 0;
}

// Four pixels (three 16-byte accesses) per lane: where n (a row's pixels; for the colour pass an image's) splits into whole groups of
// four and both bases are 16-byte aligned.  The query is told the alignment, an entry point reads it off its pointers.
static inline bool aug_aligned(const void* x, const void* y) { return sgx_aligned16(x) && sgx_aligned16(y); }
static inline bool aug_vec4(int n, bool aligned) { return n % 4 == 0 && aligned; }
// One unit per thread, one trip: blocks of 256 per image (grid x; grid y is the batch).
static inline int aug_grid(size_t units) { return (int)((units + 255) / 256); }

// One launch of a plan, in the order of sgx_aug_plan's ints.  P, mode, gated, bias are the kernel's template arguments (0 where it has
// no such argument): mode is MODE of the two sum kernels (0 = DA_PLAIN, 2 = DA_ADJ) and ADJ of every other kernel.  nparts, tiles
// (32 x 32 tiles per row of tiles) and HW are the geometry arguments the kernel receives (0 where it takes none).
enum { AUG_K_SUM = 0, AUG_K_APPLY, AUG_K_BLIT_SUM, AUG_K_BLIT_ROW, AUG_K_BLIT_TILE, AUG_K_GEOM_PX, AUG_K_GEOM_TILE, AUG_K_COLOR_PX, AUG_K_COLOR_VEC };
struct AugLaunch { int kernel, P, mode, gated, bias, gx, gy, nparts, tiles, HW; };
struct AugPlan { int n; AugLaunch l[2]; };
static_assert(SGX_AUG_PLAN_INTS == 1 + 2 * sizeof(AugLaunch) / sizeof(int), "sgx_aug_plan: the count, then two launches");

// What a call of sgx_ada_geom (adageom.hip) / sgx_ada_color (adacolor.hip) launches, or the code the entry refuses the shape with; for
// the entry itself and for sgx_aug_plan (diffaug.hip).  ptrs_ok as in aug_check_images.
int dg_plan(bool ptrs_ok, int B, int H, int W, int adjoint, bool aligned, AugPlan* p);
int dc_plan(bool ptrs_ok, int B, int H, int W, int adjoint, int with_bias, bool aligned, AugPlan* p);
