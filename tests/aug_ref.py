"""What a call of an augmentation image pass (sgx_diffaug, sgx_diffaug_gated, sgx_diffaug_blit, sgx_ada_geom, sgx_ada_color) launches:
the rules of csrc/diffaug.hip, adageom.hip and adacolor.hip restated, and the library's own answer (sgx_aug_plan) in the same form.
tests/test_aug_plan.py holds the two together without a GPU; the recording helpers of tests/test_gpu_{diffaug,ada,blit,geom,color}.py
hold every launch they record to the query (assert_recorded_is_planned)."""
import collections
import ctypes

import streaming_ref as SR

DIFFAUG, GATED, BLIT, GEOM, COLOR = range(5)                 # SGX_AUG_PLAN_*
ENTRY_NAME = ("diffaug", "diffaug_gated", "diffaug_blit", "ada_geom", "ada_color")
PLAN_INTS = 21                                               # SGX_AUG_PLAN_INTS: the count, then two launches of ten ints
EINVAL, EUNSUPPORTED = -1, -2                                # SGX_EINVAL, SGX_EUNSUPPORTED
SUM, APPLY, BLIT_SUM, BLIT_ROW, BLIT_TILE, GEOM_PX, GEOM_TILE, COLOR_PX, COLOR_VEC = range(9)
KERNELS = ("diffaug_sum_kernel", "diffaug_apply_kernel", "diffaug_blit_sum_kernel", "diffaug_blit_row_kernel", "diffaug_blit_tile_kernel",
           "ada_geom_px_kernel", "ada_geom_tile_kernel", "ada_color_px_kernel", "ada_color_vec_kernel")
# the five one-dimensional launches, which stay out of the plan
OTHER_KERNELS = ("ada_gates_kernel", "ada_gates_n_kernel", "ada_update_kernel", "ada_geom_matrix_kernel", "ada_color_matrix_kernel")
COLOR_BIT, ROT90_BIT = 1, 16
BLOCK, TILE, PART_PIXELS = 256, 32, 16384

Launch = collections.namedtuple("Launch", "kernel P mode gated bias gx gy nparts tiles HW")


def cdiv(a, b):
    return -(-a // b)


def nparts(H, W):
    return cdiv(H * W, PART_PIXELS)


def plan(entry, B, H, W, bits=0, adjoint=0, with_bias=0, aligned=1):
    """The launches of one valid call, in order."""
    adj = int(bool(adjoint))
    if entry == GEOM:
        if W % 4 == 0 and aligned:
            return [Launch(GEOM_TILE, 0, adj, 0, 0, cdiv(H, TILE) * cdiv(W, TILE), B, 0, cdiv(W, TILE), 0)]
        return [Launch(GEOM_PX, 0, adj, 0, 0, cdiv(H * W, BLOCK), B, 0, 0, 0)]
    if entry == COLOR:                                       # the pass does not know rows: whole groups of four per IMAGE
        vec = (H * W) % 4 == 0 and bool(aligned)
        return [Launch(COLOR_VEC if vec else COLOR_PX, 0, adj, 0, int(bool(with_bias)), cdiv(H * W // 4 if vec else H * W, BLOCK), B, 0, 0, H * W)]
    vec = W % 4 == 0 and bool(aligned)
    P, blit, gated, n = 4 if vec else 1, entry == BLIT, int(entry == GATED), nparts(H, W)
    out = []
    if bits & COLOR_BIT:
        out.append(Launch(BLIT_SUM if blit else SUM, P, 2 * adj, gated, 0, n, B, n, 0, 0))
    if blit and vec and bits & ROT90_BIT:
        t = cdiv(W, TILE)
        out.append(Launch(BLIT_TILE, 0, adj, 0, 0, t * t, B, n, t, 0))
    else:
        out.append(Launch(BLIT_ROW if blit else APPLY, P, adj, gated, 0, cdiv(H * (W // P), BLOCK), B, n, 0, 0))
    return out


def kernel_id(l):
    """The instantiation as the source spells it (streaming_ref.kernel_id of the profiler's name)."""
    tf = lambda v: "true" if v else "false"
    targs = {SUM: f"{l.P}, {l.mode}, {tf(l.gated)}", APPLY: f"{l.P}, {tf(l.mode)}, {tf(l.gated)}", BLIT_SUM: f"{l.P}, {l.mode}",
             BLIT_ROW: f"{l.P}, {tf(l.mode)}", BLIT_TILE: tf(l.mode), GEOM_PX: tf(l.mode), GEOM_TILE: tf(l.mode),
             COLOR_PX: f"{tf(l.mode)}, {tf(l.bias)}", COLOR_VEC: f"{tf(l.mode)}, {tf(l.bias)}"}[l.kernel]
    return f"{KERNELS[l.kernel]}<{targs}>"


def note_name(l):
    """The first word of the launch's SGX_NOTE."""
    return {SUM: "diffaug_sum_gated" if l.gated else "diffaug_sum", APPLY: "diffaug_gated" if l.gated else "diffaug", BLIT_SUM: "diffaug_blit_sum",
            BLIT_ROW: "diffaug_blit_row" if l.P == 4 else "diffaug_blit_px", BLIT_TILE: "diffaug_blit_tile", GEOM_PX: "ada_geom_px",
            GEOM_TILE: "ada_geom_tile", COLOR_PX: "ada_color_px", COLOR_VEC: "ada_color_vec"}[l.kernel]


def query(L, entry, B, H, W, bits=0, adjoint=0, with_bias=0, aligned=1):
    """sgx_aug_plan -> (return code, the PLAN_INTS ints)."""
    out = (ctypes.c_int * PLAN_INTS)(*([7] * PLAN_INTS))
    rc = L.sgx_aug_plan(entry, B, H, W, int(bits), int(adjoint), int(with_bias), int(aligned), ctypes.addressof(out))
    return rc, list(out)


def lib_plan(L, entry, B, H, W, bits=0, adjoint=0, with_bias=0, aligned=1):
    """The library's plan of a valid call, as plan() gives it."""
    rc, q = query(L, entry, B, H, W, bits, adjoint, with_bias, aligned)
    assert rc == 0, (entry, B, H, W, bits, adjoint, with_bias, aligned, rc, L.sgx_last_error())
    assert q[0] in (1, 2) and q[1 + 10 * q[0]:] == [0] * (PLAN_INTS - 1 - 10 * q[0]), q
    return [Launch(*q[1 + 10 * i:11 + 10 * i]) for i in range(q[0])]


def launches_of(launches):
    """-> (kernel ids in launch order, [(grid, block, dynamic LDS)]): the form of the profiler's records."""
    return [kernel_id(l) for l in launches], [((l.gx, l.gy, 1), (BLOCK, 1, 1), 0) for l in launches]


def assert_records_are_planned(N):
    """After a profiled stretch of several calls (a D evaluation, a backward: native.prof_records() still holds it): every recorded
    launch of a plan kernel is a launch sgx_aug_plan reports for the call its note describes -- the entry from the note's name, B, H, W
    and the pass from its text; the policy bits and the alignment, which a note does not carry, are whatever makes it one."""
    L = N.lib()
    for r, (g, b, lds) in zip(N.prof_records(), N.prof_launches()):
        kid = SR.kernel_id(r[0])
        if kid.split("<")[0] not in KERNELS:
            continue
        note, Bs, HW, pass_ = r[4].split(" ")
        entry = next(e for e, n in ((BLIT, "diffaug_blit"), (GATED, "diffaug_sum_gated"), (GATED, "diffaug_gated"), (DIFFAUG, "diffaug"), (GEOM, "ada_geom"),
                                    (COLOR, "ada_color")) if note.startswith(n))
        B, (H, W) = int(Bs[1:]), map(int, HW.split("x"))
        planned = set()
        for bits in range({DIFFAUG: 8, GATED: 8, BLIT: 32}.get(entry, 1)):
            for aligned in (0, 1):
                rc, _ = query(L, entry, B, H, W, bits, pass_ == "adj", pass_ == "fwd", aligned)
                if rc == 0:
                    planned |= {(kernel_id(l), (l.gx, l.gy, 1), note_name(l)) for l in lib_plan(L, entry, B, H, W, bits, pass_ == "adj", pass_ == "fwd", aligned)}
        L.sgx_clear_error()
        assert (kid, tuple(g), note) in planned and tuple(b) == (BLOCK, 1, 1) and int(lds) == 0, (r, g, b, lds, sorted(planned))


def assert_recorded_is_planned(N, entry, x, y, bits=0, adjoint=0, with_bias=0):
    """After one profiled call of ``entry`` on the images x -> y (native.prof_records() still holds it): every recorded launch is what
    sgx_aug_plan reported for that call -- kernel and template arguments, grid, block, LDS, and the note's name."""
    B, H, W, _ = x.shape
    aligned = x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    want = lib_plan(N.lib(), entry, B, H, W, bits, adjoint, with_bias, aligned)
    recs = N.prof_records()
    got = ([SR.kernel_id(r[0]) for r in recs], [(tuple(g), tuple(b), int(lds)) for g, b, lds in N.prof_launches()])
    assert got == launches_of(want), f"{ENTRY_NAME[entry]} B{B} {H}x{W} bits {bits} adjoint {adjoint} bias {with_bias} aligned {aligned}: launched {got}, sgx_aug_plan reported {want}"
    assert [r[4].split(" ")[0] for r in recs] == [note_name(l) for l in want], (recs, want)
