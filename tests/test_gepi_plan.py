"""CPU: what a generator-epilogue call will launch, asked of the library itself.  sgx_gepi_plan answers from the plan functions the launchers of
csrc/gepi.hip execute (gepi_fwd_plan, gepi_bwd_plan, gepi_stats_plan), so on a grid of shapes: (a) the kernel list in launch order, the geometry
and gepi_bwd2s' route are what tests/epilogue_ref.py restates; (b) sgx_gepi_ws_bytes and sgx_blur3x3_stats_nparts return what the commit before
the launchers were folded into plans returned (tests/golden/gepi_ws.json, written by tests/golden/make_golden_gepi_ws.py); (c) under each
environment of epilogue_ref.GROUPS and under two plan-only environments -- the off arms SGX_GEPI_SMALL=0 SGX_GEPI_APPLY1=0 SGX_GEPI_BWD2S=0, and
SGX_GEPI_RPT=16 -- in a child process each (the switches are read once per process), the plan is the restated one; (d) SGX_GEPI_RPT=0 and -3
plan as the default; (e) the shapes of epilogue_ref.REJECTIONS get their codes from the query.  The queries are host-only: no process here
opens the GPU.  The grid has cases on both sides of every seam of the restatement: 192 MB (B 5 / 6 at 2^20 x 16 bf16), 800 MB (B 23 / 24), the
one-launch caps (HW 256 / 257 and 1024 / 1025, B C / 16 = 63 / 64, 8 MiB at B 8 / 9 with 1024 x 512 bf16)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gepi_ws.json")
F32, BF16 = 0, 1
FWD, BWD, STATS = 0, 1, 2
PLAN_INTS = 15

BATCHES = (1, 2, 4, 5, 6, 8, 9, 23, 24, 32, 63, 64)
PIXELS = (1, 16, 64, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096, 1 << 14, 1 << 16, 1 << 18, 1 << 20)
CHANNELS = (4, 8, 16, 32, 64, 128, 256, 512, 2048)                        # C = 4: fp32 only (no bf16 vector)
REDUCED = dict(batches=(2, 6, 24, 64), pixels=(16, 257, 4096, 1 << 20), channels=(4, 16, 64, 256, 2048), flags=(0, 3))   # the grid of the child processes
# Environments planned here only (the GPU rows of epilogue_ref.GROUPS stay three child processes): the off arms, and a rows-per-thread cap
PLAN_GROUPS = {
    "off": {"SGX_GEPI_SMALL": "0", "SGX_GEPI_APPLY1": "0", "SGX_GEPI_BWD2S": "0"},
    "rpt16": {"SGX_GEPI_RPT": "16"},
}
UNSET = {"rpt0": {"SGX_GEPI_RPT": "0"}, "rpt-3": {"SGX_GEPI_RPT": "-3"}}
ENV_KEYS = {"SGX_GEPI_APPLY1": "apply1", "SGX_GEPI_BWD2S": "bwd2s", "SGX_GEPI_FOLD": "fold", "SGX_NT_MIN_MB": "nt_mb", "SGX_GEPI_SMALL": "small", "SGX_GEPI_RPT": "rpt"}


def shapes(batches=BATCHES, pixels=PIXELS, channels=CHANNELS, **_):
    """(B, HW, C, dtype)"""
    for B in batches:
        for HW in pixels:
            for C in channels:
                for dt in (F32, BF16):
                    if C % (4 if dt == F32 else 8) == 0:
                        yield B, HW, C, dt


def queries(flags=(0, 1, 2, 3), **grid):
    """(entry, B, HW, C, flags, pre, dtype): the forward and the statistics under every flag, with and without producer partials; the backward
    once (its plan takes neither)."""
    for B, HW, C, dt in shapes(**grid):
        for fl in flags:
            for pre in (0, 1):
                yield FWD, B, HW, C, fl, pre, dt
                yield STATS, B, HW, C, fl, pre, dt
        yield BWD, B, HW, C, 3, 0, dt


def lib_plan(L, q):
    """-> (rc, the ints of sgx_gepi_plan as a list)."""
    out = (ctypes.c_int * PLAN_INTS)()
    rc = L.sgx_gepi_plan(*q, ctypes.addressof(out))
    if rc:
        L.sgx_clear_error()
    return rc, list(out)


def lib_plans(L, **grid):
    return [lib_plan(L, q) for q in queries(**grid)]


def hw_split(HW):
    """H x W = HW with H the largest divisor <= sqrt(HW): the blur's shape of a grid point."""
    h = max(d for d in range(1, int(HW ** 0.5) + 1) if HW % d == 0)
    return h, HW // h


def host_sizes(L):
    """What the two host functions of the fixture return over the full grid."""
    ws = [L.sgx_gepi_ws_bytes(B, HW, C) for B in BATCHES for HW in PIXELS for C in CHANNELS]
    nparts = [L.sgx_blur3x3_stats_nparts(B, *hw_split(HW), C, dt) for B, HW, C, dt in shapes()]
    return ws, nparts


def env_of(variables):
    """The restatement's environment of a set of switches."""
    import epilogue_ref as ER
    return dict(ER.ENV_DEFAULT, **{ENV_KEYS[k]: (float(v) if k == "SGX_NT_MIN_MB" else int(v)) for k, v in variables.items()})


def decode(q, v):
    """The library's ints as epilogue_ref spells them: (kernels in launch order, geometry, (blocks per image, pre-reduction rows), gepi_fin_bwd2's (B, n))."""
    import epilogue_ref as ER
    entry, B, HW, C, flags, pre, dt = q
    t = "float" if dt == F32 else "bf16_t"
    small, reduce_pass, from_pre, fin, apply, nt = v[:6]
    assert small in (0, 1, 2) and fin in (0, 1, 2, 3) and apply in (0, 1, 2) and nt in (0, 1), (q, v)
    assert (apply == 2) == (fin == 2), (q, v)                              # the short-lived apply kernels read the table, nobody else does
    kind = "bwd" if entry == BWD else "fwd"
    if small:
        k = [f"gepi_small_{kind}<{t}, 256, 2>" if small == 1 else f"gepi_small_{kind}<{t}, 512, 4>"]
        assert (reduce_pass, from_pre, fin, apply) == (0, 0, 0, 0) and entry != STATS, (q, v)
    else:
        k = [f"gepi_pass<{t}, {1 if entry == BWD else 0}, false>"] if reduce_pass else []
        if fin in (1, 2):
            k.append("gepi_fin_bwd1" if entry == BWD else "gepi_fin_stats")
        if entry == BWD:
            k.append(f"gepi_pass<{t}, 2, {'true' if nt else 'false'}>" if apply == 1 else f"gepi_bwd2s<{t}>")
            if v[12]:
                k.append("gepi_rows_prereduce")
        elif entry == FWD:
            k.append(f"gepi_apply<{t}>" if apply == 1 else f"gepi_apply1<{t}>")
        else:
            assert apply == 0 and fin == 1, (q, v)
    if entry == BWD:
        k.append("gepi_fin_bwd2")
    return tuple(k), ER.Geom(*v[6:11]), (v[11], v[12]), (v[13], v[14])


def restated(q, env):
    import epilogue_ref as ER
    entry, B, HW, C, flags, pre, dt = q
    tdt = ER.F if dt == F32 else ER.H
    geom = ER.gepi_geom(B, HW, C, 4 if dt == F32 else 8, env["rpt"])
    if entry == FWD:
        return tuple(ER.fwd_kernels(B, HW, C, tdt, flags, pre, env)), geom, (0, 0), (0, 0)
    if entry == STATS:
        return tuple(ER.stats_kernels(B, HW, C, tdt, flags, pre)), geom, (0, 0), (0, 0)
    k = tuple(ER.bwd_kernels(B, HW, C, tdt, env))
    if k[0].startswith("gepi_small"):
        return k, geom, (0, 0), (B, 1)
    if any(x.startswith("gepi_bwd2s") for x in k):
        nblk, rows = ER.bwd2s_route(B, HW, C, tdt, env["rpt"])
        return k, geom, (nblk, rows), ((1, rows) if rows else (B, nblk))
    return k, geom, (0, 0), (B, geom.nchunk)


def differences(got, env, **grid):
    wrong, n = [], 0
    for q, (rc, v) in zip(queries(**grid), got):
        n += 1
        g, w = (rc,) + (decode(q, v) if rc == 0 else ()), (0,) + restated(q, env)
        if g != w:
            wrong.append("%s: library %s, restated %s" % (q, g, w))
    assert n == len(got)
    return wrong


def paths(got, **grid):
    """The kernel lists a grid reaches, each with the entry point that launches it."""
    return {(q[0], decode(q, v)[0]) for q, (rc, v) in zip(queries(**grid), got) if rc == 0}


def row_paths(group):
    """... and the ones the rows of epilogue_ref.CASES name (a producer's own kernel in front of the epilogue's left out)."""
    import epilogue_ref as ER
    entry = {"sgx_gepi_fwd": FWD, "sgx_blur3x3_stats": FWD, "sgx_conv3x3_stats": FWD, "sgx_gepi_bwd": BWD, "sgx_gepi_stats": STATS}
    return {(entry[c.entry], tuple(k for k in c.kernels if not k.startswith("blur_stats_kernel"))) for c in ER.CASES if c.group == group}


@pytest.fixture(scope="module")
def L():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def children(L):
    """group -> the child's plans on the reduced grid.  All started at once, after the fixture ``L`` has built the library: each only loads it
    and answers host-side queries."""
    import epilogue_ref as ER
    envs = dict({g: e for g, e in ER.GROUPS.items() if g != "default"}, **PLAN_GROUPS, **UNSET)
    base = {k: v for k, v in os.environ.items() if not k.startswith("SGX_GEPI") and k != "SGX_NT_MIN_MB"}
    procs = {g: subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=dict(base, **e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for g, e in envs.items()}
    out = {}
    for g, p in procs.items():
        so, se = p.communicate()
        assert p.returncode == 0, (g, se[-2000:])
        out[g] = [(rc, v) for rc, v in json.loads(so.splitlines()[-1])]
    return out


def test_the_grid_is_the_one_described():
    assert len(list(shapes())) == 12 * 16 * (9 + 8) and len(list(queries())) == 12 * 16 * 17 * 17
    assert len(list(shapes(**REDUCED))) == 4 * 4 * (5 + 4) and len(list(queries(**REDUCED))) == 4 * 4 * 9 * 9
    assert 2 * 6 * (1 << 20) * 16 >= 192e6 > 2 * 5 * (1 << 20) * 16 and 2 * 24 * (1 << 20) * 16 >= 800e6 > 2 * 23 * (1 << 20) * 16
    assert 8 * 1024 * 512 * 2 == 8 << 20 and 64 * 16 // 16 == 64 > 63 * 16 // 16


def test_the_plan_is_the_restated_one(L):
    import epilogue_ref as ER
    got = lib_plans(L)
    wrong = differences(got, ER.ENV_DEFAULT)                                                      # (a)
    assert not wrong, "%d of %d plans differ:\n%s" % (len(wrong), len(got), "\n".join(wrong[:40]))
    missing = row_paths("default") - paths(got)
    assert not missing, "kernel lists of epilogue_ref.CASES that the grid never plans: %s" % sorted(missing)


def test_the_host_functions_return_what_was_recorded(L):
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["axes"] == {"B": list(BATCHES), "HW": list(PIXELS), "C": list(CHANNELS)}
    ws, nparts = host_sizes(L)                                                                    # (b)
    assert len(fx["ws_bytes"]) == len(ws) == 12 * 16 * 9 and len(fx["blur_nparts"]) == len(nparts) == 12 * 16 * 17
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(ws, fx["ws_bytes"])) if g != w]
    assert not wrong, "%d workspace sizes differ (index, returned, recorded): %s" % (len(wrong), wrong[:20])
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(nparts, fx["blur_nparts"])) if g != w]
    assert not wrong, "%d partial counts differ (index, returned, recorded): %s" % (len(wrong), wrong[:20])


def test_every_switch_group_plans_as_restated(L, children):
    import epilogue_ref as ER
    assert set(children) == set(ER.GROUPS) - {"default"} | set(PLAN_GROUPS) | set(UNSET) and len(children) == 7
    default = lib_plans(L, **REDUCED)
    for g, variables in dict(ER.GROUPS, **PLAN_GROUPS).items():                                   # (c)
        if g == "default":
            continue
        env = env_of(variables)
        assert g in PLAN_GROUPS or env == ER.group_env(g), g
        wrong = differences(children[g], env, **REDUCED)
        assert not wrong, "group %s: %d plans differ:\n%s" % (g, len(wrong), "\n".join(wrong[:40]))
        assert children[g] != default, g                                                          # the group's switches move some plan of the reduced grid
        missing = row_paths(g) - paths(children[g], **REDUCED)
        assert not missing, "group %s: kernel lists of epilogue_ref.CASES that the reduced grid never plans: %s" % (g, sorted(missing))
    # the off arms: no one-launch kernel and neither short-lived apply kernel anywhere, though the grid reaches all three by default
    off, dflt = paths(children["off"], **REDUCED), paths(default, **REDUCED)
    for name in ("gepi_small", "gepi_apply1", "gepi_bwd2s"):
        assert any(k.startswith(name) for _, ks in dflt for k in ks) and not any(k.startswith(name) for _, ks in off for k in ks), name
    assert max(v[8] for _, v in children["rpt16"]) == 16 and max(v[8] for _, v in default) == 64


def test_values_that_mean_unset_plan_as_the_default(L, children):
    default = lib_plans(L, **REDUCED)
    assert children["rpt0"] == default and children["rpt-3"] == default                           # (d)


def test_the_query_refuses_what_the_entry_points_refuse(L):
    import epilogue_ref as ER
    for id_, B, HW, C, dt, short, code, why in ER.REJECTIONS:                                     # (e)
        # (the query takes the workspace as sufficient: it has no argument for it, so the row that is one byte short plans)
        want = code if not short else 0
        for entry in (FWD, BWD, STATS):
            assert lib_plan(L, (entry, B, HW, C, 3, 0, F32 if dt == ER.F else BF16))[0] == want, (id_, entry)
    out = (ctypes.c_int * PLAN_INTS)()
    for bad in ((3, 2, 16, 32, 3, 0, F32), (-1, 2, 16, 32, 3, 0, F32), (FWD, 2, 16, 32, 3, 0, 2)):
        assert L.sgx_gepi_plan(*bad, ctypes.addressof(out)) == -1, bad                            # SGX_EINVAL: entry, dtype
        L.sgx_clear_error()
    assert L.sgx_gepi_plan(FWD, 2, 16, 32, 3, 0, F32, None) == -1
    L.sgx_clear_error()


if __name__ == "__main__":                                                                        # a child process of the fixture `children`
    sys.path.insert(0, ROOT)
    from stylegan.pytorch_amd import native
    print(json.dumps(lib_plans(native.lib(), **REDUCED)))
