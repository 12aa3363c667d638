"""CPU: what a weight-gradient call will launch, asked of the library itself.  sgx_wgrad_plan is the function the launchers run
(csrc/conv.hip, WgradPlan), so on a grid of shapes: (a) with the queried workspace it answers what tests/wgrad_ref.py restates, field by field;
(b) it answers the same with an unbounded workspace -- sgx_wgrad_ws_bytes is an upper-bound estimate that never binds the launcher's clamp,
which would otherwise change the split count and with it the summation order; (c) sgx_wgrad_ws_bytes returns what the commit before the
launchers were folded into one plan returned (tests/golden/wgrad_ws.json, written by tests/golden/make_golden_wgrad_ws.py); (d) under each
environment of wgrad_ref.GROUPS, in a child process (the switches are read once per process), the plan is the restated one; (e) values <= 0
of the four switches that treat them as unset plan as the default; (f) a workspace 4 bytes short of one split is SGX_EWORKSPACE from the plan.
The queries are host-only: without a GPU the library sizes its grids for 256 compute units, the MI355X's."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_ws.json")
NCU = 256
UNBOUNDED = 1 << 62

TAPS = (9, 16)
BATCHES = (1, 2, 4, 8, 32)
HEIGHTS = (4, 8, 16, 24, 32, 64, 128, 256, 512, 1024)                     # W = H below 32, else H rounded up to a multiple of 32
CHANNELS = (16, 32, 48, 64, 96, 128, 192, 256, 320, 512, 528)
MAX_ELEMS = 1 << 33
REDUCED = dict(batches=(4,), heights=(8, 32, 128))                        # the grid of the child processes
FIELDS = ("gen", "TH", "TW", "BP", "NSUB", "KSUB", "TR", "nsplit", "finish_ns", "pre", "EPB")
UNSET = {"SGX_WGRAD_BLOCKS": "-5", "SGX_WGRAD_MAXSPLIT": "0", "SGX_WGRAD_BLOCKS_MID": "-1", "SGX_WGRAD2_MAXCT": "0"}


def shapes(batches=BATCHES, heights=HEIGHTS):
    """(taps, B, H, W, Ck, Cn): H, W the k side's size, as the C ABI takes it."""
    for taps in TAPS:
        for B in batches:
            for H in heights:
                W = H if H < 32 else (H + 31) // 32 * 32
                for Ck in CHANNELS:
                    for Cn in CHANNELS:
                        if B * H * W * max(Ck, Cn) <= MAX_ELEMS:
                            yield taps, B, H, W, Ck, Cn


def lib_plan(L, shape, dtype, wsb):
    """-> (rc, the eleven ints of sgx_wgrad_plan as a list)."""
    out = (ctypes.c_int * len(FIELDS))()
    rc = L.sgx_wgrad_plan(*shape, dtype, wsb, ctypes.addressof(out))
    if rc:
        L.sgx_clear_error()
    return rc, list(out)


def lib_plans(L, grid):
    """Every shape of the grid, fp32 then bf16, with the workspace sgx_wgrad_ws_bytes asks for."""
    return [lib_plan(L, s, dt, L.sgx_wgrad_ws_bytes(*s)) for s in grid for dt in (0, 1)]


def decode(shape, dtype, rc, v):
    """The library's ints as wgrad_ref.plan spells them: (rc, kernels, nsplit, finish_ns, gen)."""
    import wgrad_ref as WR
    f = dict(zip(FIELDS, v))
    if rc:
        return rc, (), 0, None, 1
    taps = shape[0]
    if f["gen"] == 1:
        kernels = [f"wgrad_kernel<{'float' if dtype == 0 else 'bf16_t'}, {0 if taps == 9 else 1}, {f['TH']}, {f['TW']}, {f['BP']}, {f['NSUB']}, {f['KSUB']}, {'true' if f['TR'] else 'false'}>"]
    else:
        kern = (WR.W16 if f["KSUB"] == 16 else WR.W2S) if taps == 9 else WR.w2d(f["KSUB"])
        assert (f["TH"], f["TW"], f["BP"]) == {WR.W16: (16, 32, 512), WR.W2S: (8, 32, 256)}.get(kern, (4, 16, 64)), (shape, f)
        assert dtype == 1 and f["NSUB"] == 0 and f["TR"] == 0, (shape, f)
        kernels = [kern]
    if f["pre"]:
        kernels.append(WR.PRE)
    if f["finish_ns"]:
        kernels.append(WR.fin(f["EPB"]))
    else:
        assert f["gen"] == 1 and f["nsplit"] == 1 and not f["pre"], (shape, f)
    return rc, tuple(kernels), f["nsplit"], f["finish_ns"] or None, f["gen"]


def restated(shape, dtype, wsb, env):
    import wgrad_ref as WR
    taps, B, H, W, Ck, Cn = shape
    p = WR.plan(WR.S3 if taps == 9 else WR.S4, WR.F if dtype == 0 else WR.H, B, H, W, Ck, Cn, Cn, Ck, wsb, env, NCU)
    return p.rc, p.kernels, p.nsplit, p.finish_ns, p.gen


def differences(got, grid, env):
    import wgrad_ref as WR
    it = iter(got)
    wrong = []
    for s in grid:
        wsb = WR.ws_bytes(*s, env, NCU)
        for dt in (0, 1):
            rc, v = next(it)
            g, w = decode(s, dt, rc, v), restated(s, dt, wsb, env)
            if g != w:
                wrong.append("%s dtype %d: library %s, restated %s" % (s, dt, g, w))
    return wrong


@pytest.fixture(scope="module")
def L():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def children(L):
    """group -> the child's plans on the reduced grid.  All started at once, after the fixture ``L`` has built the library: each only loads it
    and answers host-side queries."""
    import wgrad_ref as WR
    envs = dict({g: e for g, e in WR.GROUPS.items() if g != "default"}, unset=UNSET)
    base = {k: v for k, v in os.environ.items() if not k.startswith("SGX_WGRAD")}
    procs = {g: subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=dict(base, **e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for g, e in envs.items()}
    out = {}
    for g, p in procs.items():
        so, se = p.communicate()
        assert p.returncode == 0, (g, se[-2000:])
        out[g] = [tuple(r) for r in json.loads(so.splitlines()[-1])]
    return out


def test_the_grid_is_the_one_described():
    assert len(list(shapes())) == 2 * (5 * 10 * 121 - 57) == 11986           # B32 1024x1024 with more than 256 channels: above 2^33 elements
    assert len(list(shapes(**REDUCED))) == 2 * 3 * 121


def test_the_plan_is_the_restated_one_and_the_query_never_binds(L):
    import wgrad_ref as WR
    grid = list(shapes())
    got = lib_plans(L, grid)
    wrong = differences(got, grid, WR.ENV0)                                                       # (a)
    assert not wrong, "%d of %d plans differ:\n%s" % (len(wrong), len(got), "\n".join(wrong[:40]))
    unbounded = [lib_plan(L, s, dt, UNBOUNDED) for s in grid for dt in (0, 1)]                    # (b)
    bound = [(s, dt, g, u) for (s, dt), g, u in zip(((s, dt) for s in grid for dt in (0, 1)), got, unbounded) if g != u]
    assert not bound, "the queried workspace changes %d of %d plans:\n%s" % (len(bound), len(got), "\n".join(map(str, bound[:40])))
    gens = {(dt, v[0]) for (rc, v), dt in zip(got, (d for _ in grid for d in (0, 1)))}
    assert gens == {(0, 1), (1, 1), (1, 2)} and all(rc == 0 for rc, _ in got)


def test_the_workspace_query_returns_what_was_recorded(L):
    import wgrad_ref as WR
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["ncu"] == NCU and fx["axes"] == {"taps": list(TAPS), "B": list(BATCHES), "H": list(HEIGHTS), "Ck": list(CHANNELS), "Cn": list(CHANNELS)}
    grid = list(shapes())
    assert len(fx["ws_bytes"]) == len(grid)
    wrong = [(s, L.sgx_wgrad_ws_bytes(*s), w) for s, w in zip(grid, fx["ws_bytes"]) if L.sgx_wgrad_ws_bytes(*s) != w]    # (c)
    assert not wrong, "%d of %d sizes differ (shape, returned, recorded):\n%s" % (len(wrong), len(grid), "\n".join(map(str, wrong[:40])))
    assert all(WR.ws_bytes(*s, WR.ENV0, NCU) == w for s, w in zip(grid, fx["ws_bytes"]))


def test_every_switch_group_plans_as_restated(children):
    import wgrad_ref as WR
    grid = list(shapes(**REDUCED))
    assert set(children) == set(WR.GROUPS) - {"default"} | {"unset"} and len(children) == 11
    for g in WR.GROUPS:                                                                           # (d)
        if g != "default":
            wrong = differences(children[g], grid, WR.group_env(g))
            assert not wrong, "group %s: %d plans differ:\n%s" % (g, len(wrong), "\n".join(wrong[:40]))
    # each group's switch moves some plan of the reduced grid
    assert all(children[g] != children["unset"] for g in WR.GROUPS if g != "default")


def test_values_that_mean_unset_plan_as_the_default(L, children):
    assert children["unset"] == lib_plans(L, list(shapes(**REDUCED)))                             # (e)


def test_the_compiled_first_generation_kernels_are_the_rows(L):
    """WGRAD_TABLE's entries are what csrc/conv.hip compiles of wgrad_kernel (the compiler's resource remarks of the build just made): exactly the
    54 instantiations the rows of wgrad_ref.CASES name, so a plan that (a) allows always finds its slot of the table filled."""
    import importlib.util
    import wgrad_ref as WR
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    built = {k["name"].replace("unsigned short", "bf16_t").replace("(WgradArgs)", "") for k in kr.collect() if k["name"].startswith("wgrad_kernel<")}
    named = {k for c in WR.CASES for k in c.kernels if k.startswith("wgrad_kernel<")}
    assert built == named and len(built) == 54, (sorted(built - named), sorted(named - built))


def test_the_query_refuses_what_the_entry_point_refuses(L):
    out = (ctypes.c_int * len(FIELDS))()
    for bad in ((16, 4, 31, 32, 32, 32, 0), (16, 4, 32, 31, 32, 32, 1), (12, 4, 32, 32, 32, 32, 0), (9, 4, 32, 32, 32, 32, 2)):
        assert L.sgx_wgrad_plan(*bad, UNBOUNDED, ctypes.addressof(out)) == -1, bad            # SGX_EINVAL: odd fine size, taps, dtype
        L.sgx_clear_error()


def test_a_workspace_short_of_one_split_is_an_error_of_the_plan(L):
    import wgrad_ref as WR
    for s in ((9, 4, 16, 16, 32, 32), (9, 4, 32, 32, 64, 64), (16, 4, 32, 32, 64, 64), (9, 2, 128, 128, 16, 16)):
        one = (s[0] * s[4] * s[5] + s[5]) * 4
        for dt in (0, 1):                                                                         # (f)
            assert lib_plan(L, s, dt, one - 4)[0] == WR.EWORKSPACE, (s, dt)
            rc, v = lib_plan(L, s, dt, one)
            assert rc == 0 and v[0] == 1 and v[7] == 1 and v[8] == 0, (s, dt, v)                  # one split: the first generation's direct epilogue


if __name__ == "__main__":                                                                        # a child process of the fixture `children`
    sys.path.insert(0, ROOT)
    from stylegan.pytorch_amd import native
    print(json.dumps(lib_plans(native.lib(), list(shapes(**REDUCED)))))
