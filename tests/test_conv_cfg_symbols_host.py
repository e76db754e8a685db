"""Every configuration id of every conv family keeps the kernel symbols it reports and the ops it reaches, and the library keeps exactly
the family kernels' instances it had: tests/golden/conv_cfg_symbols.txt records both, written by this module's --write switch. Each id is
forced in turn (yp_debug_force_conv_cfg) and unfinalized bf16 engines are planned; per id, the ops that launch with it (cfg == id and a
kernel of their own) are counted and their kernel names collected. Id 504 is admitted by no shape: its line records
the LDS bytes conv_s2_admits reports for its one intended layer. The second part lists the library's kernel symbols of the 12 families.
After adding or changing a tile configuration: python tests/test_conv_cfg_symbols_host.py --write. No GPU needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
from yolo_puncture_amd.engine import Engine, conv_families, conv_s2_admits, load_library

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_cfg_symbols.txt")
ENGINES = [("v10", v, seg) for v in "nsmblx" for seg in (False, True)] + [("11", "n", True), ("11", "s", True), ("v8", "n", True)]
SHAPES = [(1, 640, 640), (8, 640, 640), (1, 96, 128), (2, 1280, 1280)]
# the kernel templates of the 12 families (conv_wres_clk_kernel: conv_wres' stamped debug instance)
FAMILY_KERNELS = {"conv_dma_kernel", "conv_halo_kernel", "conv_halo_p_kernel", "conv_dma_p_kernel", "conv_halo_s2_kernel", "conv_tile1_kernel",
                  "conv_tile1w_kernel", "conv_dma_lc_kernel", "conv_wreg_kernel", "conv_pxd_kernel", "conv_ks_kernel", "conv_wres_kernel",
                  "conv_wres_clk_kernel", "conv_wrs_kernel"}
NEVER_ADMITTED = {504: (1, 64, 64, 32, 128)}       # id -> (B, H, W, Cin, Cout) of the layer it was written for


def _all_ids():
    return [b + i for b, n in conv_families() for i in range(n)]


def _reach():
    """-> {id: (number of ops that launch with it, sorted kernel names)} over ENGINES x SHAPES"""
    lib = load_library()
    ids = _all_ids()
    count = {i: 0 for i in ids}
    names = {i: set() for i in ids}
    try:
        for family, variant, seg in ENGINES:
            e = Engine(variant, 80, seg, "bf16", 0, finalize=False, family=family)
            for cfg in ids:
                lib.yp_debug_force_conv_cfg(cfg)
                for shape in SHAPES:
                    e.plan(1, 64, 64)                      # (a plan of the same shape is kept as it is: re-plan from scratch)
                    for o in e.plan(*shape):
                        if o["cfg"] == cfg and o["kernel"] != "-":
                            count[cfg] += 1
                            names[cfg].add(o["kernel"].replace(" ", ""))
            e.close()
    finally:
        lib.yp_debug_force_conv_cfg(-1)
    return {i: (count[i], sorted(names[i])) for i in ids}


def _render():
    lines = ["# part 1: configuration id, ops that launch with it, the kernel symbols they report"]
    for i, (n, ks) in sorted(_reach().items()):
        if i in NEVER_ADMITTED:
            ok, lds, _ = conv_s2_admits(i, *NEVER_ADMITTED[i])
            assert n == 0 and not ok, (i, n, ok)
            lines.append(f"{i} never admitted, {lds}")
        else:
            lines.append(f"{i} {n} " + " ".join(ks))
    lines.append("# part 2: the library's kernel symbols of the conv families")
    lines += sorted(s for s in _kernel_symbols(load_library()._name) if s.split("<")[0] in FAMILY_KERNELS)
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def rendered(request):
    os.environ.pop("YOLOP_TUNE_CACHE", None)
    return _render()


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_ids_keep_their_symbols_reach_and_instances(rendered):
    want = open(GOLDEN).read()
    if rendered != want:
        got, exp = rendered.splitlines(), want.splitlines()
        diff = [(g, w) for g, w in zip(got, exp) if g != w][:5]
        pytest.fail(f"{len(got)} lines against {len(exp)}; first differing (got, expected): {diff}")


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_fixture_lists_every_id_and_only_kernel_symbols():
    part1 = open(GOLDEN).read().split("# part 2")[0].splitlines()[1:]
    assert [int(ln.split()[0]) for ln in part1] == sorted(_all_ids())
    syms = _kernel_symbols(load_library()._name)
    reached = 0
    for ln in part1:
        f = ln.split()
        if int(f[0]) in NEVER_ADMITTED:
            assert ln == f"{f[0]} never admitted, 185344"
            continue
        assert int(f[1]) > 0 and len(f) > 2, f"id {f[0]} is reached by no op"
        reached += 1
        for k in f[2:]:
            assert k in syms, (f[0], k)
    assert reached == len(part1) - len(NEVER_ADMITTED)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: test_conv_cfg_symbols_host.py --write")
    os.environ.pop("YOLOP_TUNE_CACHE", None)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        fh.write(_render())
    print("wrote", GOLDEN)
