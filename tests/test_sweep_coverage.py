"""The forced-id sweeps of the per-op bf16 tests (perop_bf16.py: V10_SWEEP, FAMILY_SWEEP) are not vacuous: each case's plan has an op that
launches with the id it forces, and together they take every configuration id of every conv family plus 1000 (pwsp_kernel), less the ids
no layer admits. Plans and the id each op launches with (yp_debug_op_cfg) are host-side: no GPU needed."""
import pytest

from perop_bf16 import FAMILY_SWEEP, UNREACHABLE, V10_SWEEP
from yolo_puncture_amd.engine import Engine, conv_families, load_library

PWSP_CFG = 1000
# the kernel each family's configurations launch, as the plan names it (yp_op_kernel)
_KERNEL = {100: "conv_halo_kernel<", 200: "conv_halo_p_kernel<", 300: "conv_dma_p_kernel<", 400: "conv_dma_lc_kernel<", 500: "conv_halo_s2_kernel<",
           600: "conv_tile1", 700: "conv_wreg_kernel<", 800: "conv_pxd_kernel<", 900: "conv_ks_kernel<", 1100: "conv_wres_kernel<",
           1200: "conv_wrs_kernel<"}


def _taken(cases, monkeypatch):
    """-> {case: number of non-head ops that launch with the case's id}"""
    lib = load_library()
    got = {}
    groups = {}
    for c in cases:
        groups.setdefault((c[0], c[1], c[2], c[5]), []).append(c)
    try:
        for (family, variant, seg, fuse), cs in groups.items():
            if fuse:
                monkeypatch.delenv("YOLOP_NO_FUSE", raising=False)
            else:
                monkeypatch.setenv("YOLOP_NO_FUSE", "1")          # read at yp_create
            e = Engine(variant, 80, seg, "bf16", 0, family=family)
            for c in cs:
                shape, cfg = c[3], c[4]
                lib.yp_debug_force_conv_cfg(cfg)
                e.plan(1, 32, 32)                                  # (a plan of the same shape is kept as it is: plan another shape first)
                ops = [o for o in e.plan(*shape) if o["kind"] != "head"]
                took = [o for o in ops if o["cfg"] == cfg]
                got[c] = len(took)
                fam = max((b for b in _KERNEL if b <= cfg), default=None)
                if cfg >= 100 and cfg != PWSP_CFG:
                    # the id the accessor reports is the kernel the plan names (skipped ops launch only when stepped: they name none)
                    for o in took:
                        assert o["kernel"] == "-" or o["kernel"].startswith(_KERNEL[fam]), (c, o["name"], o["kernel"])
            e.close()
    finally:
        lib.yp_debug_force_conv_cfg(-1)
    return got


def _all_ids():
    return {b + i for b, n in conv_families() for i in range(n)} | {PWSP_CFG}


def test_conv_family_table():
    fams = conv_families()
    assert len(fams) == 12 and fams[0] == (0, 14)
    ids = sorted(b + i for b, n in fams for i in range(n))
    assert len(ids) == len(set(ids)) and PWSP_CFG not in ids          # the ranges are disjoint, and 1000 is no family's
    assert {b for b, _ in fams} == {0} | set(_KERNEL)


@pytest.mark.parametrize("name,cases", [("v10", V10_SWEEP), ("families", FAMILY_SWEEP)])
def test_sweep_cases_take_their_id(name, cases, monkeypatch):
    assert len(set(cases)) == len(cases), "a case appears twice"
    got = _taken(cases, monkeypatch)
    idle = [c for c in cases if got[c] == 0]
    assert not idle, f"{name}: cases whose plan has no op on the forced id: {idle}"
    # every id of every family (and 1000) is swept, except those no layer admits
    swept = {c[4] for c in cases}
    assert not swept & set(UNREACHABLE)
    assert swept == _all_ids() - set(UNREACHABLE), sorted(swept ^ (_all_ids() - set(UNREACHABLE)))


def test_unreachable_ids_are_admitted_by_no_layer(monkeypatch):
    """The exclusions hold on every graph of both sweeps, at their shapes and at full frame."""
    graphs = {(c[0], c[1], c[2], c[3], c[5]) for c in V10_SWEEP + FAMILY_SWEEP} | \
             {(f, v, True, (1, 640, 640), True) for f in ("v10", "v8", "11") for v in "nsmlx"}
    cases = [(f, v, seg, shape, cfg, fuse) for f, v, seg, shape, fuse in sorted(graphs) for cfg in UNREACHABLE]
    got = _taken(cases, monkeypatch)
    assert not any(got.values()), [c for c in cases if got[c]]
