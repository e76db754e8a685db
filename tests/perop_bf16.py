"""Teacher-forced per-op bf16 check, shared by the YOLOv10 (test_gpu_parity.py) and YOLOv8 / YOLO11 (test_gpu_families_bf16.py) suites,
and the forced-id sweep cases both of them run (test_sweep_coverage.py pins, without a GPU, that every case's id is taken by its plan).

Each op consumes the bf16-emulating oracle's tensors (its output slice is overwritten with the oracle's tap after it ran), so the only
admissible difference is the bf16 rounding of an fp32 sum taken in another order: <= 1 bf16 ulp per element on < 2 % of the elements
(DESIGN.md section 2)."""
import collections

import torch

from helpers import make_case, make_case_family, nchw_to_nhwc, rel_err

# ---- forced-id sweep cases: (family, variant, seg, shape, cfg, fuse) --------------------------------------------------------------------
# Every case forces one conv tile configuration id (yp_debug_force_conv_cfg) and must find at least one op of its plan that launches with it
# (Engine.plan()[i]["cfg"]); together they take every id of every conv family plus 1000 (pwsp_kernel), less UNREACHABLE.

# Ids that no conv of any graph admits at any shape, each with the reason.
UNREACHABLE = {
    504: "conv_halo_s2 <2,4,4,2> (128 output channels): its LDS need, 3 x 36 KiB halo ring + 1 KiB + 9 x (Cin / 32) x 8 KiB of weights, "
         "is 181 KiB at the smallest admitted Cin = 32, over the 160 KiB the predicate allows, so it admits no layer",
}

_V10_IDS = (list(range(14)) + [100, 101, 102, 103, 200, 201, 202, 203, 204] + list(range(300, 341)) + list(range(400, 409)) + list(range(500, 505))
            + [600, 601, 602] + list(range(700, 713)) + list(range(800, 808)) + list(range(900, 904)) + [1000, 1100, 1101, 1102, 1200, 1201])
# ids that no op of v10-S-seg admits on the 24x40 .. 6x10 maps of (3, 96, 160): the halo / halo_p / wreg tiles want larger maps. They run
# on (1, 256, 256) instead (6-26 ops each), in the same position of the list (the test ids stay those of the moved cases).
_V10_MOVED = {100, 101, 103, 200, 201, 202, 203, 700, 701, 705, 706, 707, 708, 711, 712}


def _v10_sweep_case(c):
    if c == 504:      # UNREACHABLE: this position runs conv_halo_s2 id 500 in its plain form (model.1 un-fused) instead
        return ("v10", "s", True, (3, 96, 160), 500, False)
    return ("v10", "s", True, (1, 256, 256) if c in _V10_MOVED else (3, 96, 160), c, True)


V10_SWEEP = ([_v10_sweep_case(c) for c in _V10_IDS] +
             [("v10", "s", False, (1, 256, 256), c, True) for c in (500, 501, 502, 503)] +     # stride-2 halo family: model.1 / .3 / .17 all valid here
             [("v10", "x", False, (2, 128, 160), 200, True)] +     # (was 504, UNREACHABLE): 26 layers of the shipped v10-X table take 200
             # weights-resident 1x1: 48 / 192-channel rows of v10-M, 3-5 channel blocks. Of v10-X's 80 / 320-channel rows only 1102 admits any;
             # 1100 / 1101 / 1200 / 1201 run on v10-L (the same positions of the list)
             [("v10", "l" if v == "x" and c != 1102 else v, False, (2, 128, 160), c, True) for v in ("x", "m") for c in (1100, 1101, 1102, 1200, 1201)] +
             [("v10", "x", False, (1, 64, 64), c, True) for c in (801, 803, 807)] +      # pixels-direct 1x1 with Cin % 64 == 32 (80 / 160 / 480-channel layers of v10-X)
             [("v10", "x", False, (2, 128, 160), 101, True)] + [("v10", "m", False, (2, 128, 160), c, True) for c in (101, 103, 200)])   # the other ids the shipped X / M tables launch

# YOLOv8-seg / YOLO11-seg: every id on the graph and shape where the family's widths put it. 11-x (384-wide trunk, 96- / 48-channel C3k
# layers), 11-l and v8-m (48 / 96 / 192 / 576 channels: Cin % 64 == 32) on the fp32 layerwise shapes; the halo / halo_p / wreg / stride-2
# tiles on 11-s / v8-s at (1, 256, 256), where the maps are large enough for them.
_FAMILY_GRAPHS = (
    (("11", "x", (1, 64, 64)), list(range(14)) + list(range(800, 808)) + [1000, 1100, 1101, 1102, 1200, 1201]),
    (("v8", "m", (1, 64, 96)), list(range(300, 341))),
    (("11", "l", (1, 64, 64)), list(range(400, 409)) + list(range(900, 904)) + [600, 601, 602]),
    (("11", "s", (1, 256, 256)), [200, 201, 202, 203, 204, 500, 501, 502, 503, 700, 701, 705, 706, 707, 708, 712]),
    (("v8", "s", (1, 256, 256)), [100, 101, 102, 103, 702, 703, 704, 709, 710, 711]),
)
FAMILY_SWEEP = [(f, v, True, shape, c, True) for (f, v, shape), ids in _FAMILY_GRAPHS for c in ids]


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def ulps_bf16(got, want):
    """difference in units of the bf16 spacing at |want| (2^-7 of the leading power of two). The magnitude is
    floored at 2^-10 of the tensor's max: a result that cancels to ~0 still carries the fp32 summation noise of
    its O(max) terms (~1e-6*max), which is many 'ulps' of a tiny value but is not a rounding disagreement."""
    mag = want.abs().clamp_min(float(want.abs().max()) * 2.0 ** -10 + 2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return (got - want).abs() / ulp


_TAPS = collections.OrderedDict()     # (family, variant, seg, nc, shape) -> (state, frames, bf16emu taps): the CPU oracle runs once per graph


def oracle_case(family, variant, seg, nc, shape):
    key = (family, variant, seg, nc, tuple(shape))
    if key in _TAPS:
        _TAPS.move_to_end(key)
    else:
        taps = {}
        if family == "v10":
            from oracle.yolov10_oracle import Oracle
            st, im = make_case(variant, nc, seg, 0, shape)
            Oracle(st, variant, nc, seg, "bf16emu", tap=lambda n, x: taps.__setitem__(n, x.float())).forward(im)
        else:
            from oracle.yolo_seg_oracle import SegOracle
            st, im = make_case_family(family, variant, nc, 0, shape)
            SegOracle(st, family, variant, nc, "bf16emu", tap=lambda n, x: taps.__setitem__(n, x.float())).forward(im)
        _TAPS[key] = (st, im, taps)
        while len(_TAPS) > 4:
            _TAPS.popitem(last=False)
    st, im, taps = _TAPS[key]
    return {k: v.clone() for k, v in st.items()}, im.clone(), taps


def _amax_name(logit_conv):
    # "model.23.one2one_cv3.0.2" / "model.22.cv3.0.2" -> "model.23.amax.0" / "model.22.amax.0": the class-max op of that level
    p = logit_conv.split(".")
    return f"{p[0]}.{p[1]}.amax.{p[3]}"


def per_op_bf16(variant, seg, shape, cfg, fuse, monkeypatch, nc, want_tail=False, family="v10", autotune=None):
    """bf16 kernels one at a time: every op consumes the ORACLE's (bf16emu) tensors - after each op its output
    slice is overwritten with the oracle's tap - so the only admissible difference is the bf16 rounding of an
    fp32 sum taken in a different order: <= 1 bf16 ulp per element, on a small fraction of the elements.
    (The chained bf16 forward cannot be compared this tightly: once two bf16 trajectories differ they decorrelate
    to the bf16 noise floor, see test_end_to_end_bf16_accuracy.)
    cfg >= 0 forces that tile configuration id wherever it is valid, and at least one op must launch with it. autotune: None = the
    tuner's choices for cfg < 0 and the heuristic's otherwise; False / True to say. Returns the counters the callers assert on."""
    st, im, taps = oracle_case(family, variant, seg, nc, shape)
    from yolo_puncture_amd.engine import load_library
    assert load_library().yp_debug_force_conv_cfg(cfg) >= 14    # cfg >= 0: every conv that admits this tile config uses it
    try:
        return _per_op_bf16(st, im, taps, variant, seg, shape, cfg, fuse, monkeypatch, nc, want_tail, family, autotune)
    finally:
        load_library().yp_debug_force_conv_cfg(-1)         # (also when an assertion failed: the next test must not run under it)


def _per_op_bf16(st, im, taps, variant, seg, shape, cfg, fuse, monkeypatch, nc, want_tail, family, autotune):
    from yolo_puncture_amd.engine import Engine
    if not fuse:
        monkeypatch.setenv("YOLOP_NO_FUSE", "1")     # read at yp_create: the dw / pw kernels of the fused pairs run unfused
    eng = Engine(variant, nc, seg, "bf16", 0, state=st, family=family)
    if autotune is None:
        autotune = cfg < 0
    if not autotune:
        eng.set_autotune(False)
    imc = im.cuda()
    out = eng.forward(imc)               # allocates the plan; results are recomputed op by op below
    torch.cuda.synchronize()
    ops = eng.plan(*shape)
    if family == "v10" and shape == (2, 256, 384):           # 8x12 P5 map: the 7x7 depthwise runs on the matrix-core kernel, or inside pwsp_kernel behind its 1x1 conv
        k7 = [str(o.get("kernel", "")) for o in ops if o["name"].endswith("cv1.2")]
        assert k7 and all(k.startswith(("dwconv_mfma", "pwsp_kernel") if fuse else "dwconv_mfma") for k in k7), k7
    if family == "v10" and cfg >= 1100:
        assert variant != "s" or any(str(o.get("kernel", "")).startswith("conv_wres_kernel" if cfg < 1200 else "conv_wrs_kernel") for o in ops), "no op took the forced weights-resident configuration"
    # the ops that launch with the forced id: each is stepped below (yp_run_op launches an op as itself, also one the forward fuses away)
    ntaken = sum(1 for o in ops if o["kind"] != "head" and o["cfg"] == cfg) if cfg >= 0 else 0
    if cfg >= 0:
        assert ntaken > 0, f"no op of {family}{variant} {shape} launches with the forced configuration {cfg}: the case tests nothing"
    nclsout_planned = sum(1 for o in ops if str(o.get("kernel", "")).startswith("cls_out_kernel"))
    rows = []
    from yolo_puncture_amd.weights import fold_state
    folded = fold_state(st)
    nfused = ntail = npwsp = nclsout = 0
    for i, o in enumerate(ops):
        if o["kind"] == "head":
            continue
        eng.run_op(i, imc, out)
        is_pwsp = str(o.get("kernel", "")).startswith("pwsp_kernel") and o.get("pre", -1) >= 0
        if is_pwsp:
            npwsp += 1
        if is_pwsp and o["kind"] == "pool3":
            # pwsp_kernel, SPPF form: 1x1 conv -> three chained 5x5 max-pools in one launch. The pools are exact operators applied to the
            # kernel's own 1x1 result, which is within 1 bf16 ulp of the oracle's on a small fraction of elements - so are the pooled maps
            pre = ops[o["pre"]]
            y = [taps[pre["name"]]]
            for _ in range(3):
                y.append(torch.nn.functional.max_pool2d(y[-1], 5, 1, 2))
            t, c0, cc = o["out"]
            want = nchw_to_nhwc(torch.cat(y[1:], 1))
            got = eng.read_tensor(t)[..., c0:c0 + cc]
            u = ulps_bf16(got, want)
            assert float(u.max()) <= 1.0 + 1e-6 and float((u > 0).float().mean()) < 0.02, (o["name"], float(u.max()), float((u > 0).float().mean()))
            rows.append((o["name"], o["kind"], float(u.max()), float((u > 0).float().mean())))
            eng.write_tensor(t, c0, want)
            tp, cp0, cpc = pre["out"]
            if o["pre_stored"]:                                    # the 1x1's own output, written by the same launch: the strict contract again
                gp = eng.read_tensor(tp)[..., cp0:cp0 + cpc]
                up = ulps_bf16(gp, nchw_to_nhwc(taps[pre["name"]]))
                assert float(up.max()) <= 1.0 + 1e-6 and float((up > 0).float().mean()) < 0.02, (pre["name"], float(up.max()))
            eng.write_tensor(tp, cp0, nchw_to_nhwc(taps[pre["name"]]))
            continue
        if o["name"] not in taps:
            continue
        t, c0, cc = o["out"]
        got = eng.read_tensor(t)[..., c0:c0 + cc]
        want = nchw_to_nhwc(taps[o["name"]])
        is_f32 = eng.tensors()[t]["f32"]
        if is_f32 and str(o.get("kernel", "")).startswith("conv_dwpw"):
            # TAIL form: depthwise -> pointwise -> this logit conv in one kernel; neither intermediate leaves the chip. A 1-ulp flip of an
            # element of the pointwise result t moves a logit by |w3| * ulp(t); the fp32 sum itself carries summation-order noise 2e-5 * max
            pw_name = ops[i - 1]["name"]
            tmax = float(taps[pw_name].abs().max())
            wmax = float(folded[o["name"]][0].abs().max())
            ulp_t = 2.0 ** (torch.floor(torch.log2(torch.tensor(tmax))).item() - 7)
            d = (got - want).abs()
            bound = 2e-5 * float(want.abs().max()) + 6.0 * wmax * ulp_t
            assert float(d.max()) <= bound, (o["name"], float(d.max()), bound)
            assert float((d > 2e-5 * float(want.abs().max())).float().mean()) < 0.05, o["name"]     # ... and such flips are rare
            rows.append((o["name"], o["kind"], float(d.max() / want.abs().max()), 0.0))
            nfused += 1
            ntail += 1
            # the class-max keys the kernel wrote beside the logits: bits of sigmoid(max_c logit) of ITS logits
            am = [q for q in ops if q["name"] == _amax_name(o["name"])]
            if am and am[0]["kernel"] == "-":
                keys = eng.read_tensor(am[0]["out"][0])[..., 0]
                mx = got.max(-1).values
                assert float((keys - torch.sigmoid(mx)).abs().max()) < 2e-7, o["name"]
        elif is_f32:      # head logits are stored as fp32: compare like an fp32 op
            err = rel_err(got, want)
            rows.append((o["name"], o["kind"], err, 0.0))
            assert err < 2e-5, (o["name"], err)
            if str(o.get("kernel", "")).startswith("cls_out_kernel"):
                # the same launch wrote the class-max keys (the OP_AMAX op is skipped): bits of sigmoid(max_c logit) of ITS logits
                am = [q for q in ops if q["name"] == _amax_name(o["name"])]
                assert am and am[0]["kernel"] == "-", (o["name"], am)
                keys = eng.read_tensor(am[0]["out"][0])[..., 0]
                assert float((keys - torch.sigmoid(got.max(-1).values)).abs().max()) < 2e-7, o["name"]
                nclsout += 1
        elif str(o.get("kernel", "")).startswith(("conv_dwpw", "frontend_kernel", "c2f_fused_kernel", "scdown_fused_kernel")) or is_pwsp or \
                (str(o.get("kernel", "")).endswith(",false,false,true>") and "halo_s2" in str(o.get("kernel", ""))) or \
                (o["kernel"] == "-" and o["kind"] == "conv" and i + 1 < len(ops) and ",tail," in str(ops[i + 1].get("kernel", ""))):
            # (last case: the pointwise conv of a dw -> pw -> logits TAIL kernel; stepped on its own, yp_run_op runs it as the two-stage fused pair)
            # fused depthwise -> pointwise (and 3x3 s2 -> 1x1): the first stage's result never leaves the chip, so it cannot be teacher-forced.
            # It is itself within 1 bf16 ulp of the oracle's intermediate on a small fraction of elements (the contract
            # of every unfused op), and such a flip of element j moves output co by |w[co,j]| * ulp(t_j). Tolerance:
            # 1 output ulp + 4 simultaneous flips at the largest weight and the largest intermediate ulp; the differing
            # fraction stays small because almost all such moves are far below an output ulp.
            dw_name = ops[o["pre"] if is_pwsp else i - 1]["name"]   # the producer that was fused in (graph passes pair neighbours; pwsp names its own)
            tmax = float(taps[dw_name].abs().max())
            wmax = float(folded[o["name"]][0].abs().max())
            ulp_t = 2.0 ** (torch.floor(torch.log2(torch.tensor(tmax))).item() - 7)
            mag = torch.clamp(want.abs(), min=float(want.abs().max()) * 2.0 ** -10)
            ulp_o = torch.exp2(torch.floor(torch.log2(mag)) - 7)
            d = (got - want).abs()
            assert bool((d <= ulp_o * (1.0 + 1e-6) + 4.0 * wmax * ulp_t).all()), (o["name"], float((d / ulp_o).max()))
            u = d / ulp_o
            frac = float((u > 0).float().mean())
            rows.append((o["name"], o["kind"], min(float(u.max()), 1.0), frac))
            assert float((u > 1.0 + 1e-6).float().mean()) < 0.005, (o["name"], float((u > 1.0).float().mean()))
            assert frac < 0.05, (o["name"], frac)
            nfused += 1
            if is_pwsp:
                # the launch also wrote the 1x1's own output when that has other readers: strict per-op contract, then the oracle's values
                # again (this op overwrote what was teacher-forced after the stand-alone conv)
                pre = ops[o["pre"]]
                tp, cp0, cpc = pre["out"]
                if o["pre_stored"]:
                    gp = eng.read_tensor(tp)[..., cp0:cp0 + cpc]
                    up = ulps_bf16(gp, nchw_to_nhwc(taps[pre["name"]]))
                    assert float(up.max()) <= 1.0 + 1e-6 and float((up > 0).float().mean()) < 0.02, (pre["name"], float(up.max()))
                    eng.write_tensor(tp, cp0, nchw_to_nhwc(taps[pre["name"]]))
        else:
            u = ulps_bf16(got, want)
            frac = float((u > 0).float().mean())
            rows.append((o["name"], o["kind"], float(u.max()), frac))
            assert float(u.max()) <= 1.0 + 1e-6, (o["name"], float(u.max()))
            assert frac < 0.02, (o["name"], frac)
        eng.write_tensor(t, c0, want)    # teacher forcing
    print(family, variant, shape, "cfg", cfg, "ops that took it", ntaken, "ops checked", len(rows), "pwsp launches", npwsp, "cls_out launches", nclsout,
          "fused dw->pw ops", nfused, "of them with the logit conv as third stage", ntail, "max ulp", max(r[2] for r in rows if r[1] != "f32"),
          "max differing fraction", max(r[3] for r in rows))
    eng.close()
    assert len(rows) > 50
    assert nfused == 0 if not fuse else (nfused > 0 or shape != (2, 256, 384) or nc != 80)
    assert ntail > 0 if want_tail else ntail == 0
    if family == "v10" and fuse and cfg < 0 and variant == "s" and nc == 80 and not want_tail:
        assert nclsout == 3, nclsout                 # one per level: the logit conv and the class-max keys in one launch
    assert nclsout == nclsout_planned, (nclsout, nclsout_planned)      # every cls_out launch of the plan was checked
    return dict(ntaken=ntaken, nrows=len(rows), nfused=nfused, ntail=ntail, npwsp=npwsp, nclsout=nclsout,
                rows=[(n, k, e) for n, k, e, _ in rows])       # (op, kind, max ulp or relative error) per checked op
