"""GPU parity tests proper: the HIP path (through the C-ABI, via ctypes) against the CPU oracle on the same
seeded inputs. Tolerances are stated where they are used; their basis is in DESIGN.md "Parity contract"."""
import json
import os

import pytest
import torch

from helpers import make_case, nchw_to_nhwc, rel_err
from perop_bf16 import V10_SWEEP, per_op_bf16

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


def _engine(variant, nc, seg, dtype, st):
    from yolo_puncture_amd.engine import Engine
    return Engine(variant, nc, seg, dtype, 0, state=st)


def _layerwise(variant, seg, dtype, mode, shape, seed=0, nc=80):
    """Run engine + oracle, compare every conv-like op's output slice with the oracle tap of the same name.
    -> list of (op name, kind, rel err) in execution order, final outputs of both."""
    from oracle.yolov10_oracle import Oracle
    st, im = make_case(variant, nc, seg, seed, shape)
    taps = {}
    ref = Oracle(st, variant, nc, seg, mode, tap=lambda n, x: taps.__setitem__(n, x.float())).forward(im)
    eng = _engine(variant, nc, seg, dtype, st)
    out = eng.forward(im.cuda())
    torch.cuda.synchronize()
    ops = eng.plan(*shape)
    owner = {}
    for i, o in enumerate(ops):           # last writer of every (tensor, channel) wins
        t, c0, cc = o["out"]
        for c in range(c0, c0 + cc):
            owner[(t, c)] = i
    cache = {}
    rows = []
    for i, o in enumerate(ops):
        if o["name"] not in taps or o["kind"] not in ("stem", "conv", "dwconv", "attn", "convT"):
            continue
        t, c0, cc = o["out"]
        if t not in cache:
            cache[t] = eng.read_tensor(t)
        keep = [c for c in range(cc) if owner[(t, c0 + c)] == i]
        if not keep:
            continue
        got = cache[t][..., c0:c0 + cc][..., keep]
        want = nchw_to_nhwc(taps[o["name"]])[..., keep]
        rows.append((o["name"], o["kind"], rel_err(got, want)))
    res = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
    if seg:
        res["proto"] = eng.proto()
    eng.close()
    return rows, res, ref


def _dump(tag, rows):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"layerwise_{tag}.json"), "w") as f:
        json.dump([dict(op=n, kind=k, rel_err=e) for n, k, e in rows], f, indent=1)


@pytest.mark.parametrize("variant,seg,shape", [("n", True, (2, 96, 128)), ("s", False, (1, 160, 192)),
                                               ("m", False, (1, 64, 96)), ("x", False, (1, 64, 64))])
def test_layerwise_fp32(variant, seg, shape):
    """fp32 engine (MFMA 16x16x4 f32 = exact fp32 FMA chains) vs fp32 oracle: every op output within 1e-4 of the
    tensor's max magnitude (fp32 accumulation-order noise through <=60 layers; fp64-vs-fp32 oracle gives 1e-5)."""
    rows, res, ref = _layerwise(variant, seg, "fp32", "fp32", shape)
    _dump(f"fp32_{variant}", rows)
    assert len(rows) > 50
    tol = 1e-4 if variant in "nsm" else 5e-4   # 174 chained convs on a 2x2 P5 map (x @64x64) measured 1.7e-4
    bad = [(n, e) for n, _, e in rows if not (e < tol)]
    assert not bad, bad[:10]


def _per_op_bf16(*a, **k):
    _dump(f"perop_bf16_{a[0]}", per_op_bf16(*a, **k)["rows"])


@pytest.mark.parametrize("variant,seg,shape,cfg,fuse",
                         [("n", True, (2, 96, 128), -1, True), ("s", False, (1, 160, 192), -1, True), ("x", False, (1, 64, 64), -1, True),
                          ("s", False, (2, 256, 384), -1, True), ("s", False, (2, 256, 384), -1, False),
                          ("s", False, (1, 480, 608), -1, True), ("m", False, (2, 128, 160), -1, True)] +   # (m: 288- / 576-channel rows, K % 64 == 32)      # 60x76 at P3: partial tiles of the fused SCDown (4x8) and C2f-tail (8x16) kernels
                         [c[1:] for c in V10_SWEEP])      # every conv tile configuration id, each on a graph and shape where ops take it (perop_bf16.py)
def test_per_op_bf16_teacher_forced(variant, seg, shape, cfg, fuse, monkeypatch):
    _per_op_bf16(variant, seg, shape, cfg, fuse, monkeypatch, 80)


@pytest.mark.parametrize("variant,seg,shape", [("s", True, (1, 256, 320)), ("s", False, (2, 256, 384)), ("s", False, (1, 480, 608))])
def test_per_op_bf16_tail_form(variant, seg, shape, monkeypatch):
    """conv_dwpw's TAIL form (YOLOP_TAIL=1: the class branch's logit conv and the class-max keys as a third stage of the last dw -> pw pair;
    opt-in because the replayed step is not faster with it): same per-op contract, keys = sigmoid(max logit) of the kernel's own logits.
    (The form needs a 128-wide class branch - variant s at nc = 80 - and level maps that fill the kernel's 8x16 tiles.)"""
    monkeypatch.setenv("YOLOP_TAIL", "1")
    _per_op_bf16(variant, seg, shape, -1, True, monkeypatch, 80, want_tail=True)


@pytest.mark.parametrize("variant,seg,shape,nc", [("s", True, (3, 96, 160), 1), ("s", True, (3, 96, 160), 3), ("n", False, (2, 256, 384), 1),
                                                  ("s", False, (1, 160, 192), 3)])
def test_per_op_bf16_small_nc(variant, seg, shape, nc, monkeypatch):
    """The class counts of the reference's checkpoints - needle fine-tunes, nc = 1 or a handful (yolo_seg/app.py:218-223,
    yolo_with_deva.py:226): a 1- / 3-channel fp32 class map through the conv epilogues' 4-channel lane stores, the class-max pass'
    scalar branch and the class branch's narrow (max(ch0, min(nc,100)) wide) depthwise -> pointwise pairs. Same per-op contract as nc = 80."""
    _per_op_bf16(variant, seg, shape, -1, True, monkeypatch, nc)


def _final_report(res, ref, k):
    det, rdet = res["det"][:, :k], ref["det"]
    idx, ridx = res["idx"][:, :k].long(), ref["idx"]
    same = (idx == ridx) & (det[..., 5] == rdet[..., 5])
    return dict(box=float((det[..., :4] - rdet[..., :4])[same].abs().max()) if same.any() else 0.0,
                score=float((det[..., 4] - rdet[..., 4]).abs().max()), agree=float(same.float().mean()))


@pytest.mark.parametrize("variant,seg,shape,nc", [("n", True, (2, 96, 128), 80), ("s", False, (2, 320, 320), 80),
                                                  ("n", False, (1, 640, 640), 80), ("n", True, (2, 96, 128), 1), ("s", False, (2, 320, 320), 3)])
def test_end_to_end_fp32(variant, seg, shape, nc):
    """[B,300,6] + anchor indices, fp32 engine vs the oracle. Indices and class ids identical on every row whose score gap to its
    neighbours exceeds 1e-5; box / score / coefficient / prototype floats within 2 x the reference's own fp32 noise floor, measured per
    case as |oracle_fp32 - oracle_fp64| (helpers.assert_within_noise_floor; north_star's 1e-3 is printed beside both numbers).
    nc = 1 / 3: the class counts of the reference's needle checkpoints (yolo_seg/app.py:218-223)."""
    from oracle.yolov10_oracle import Oracle
    from helpers import assert_within_noise_floor
    rows, res, ref = _layerwise(variant, seg, "fp32", "fp32", shape, nc=nc)
    st, im = make_case(variant, nc, seg, 0, shape)
    ref64 = Oracle(st, variant, nc, seg, "fp64").forward(im)
    k = ref["det"].shape[1]
    rep = _final_report(res, ref, k)
    s = ref["det"][..., 4]
    gap = torch.minimum((s[:, :-1] - s[:, 1:]).abs(), torch.ones(())).clamp_min(0)
    safe = torch.ones_like(s, dtype=torch.bool)
    safe[:, 1:] &= gap > 1e-5
    safe[:, :-1] &= gap > 1e-5
    idx_ok = (res["idx"][:, :k].long() == ref["idx"]) & (res["det"][:, :k, 5] == ref["det"][..., 5])
    print(variant, shape, "nc", nc, rep, "near-tie rows:", float((~safe).float().mean()))
    assert bool(idx_ok[safe].all()), "index/class mismatch on a row with a clear score gap"
    assert safe.float().mean() > 0.5
    # rows on which engine, fp32 oracle and fp64 oracle all hold the same (anchor, class): the floats of those rows are comparable
    same = idx_ok & (ref64["idx"] == ref["idx"]) & (ref64["det"][..., 5].float() == ref["det"][..., 5])
    assert same.float().mean() > 0.9, float(same.float().mean())
    det = res["det"][:, :k]
    assert_within_noise_floor("boxes [px]", det[..., :4][same], ref["det"][..., :4][same], ref64["det"][..., :4][same], 1e-3)
    assert_within_noise_floor("scores", det[..., 4][same], ref["det"][..., 4][same], ref64["det"][..., 4][same], 1e-3, ceiling=1e-4)
    if seg:
        assert_within_noise_floor("mask coefficients", res["coeff"][:, :k][same], ref["coeff"][same], ref64["coeff"][same], 1e-3)
        assert_within_noise_floor("prototypes", res["proto"], nchw_to_nhwc(ref["proto"]), nchw_to_nhwc(ref64["proto"]), 1e-3, ceiling=1e-3)


@pytest.mark.parametrize("variant,seg,shape,dense", [("n", True, (2, 96, 128), True), ("s", False, (2, 320, 320), True),
                                                       ("n", True, (2, 96, 128), False), ("s", False, (2, 320, 320), False), ("s", True, (3, 160, 192), False)])
def test_end_to_end_bf16_accuracy(variant, seg, shape, dense, monkeypatch):
    """Chained bf16 forward. Two faithful bf16 implementations decorrelate over ~60 re-rounded layers, so the
    engine is not compared with the bf16emu oracle element by element; instead both are measured against the fp32
    oracle (the reference's CPU path) on the head's raw logits: the engine's error must not exceed 1.25x the error of the
    bf16-emulating oracle (i.e. it is as accurate as bf16 storage allows). dense: every branch of the head dense (YOLOP_DENSE_HEAD=1), all
    anchors compared; else the default winners-only head - box logits (and mask coefficients) exist at the stage-1 winners only and are
    compared there, row by row, with the oracle's maps at those anchors."""
    from oracle.yolov10_oracle import Oracle
    if dense:
        monkeypatch.setenv("YOLOP_DENSE_HEAD", "1")
    st, im = make_case(variant, 80, seg, 0, shape)
    t32, t16 = {}, {}
    Oracle(st, variant, 80, seg, "fp32", tap=lambda n, x: t32.__setitem__(n, x.float())).forward(im)
    Oracle(st, variant, 80, seg, "bf16emu", tap=lambda n, x: t16.__setitem__(n, x.float())).forward(im)
    eng = _engine(variant, 80, seg, "bf16", st)
    eng.forward(im.cuda())
    torch.cuda.synchronize()
    rep = {}
    B = shape[0]
    mode, sel, rows, cfrows = eng.head_winners(B)
    assert (mode == 0) == dense, mode
    names = [f"model.23.one2one_cv3.{l}.2" for l in range(3)]
    if dense or not (mode & 1):
        names += [f"model.23.one2one_cv2.{l}.2" for l in range(3)]
    if seg:
        names += ["model.23.proto.cv3"]
        if dense or not (mode & 2):
            names += [f"model.23.cv4.{l}.2" for l in range(3)]
    for n in names:
        got = eng.read_tensor(eng.find_tensor(n))
        truth = nchw_to_nhwc(t32[n])
        e_eng = float((got - truth).abs().mean())
        e_emu = float((nchw_to_nhwc(t16[n]) - truth).abs().mean())
        rep[n] = (e_eng, e_emu)
        assert e_eng <= 1.25 * e_emu + 1e-6, (n, e_eng, e_emu)
    if not dense:
        # the winners' rows against the oracle's maps at the same anchors (all three levels pooled: a level may hold a handful of winners)
        A_l = [(shape[1] // s) * (shape[2] // s) for s in (8, 16, 32)]
        k = min(eng.max_det, sum(A_l))
        for bit, pre, width, got_rows in ((1, "model.23.one2one_cv2", 64, rows), (2, "model.23.cv4", 32, cfrows)):
            if not (mode & bit):
                continue
            flat32 = torch.cat([nchw_to_nhwc(t32[f"{pre}.{l}.2"]).reshape(B, -1, width) for l in range(3)], 1)
            flat16 = torch.cat([nchw_to_nhwc(t16[f"{pre}.{l}.2"]).reshape(B, -1, width) for l in range(3)], 1)
            bi = torch.arange(B)[:, None].expand(B, k)
            truth, emu = flat32[bi, sel[:, :k].long()], flat16[bi, sel[:, :k].long()]
            e_eng, e_emu = float((got_rows[:, :k] - truth).abs().mean()), float((emu - truth).abs().mean())
            rep[pre + " (winners)"] = (e_eng, e_emu)
            assert e_eng <= 1.25 * e_emu + 1e-6, (pre, e_eng, e_emu)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"e2e_bf16_{variant}.json"), "w") as f:
        json.dump(rep, f, indent=1)
    print(variant, shape, {k: (round(a, 5), round(b, 5)) for k, (a, b) in rep.items()})
    eng.close()


@pytest.mark.parametrize("variant,seg,shape,nc", [("s", True, (3, 160, 192), 80), ("n", False, (2, 256, 384), 80), ("s", False, (1, 480, 608), 80), ("m", True, (1, 96, 128), 80),
                                                  ("n", False, (2, 128, 160), 3), ("s", True, (2, 96, 128), 1), ("n", False, (5, 32, 64), 80)])
def test_winners_only_head_equals_dense(variant, seg, shape, nc, monkeypatch):
    """The default head evaluates the box branch (and the coefficient branch where its width is 32) at the top-k winners only
    (head_branch.hip). Against the same engine with every branch dense (YOLOP_DENSE_HEAD=1): anchors, classes and scores are bit-identical
    (they depend on the class branch alone); the winners' box logits / coefficients are the dense maps' values at those anchors up to fp32
    summation order through two bf16-rounded intermediates - almost all of them within 1e-3 of the map's range, none beyond 5 %; boxes
    move by a fraction of a pixel. Frame borders (zero padding of both 3x3 convolutions) are part of every case: winners sit on them.
    Also: class counts 1 / 3 (the reference's needle checkpoints) and a frame with fewer anchors than max_det (every anchor a winner,
    every position listed)."""
    st, im = make_case(variant, nc, seg, 0, shape)
    imc = im.cuda()
    B = shape[0]
    sp = _engine(variant, nc, seg, "bf16", st)
    sp.set_autotune(False)
    out_s = {k: v.cpu() for k, v in sp.forward(imc).items() if v is not None}
    mode, sel, rows, cfrows = sp.head_winners(B)
    assert mode & 1, "the box branch should run winners-only for this model"
    sp.close()
    monkeypatch.setenv("YOLOP_DENSE_HEAD", "1")
    de = _engine(variant, nc, seg, "bf16", st)
    de.set_autotune(False)
    out_d = {k: v.cpu() for k, v in de.forward(imc).items() if v is not None}
    assert de.head_winners(B)[0] == 0
    assert torch.equal(out_s["idx"], out_d["idx"]) and torch.equal(out_s["det"][..., 4:], out_d["det"][..., 4:])
    A_l = [(shape[1] // s) * (shape[2] // s) for s in (8, 16, 32)]
    k = min(sp.max_det, sum(A_l))
    bi = torch.arange(B)[:, None].expand(B, k)
    for bit, pre, width, got_rows in ((1, "model.23.one2one_cv2", 64, rows), (2, "model.23.cv4", 32, cfrows)):
        if not (mode & bit):
            continue
        dense = torch.cat([de.read_tensor(de.find_tensor(f"{pre}.{l}.2")).reshape(B, -1, width) for l in range(3)], 1)
        want = dense[bi, sel[:, :k].long()]
        d = (got_rows[:, :k] - want).abs()
        rng = float(want.abs().max())
        print(pre, "winners vs dense: max", float(d.max()), "of range", rng, "; fraction beyond 1e-3 of the range", float((d > 1e-3 * rng).float().mean()))
        assert float(d.max()) <= 0.05 * rng and float((d > 1e-3 * rng).float().mean()) < 0.02
    on_border = 0
    for b in range(B):
        for a in sel[b, :k].tolist():
            off = 0
            for l, s in enumerate((8, 16, 32)):
                h, w = shape[1] // s, shape[2] // s
                if a < off + h * w:
                    y, x = divmod(a - off, w)
                    on_border += int(y in (0, h - 1) or x in (0, w - 1))
                    break
                off += h * w
    print("winners on a frame border:", on_border)
    assert on_border > 0 or shape[1] > 256          # (the small maps always put winners on the border; a 60x76 P3 map need not)
    assert float((out_s["det"][..., :4] - out_d["det"][..., :4]).abs().max()) < 2.0       # (px; a 0.2 % logit difference on a stride-32 winner is 0.6 px)
    if seg:
        assert float((out_s["coeff"] - out_d["coeff"]).abs().max()) <= 0.05 * float(out_d["coeff"].abs().max()) + 1e-6
    de.close()


def test_topk_adversarial():
    """Ties through a whole forward: an engine whose class head is constant (all scores equal) -> ordering must be anchor-index then
    class ascending, with fewer anchors than max_det. Crafted logits - tie groups across a cut, saturated scores, two stage-2 rounds -
    are written over a real engine's head tensors in tests/test_gpu_head_crafted.py."""
    from oracle.yolov10_oracle import Oracle
    st, im = make_case("n", 80, False, 0, (1, 64, 64))
    for l in range(3):
        st[f"model.23.one2one_cv3.{l}.2.weight"].zero_()        # every class logit == bias == -3.0: 84*80 exact ties
    ref = Oracle(st, "n", 80, False, "fp32").forward(im)
    eng = _engine("n", 80, False, "fp32", st)
    out = eng.forward(im.cuda())
    torch.cuda.synchronize()
    k = ref["det"].shape[1]
    assert torch.equal(out["idx"].cpu()[:, :k].long(), ref["idx"])
    assert torch.equal(out["det"].cpu()[:, :k, 5], ref["det"][..., 5])
    assert float((out["det"].cpu()[:, :k, 4] - ref["det"][..., 4]).abs().max()) < 1e-6
    # fewer anchors (84) than max_det: the remaining rows are zero / -1
    assert k == 84 and bool((out["idx"].cpu()[:, k:] == -1).all()) and float(out["det"].cpu()[:, k:].abs().max()) == 0.0
    eng.close()


def test_graph_replay_matches_eager():
    """hipGraph replay (with the concurrent head-branch lanes derived from tensor dependencies) must reproduce the
    eager op-by-op result bit for bit, call after call."""
    st, im = make_case("s", 80, True, 0, (3, 160, 192))
    eng = _engine("s", 80, True, "bf16", st)
    imc = im.cuda()
    ref = {k: v.clone() for k, v in eng.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    eng.set_graph(True)
    for _ in range(3):
        out = eng.forward(imc)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    eng.close()


def _poison_everything(eng):
    """Fill every engine tensor with bit patterns that read as bf16 NaN: bf16 tensors get NaN, fp32 tensors a finite float
    (bits 0x3F80FFFF) whose LOW half - the first two bytes in memory, what a bf16 over-read of it sees - is 0xFFFF."""
    bad32 = torch.tensor([0x3F80FFFF], dtype=torch.int32).view(torch.float32).item()
    for t in eng.tensors():
        fill = bad32 if t["f32"] else float("nan")
        eng.write_tensor(t["index"], 0, torch.full(t["shape"], fill, dtype=torch.float32))


@pytest.mark.parametrize("family,variant,seg", [("v10", "x", False), ("v8", "m", True), ("v10", "x", True)])
def test_padded_tap_overread_reads_zeroed_tail(family, variant, seg):
    """Dense convs on 48- / 80-channel inputs run with padded taps (WeightDesc::cin_pad): at the last pixel of the last image they read up
    to 32 bytes past their input tensor, times zero weights - NaN bit patterns there would poison the bottom-right anchor (NaN * 0 = NaN
    on the matrix cores). Every such tensor owns a tail that allocate_plan zeroes on EVERY layout. The test plans a large shape, fills the
    whole arena's tensors with bf16-NaN patterns, re-plans a smaller shape into the kept arena (so tensors land on stale bytes, fp32 logits
    right behind bf16 activations) and requires every padded-tap conv's output - last pixel of the last image included - to be finite."""
    from yolo_puncture_amd.engine import Engine
    if family == "v10":
        st, im = make_case(variant, 80, seg, 0, (1, 64, 64))
        eng = Engine(variant, 80, seg, "bf16", 0, state=st)
    else:
        from helpers import make_case_family
        st, im = make_case_family(family, variant, 80, 0, (1, 64, 64))
        eng = Engine(variant, 80, True, "bf16", 0, state=st, family=family)
    eng.set_autotune(False)
    big = torch.zeros((2, 96, 128, 3), dtype=torch.uint8).cuda()
    eng.forward(big)
    torch.cuda.synchronize()
    _poison_everything(eng)
    imc = im.cuda()
    out = eng.forward(imc)                      # re-plan into the kept (poisoned) arena
    torch.cuda.synchronize()
    ops = eng.plan(1, 64, 64)
    padded = [(i, o) for i, o in enumerate(ops) if o["kind"] == "conv" and o["c_read"] > o["in"][2] and o["kernel"] != "-"]
    assert padded, "this model should have padded-tap convs"
    assert bool(torch.isfinite(out["det"]).all())
    for i, o in padded:
        t, c0, cc = o["out"]
        y = eng.read_tensor(t)[..., c0:c0 + cc]
        assert bool(torch.isfinite(y).all()), (o["name"], o["in"], o["c_read"])
        assert bool(torch.isfinite(y[-1, -1, -1]).all())
    # and directly: poison again (tails included? no - write_tensor only touches payloads), run each padded op alone, check again
    _poison_everything(eng)
    for i, o in padded:
        ti, ci, cin = o["in"]
        shp = eng.tensors()[ti]["shape"]
        eng.write_tensor(ti, 0, torch.zeros(shp))            # a finite input; everything else (the NEXT tensor included) stays poisoned
        eng.run_op(i, imc, out)
        t, c0, cc = o["out"]
        y = eng.read_tensor(t)[..., c0:c0 + cc]
        assert bool(torch.isfinite(y).all()), (o["name"], "next tensor poisoned")
    eng.close()


def test_tuning_export_import_reproduces_bits():
    """bf16 results depend on the conv tile configurations in the last bit (fp32 summation order). An engine that IMPORTS another engine's
    configurations (what parallel.sync_tuning does between ranks, include/yolop.h yp_tuning_*) must reproduce its outputs bit for bit, whatever
    its own tuner would have picked; an id that is not launchable for its layer is refused."""
    from yolo_puncture_amd.engine import YolopError
    shape = (3, 160, 192)
    st, im = make_case("s", 80, True, 0, shape)
    imc = im.cuda()
    a = _engine("s", 80, True, "bf16", st)
    ref = {k: v.clone() for k, v in a.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    cfgs = a.tuning_export()
    ops = a.plan(*shape)
    assert len(cfgs) == len(ops) and any(c >= 100 for c in cfgs)
    logits_a = a.read_tensor(a.find_tensor("model.23.one2one_cv3.0.2"))
    a.close()
    b = _engine("s", 80, True, "bf16", st)
    b.set_autotune(False)                                    # b's own choice would be the heuristic: different kernels for many layers
    b.tuning_import(*shape, cfgs)
    out = b.forward(imc)
    torch.cuda.synchronize()
    assert b.tuning_export() == cfgs
    assert [o["kernel"] for o in b.plan(*shape)] == [o["kernel"] for o in ops]
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(b.read_tensor(b.find_tensor("model.23.one2one_cv3.0.2")), logits_a)
    bad = list(cfgs)
    j = next(i for i, c in enumerate(cfgs) if 300 <= c < 500 or 600 <= c < 900)      # a plain (never fused) tunable conv
    bad[j] = 999                                             # conv_ks id beyond its table
    with pytest.raises(YolopError):
        b.tuning_import(*shape, bad)
    b.close()


def test_forward_reads_only_its_own_frames():
    """Two forwards on different frames: the second equals a fresh engine's forward on its frames, bit for bit. A fused pair whose
    stored intermediate has a reader between the pair's two ops (v10-S at small shapes: model.19.cv2 -> one2one_cv3.1.0.0 past the
    SCDown model.20) would hand that reader the previous forward's values."""
    from helpers import rand_image
    from yolo_puncture_amd.engine import Engine
    st, im_a = make_case("s", 80, False, 0, (2, 96, 128))
    im_b = rand_image(tuple(im_a.shape), seed=7)
    outs = []
    for frames in ((im_a, im_b), (im_b,)):
        eng = Engine("s", 80, False, "bf16", 0, state=st)
        eng.set_autotune(False)
        for im in frames:
            out = eng.forward(im.cuda())
        torch.cuda.synchronize()
        outs.append({k: out[k].cpu().clone() for k in ("det", "idx")})
        eng.close()
    assert torch.equal(outs[0]["idx"], outs[1]["idx"]) and torch.equal(outs[0]["det"], outs[1]["det"])
