"""YOLOv10 engines on inputs beyond 12288 anchors: the head's stage 1 runs as head_chunk_topk_kernel + head_select_large_kernel
(head_large.hip). Shapes: 800x768 (12600 anchors: a second chunk of 312), 832x736 (12558: a second chunk of 270, fewer than k = 300),
1280x960 (25200: three chunks; 1200 attention tokens, so the PSA block runs the generic attention kernel)."""
import pytest
import torch

from helpers import assert_within_noise_floor, make_case

pytestmark = pytest.mark.gpu


def _engine(variant, nc, seg, dtype, st):
    from yolo_puncture_amd.engine import Engine
    e = Engine(variant, nc, seg, dtype, 0, state=st)
    e.set_autotune(False)
    return e


def _two_stage_topk(logits, k):
    """v10postprocess restated on [B, A, nc] class logits with the ordering rule of SURVEY 7.2 (score descending, flat index ascending, in
    both stages) -> anchors [B, k], classes [B, k], scores [B, k]"""
    B, A, nc = logits.shape
    s = torch.sigmoid(logits)
    m = s.max(2).values
    key1 = (m.view(torch.int32).long() << 32) | (0xFFFFFFFF - torch.arange(A, dtype=torch.int64))[None]
    a1 = 0xFFFFFFFF - (torch.sort(key1, dim=1, descending=True).values[:, :k] & 0xFFFFFFFF)          # stage-1 winners by rank
    cand = s[torch.arange(B)[:, None], a1].reshape(B, k * nc)
    key2 = (cand.view(torch.int32).long() << 32) | (0xFFFFFFFF - torch.arange(k * nc, dtype=torch.int64))[None]
    top = torch.sort(key2, dim=1, descending=True).values[:, :k]
    flat = 0xFFFFFFFF - (top & 0xFFFFFFFF)
    return a1.gather(1, flat // nc), flat % nc, (top >> 32).int().view(torch.float32)


@pytest.mark.parametrize("variant,seg,shape", [("n", False, (1, 800, 768)), ("n", True, (2, 832, 736)), ("s", False, (1, 1280, 960))])
def test_large_head_bf16(variant, seg, shape, monkeypatch):
    """(a) idx / classes / scores are the two-stage top-k of the engine's own dense class logits, restated on the host (anchor and class
    identical on every row whose score is no float near-tie (1e-6) with a neighbour's - the host's sigmoid may round the last bit differently -
    scores within 1e-6); (b) hipGraph replay == eager, bit for bit; (c) the winners-only head equals the dense head as
    test_winners_only_head_equals_dense asserts it for the small form."""
    st, im = make_case(variant, 80, seg, 0, shape)
    imc = im.cuda()
    B = shape[0]
    A_l = [(shape[1] // s) * (shape[2] // s) for s in (8, 16, 32)]
    assert sum(A_l) > 12288
    sp = _engine(variant, 80, seg, "bf16", st)
    head = sp.plan(*shape)[-1]["kernel"]
    assert "head_chunk_topk_kernel + head_select_large_kernel<1>" in head, head
    ref = {k_: v.clone() for k_, v in sp.forward(imc).items() if v is not None}
    torch.cuda.synchronize()
    out_s = {k_: v.cpu() for k_, v in ref.items()}
    mode, sel, rows, cfrows = sp.head_winners(B)
    assert mode & 1
    k = sp.max_det
    logits = torch.cat([sp.read_tensor(sp.find_tensor(f"model.23.one2one_cv3.{l}.2")).reshape(B, -1, 80) for l in range(3)], 1)
    wa, wc, ws = _two_stage_topk(logits, k)
    # same logits on both sides: only the last bits of the two sigmoids differ (each within a few ulp, 6e-8 apiece below 1.0), so rows whose
    # score is more than 1e-6 from both neighbours have the same rank on the host and on the device
    gap = (ws[:, :-1] - ws[:, 1:]).abs()
    safe = torch.ones_like(ws, dtype=torch.bool)
    safe[:, 1:] &= gap > 1e-6
    safe[:, :-1] &= gap > 1e-6
    print(variant, shape, "rows with a clear score gap:", float(safe.float().mean()))
    assert bool(safe.any())
    assert torch.equal(out_s["idx"].long()[safe], wa[safe]) and torch.equal(out_s["det"][..., 5][safe], wc.float()[safe])
    assert float((out_s["det"][..., 4] - ws).abs().max()) < 1e-6
    # and on every row, near-ties included: the row's score is the score of its (anchor, class), rows are best first and distinct, and
    # every (anchor, class) of the image that beats the last row by more than the sigmoids' rounding is among the rows
    sflat = torch.sigmoid(logits).reshape(B, -1)
    pairs = out_s["idx"].long() * 80 + out_s["det"][..., 5].long()
    assert float((sflat.gather(1, pairs) - out_s["det"][..., 4]).abs().max()) < 1e-6
    assert bool((out_s["det"][:, :-1, 4] >= out_s["det"][:, 1:, 4]).all())
    for b in range(B):
        assert pairs[b].unique().numel() == k
        must = torch.nonzero(sflat[b] > out_s["det"][b, -1, 4] + 1e-6).flatten()
        assert must.numel() < k and bool(torch.isin(must, pairs[b]).all())
    assert int(wa.max()) >= 12288, "no winner in a later chunk: the case does not exercise the merge"
    # (b)
    sp.set_graph(True)
    for _ in range(2):
        out = sp.forward(imc)
        torch.cuda.synchronize()
        for k_ in ref:
            assert torch.equal(out[k_], ref[k_]), k_
    sp.close()
    # (c)
    monkeypatch.setenv("YOLOP_DENSE_HEAD", "1")
    de = _engine(variant, 80, seg, "bf16", st)
    assert de.plan(*shape)[-1]["kernel"] == "head_chunk_topk_kernel + head_select_large_kernel<0>"
    out_d = {k_: v.cpu() for k_, v in de.forward(imc).items() if v is not None}
    assert de.head_winners(B)[0] == 0
    assert torch.equal(out_s["idx"], out_d["idx"]) and torch.equal(out_s["det"][..., 4:], out_d["det"][..., 4:])
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
    de.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_large_head_all_ties(dtype):
    """Every class logit equal (class weights zeroed: logit == bias == -3 in any storage type): 12600 * 80 exact ties, so winner r is
    anchor r // 80 with class r % 80 - the tie rule must survive the chunk pass and the merge."""
    st, im = make_case("n", 80, False, 0, (1, 800, 768))
    for l in range(3):
        st[f"model.23.one2one_cv3.{l}.2.weight"].zero_()
    eng = _engine("n", 80, False, dtype, st)
    out = {k_: v.cpu() for k_, v in eng.forward(im.cuda()).items() if v is not None}
    k = eng.max_det
    r = torch.arange(k)
    assert torch.equal(out["idx"][0].long(), r // 80) and torch.equal(out["det"][0, :, 5], (r % 80).float())
    assert float((out["det"][0, :, 4] - torch.sigmoid(torch.tensor(-3.0))).abs().max()) < 1e-6
    eng.close()


def test_large_head_fp32_against_oracle():
    """fp32 engine vs the oracle at 800x768, as test_end_to_end_fp32 holds the small form."""
    from oracle.yolov10_oracle import Oracle
    shape = (1, 800, 768)
    st, im = make_case("n", 80, False, 0, shape)
    ref = Oracle(st, "n", 80, False, "fp32").forward(im)
    ref64 = Oracle(st, "n", 80, False, "fp64").forward(im)
    eng = _engine("n", 80, False, "fp32", st)
    res = {k_: v.cpu() for k_, v in eng.forward(im.cuda()).items() if v is not None}
    eng.close()
    k = ref["det"].shape[1]
    s = ref["det"][..., 4]
    gap = (s[:, :-1] - s[:, 1:]).abs()
    safe = torch.ones_like(s, dtype=torch.bool)
    safe[:, 1:] &= gap > 1e-5
    safe[:, :-1] &= gap > 1e-5
    idx_ok = (res["idx"][:, :k].long() == ref["idx"]) & (res["det"][:, :k, 5] == ref["det"][..., 5])
    assert bool(idx_ok[safe].all()), "index/class mismatch on a row with a clear score gap"
    assert safe.float().mean() > 0.5
    same = idx_ok & (ref64["idx"] == ref["idx"]) & (ref64["det"][..., 5].float() == ref["det"][..., 5])
    assert same.float().mean() > 0.9, float(same.float().mean())
    det = res["det"][:, :k]
    assert_within_noise_floor("boxes [px]", det[..., :4][same], ref["det"][..., :4][same], ref64["det"][..., :4][same], 1e-3)
    assert_within_noise_floor("scores", det[..., 4][same], ref["det"][..., 4][same], ref64["det"][..., 4][same], 1e-3, ceiling=1e-4)
