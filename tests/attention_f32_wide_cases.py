"""Stand-alone cases of the fp32 streaming attention kernel for 36/72 heads (csrc/attention_stream_wide_f32.hip) and a CPU restatement of
its block and summation order, shared by test_attention_f32_wide_host.py (CPU: the restatement against the contract) and
test_gpu_attention_f32_wide.py (the kernel, through yp_debug_attention_f32 under switch value 3). Inputs, reference and the bound are
attention_ref.py's: helpers.assert_within_noise_floor(got, o32, o64, F32_TARGET) - at most twice the error torch's own float32 expression
makes on the case.

The kernel's sizes: keys stream in blocks of KEY_BLOCK, a workgroup walks query groups of QUERY_GROUP rows (4 waves x one 16-row tile),
the launcher hands the call over above RESIDENT_TOKENS when the engine's switch has the wide bit. 511, 512, 513 lie on both sides of a key
block (8 x 64) and of a query group (8 x 64), 401 is the first N the kernel takes, 641 and 1025 leave a last block of one key, 2364 / 2365
are the generic kernel's last N with 36-wide keys and the first it refuses, 3680 is 2560 x 1472.

`emulate` follows the kernel step by step in float32 (a fused multiply-add is a float64 product and sum rounded once to float32; exp(x) is
the kernel's exp2(x * log2 e) with the product rounded to float32 and the hardware's exp2 taken as correctly rounded: it is within an ulp):
  S      per (query, key) 36 FMAs in nine matrix-core steps of four. Lane group g holds d = 8 g .. 8 g + 7 and d = 32 + g of its row:
         step s = 0..7 takes, in order, d = 8 g + s for g = 0..3, step 8 takes d = 32 + g. ORDER says how the steps chain:
           "4x8+1"  steps 2 c, 2 c + 1 form chain c of four and step 8 a fifth chain of its own: ((c0 + c1) + (c2 + c3)) + c4 (the kernel's)
           "8,8,8,12"  step 8 continues chain 3: (c0 + c1) + (c2 + c3)
           "4x9"    chain c is d = 9 c .. 9 c + 8, (c0 + c1) + (c2 + c3): what four even chains would be; no whole number of matrix-core
                    steps, emulated for the comparison only
         The scale multiplies the finished sum.
  pass 1 lane group g of a query row owns keys 4 g .. 4 g + 3 of every 16-key tile. Per key block: the max of its 16 keys, then
         l = l * exp(m - m') + sum of exp(s - m') over those keys in tile order; the four groups merge once behind the last block,
         (s0 + s1) + (s2 + s3) after rescaling to the common max.
  pass 2 p = exp(s - m) * (1 / l); every key block accumulates P.V in a fresh accumulator, one FMA per key and output column in the order
         tile j, step r = 0..3, group g = 0..3 -> key 16 j + 4 g + r, and the block's sum is added to the row's total: chains of 64 and
         of N / 64 additions, never one of N. The 72 columns are five 16-column tiles whose last eight columns are fed zeros and never
         stored: they do not exist here."""
import torch

import attention_ref as A

KD, HD = 36, 72
KEY_BLOCK = 64
QUERY_GROUP = 64
RESIDENT_TOKENS = 400
DEFAULT_WGS = 1024            # the launcher's workgroup target without wgs / YOLOP_ATTN_WGS
STREAM_WIDE_F32, STREAM_F32, GENERIC = 5, 4, 0
ORDERS = ("4x8+1", "8,8,8,12", "4x9")
ORDER = "4x8+1"               # the kernel's

ALL_DISTS = ("flat", "peaked", "shifted")
# (B, N, nh, kd, hd, dist): the GPU contract cases
CASES = ([(2, n, 2, KD, HD, d) for n in (401, 511, 512, 513, 641) for d in ALL_DISTS] +
         [(1, n, 4, KD, HD, d) for n in (1025, 2364, 2365) for d in ALL_DISTS] +
         [(1, 3680, 4, KD, HD, d) for d in ("peaked", "shifted")])
# the emulation's cases (host test)
EMULATION_CASES = [(1, n, 2, KD, HD, d) for n in (401, 513, 2365, 3680) for d in ALL_DISTS]
assert any(n % KEY_BLOCK == KEY_BLOCK - 1 for _, n, *_ in CASES) and any(n % KEY_BLOCK == 0 for _, n, *_ in CASES) and \
    any(n % KEY_BLOCK == 1 for _, n, *_ in CASES) and any(n % QUERY_GROUP == 0 for _, n, *_ in CASES) and \
    any(n % QUERY_GROUP == 1 for _, n, *_ in CASES), "the cases straddle a key block and a query group"

# (B, N, nh) of tools/attention_f32_latency.py --heads wide; the first is the gated one
LATENCY_CASES = ((8, 1600, 4), (4, 2040, 4), (1, 920, 4), (1, 3680, 4), (1, 8160, 4))


def groups_per_workgroup(B, N, nh, wgs=0):
    """the launcher's split (attention_stream_f32_split's rule): (workgroups per head, query groups each walks)"""
    target = wgs if wgs > 0 else DEFAULT_WGS
    ngroups, BH = (N + QUERY_GROUP - 1) // QUERY_GROUP, B * nh
    nsplit = min(ngroups, max(1, (target + BH - 1) // BH))
    gpw = (ngroups + nsplit - 1) // nsplit
    return (ngroups + gpw - 1) // gpw, gpw


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


LOG2E = torch.tensor(1.44269504088896341, dtype=torch.float32)


def _exp(x):
    return torch.exp2((x * LOG2E).double()).float()


def score_chains(order=ORDER):
    """the key dimensions of every FMA chain of a score, in the order they are added"""
    steps = [[8 * g + s for g in range(4)] for s in range(8)] + [[32 + g for g in range(4)]]
    if order == "4x8+1":
        return [steps[2 * c] + steps[2 * c + 1] for c in range(4)] + [steps[8]]
    if order == "8,8,8,12":
        return [steps[2 * c] + steps[2 * c + 1] for c in range(3)] + [steps[6] + steps[7] + steps[8]]
    if order == "4x9":
        return [list(range(9 * c, 9 * c + 9)) for c in range(4)]
    raise ValueError(order)


def emulate(qkv, nh=2, kd=KD, hd=HD, order=ORDER):
    """qkv float32 [B, N, nh * (2 kd + hd)] -> o float32 [B, N, nh * hd] in the kernel's order (module docstring)"""
    assert qkv.dtype == torch.float32 and kd == KD and hd == HD
    B, N, _ = qkv.shape
    KB = KEY_BLOCK
    nkb = (N + KB - 1) // KB
    NP = nkb * KB
    scale = torch.tensor(1.0 / (kd ** 0.5), dtype=torch.float32)
    out = torch.empty(B, N, nh, hd, dtype=torch.float32)
    x = qkv.reshape(B, N, nh, 2 * kd + hd)
    chains = score_chains(order)
    assert sorted(d for c in chains for d in c) == list(range(kd))
    for b in range(B):
        for h in range(nh):
            q, k, v = x[b, :, h, :kd], x[b, :, h, kd:2 * kd], x[b, :, h, 2 * kd:]
            kp = torch.zeros(NP, kd)
            kp[:N] = k
            vp = torch.zeros(NP, hd)
            vp[:N] = v                                                    # absent keys are fetched as zeros
            part = []
            for chain in chains:
                s = torch.zeros(N, NP)
                for d in chain:
                    s = _fma(q[:, d:d + 1], kp[:, d][None, :], s)
                part.append(s)
            s = (part[0] + part[1]) + (part[2] + part[3])
            if len(part) == 5:
                s = s + part[4]
            s = s * scale
            s[:, N:] = float("-inf")
            # pass 1: s5[n, block, tile, g, r]
            s5 = s.reshape(N, nkb, KB // 16, 4, 4)
            m = torch.full((N, 4), -3.0e38)
            l = torch.zeros(N, 4)
            for kb in range(nkb):
                blk = s5[:, kb]                                           # [N, tiles, g, r]
                mn = torch.maximum(m, blk.amax(dim=(1, 3)))
                e = _exp(blk - mn[:, None, :, None])
                acc = torch.zeros(N, 4)
                for j in range(KB // 16):
                    for r in range(4):
                        acc = acc + e[:, j, :, r]
                l = l * _exp(m - mn) + acc
                m = mn
            mm = m.amax(dim=1, keepdim=True)
            sg = l * _exp(m - mm)
            tot = (sg[:, 0] + sg[:, 1]) + (sg[:, 2] + sg[:, 3])
            inv = (1.0 / tot)[:, None]
            p = _exp(s - mm) * inv                                   # [N, NP]
            # pass 2: all blocks side by side, 64 sequential FMAs each, then the blocks in order
            p4 = p.reshape(N, nkb, KB)
            v4 = vp.reshape(nkb, KB, hd)
            ob = torch.zeros(N, nkb, hd)
            for j in range(KB // 16):
                for r in range(4):
                    for g in range(4):
                        key = 16 * j + 4 * g + r
                        ob = _fma(p4[:, :, key, None], v4[None, :, key, :], ob)
            o = torch.zeros(N, hd)
            for kb in range(nkb):
                o = o + ob[:, kb]
            out[b, :, h] = o
    return out.reshape(B, N, nh * hd)


def case_id(c):
    return A.case_id(c)
