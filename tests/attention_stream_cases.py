"""Stand-alone cases of the streaming attention kernel (csrc/attention_stream.hip), shared by test_attention_stream_host.py (CPU: the
reference pair alone) and test_gpu_attention_stream.py (the kernel, through yp_debug_attention_form). Inputs, reference and bounds are
those of attention_ref.py.

The kernel's sizes: it streams keys in blocks of KEY_BLOCK, a workgroup walks query groups of QUERY_GROUP rows, a wave owns 32 of them as
two 16-row tiles, and the launcher hands the form over above RESIDENT_TOKENS. N = 511, 512, 513 lie on both sides of a key block and of a
query group (4 x 128), 401 is the first N the form takes, 641 and 1025 leave a ragged last block of 1 key, 2368 / 2369 are the generic
kernel's last N and the first it refuses, 3680 is 2560 x 1472."""
import attention_ref as A

KEY_BLOCK = 128
QUERY_GROUP = 128
RESIDENT_TOKENS = 400
STREAM, MFMA, GENERIC = 2, 1, 0

# (B, N, nh, kd, hd, dist)
CASES = ([(2, n, 2, 32, 64, d) for n in (401, 511, 512, 513, 641, 1025) for d in A.DISTS] +
         [(1, n, 2, 32, 64, d) for n in (2368, 2369) for d in ("flat", "peaked", "shifted")] +
         [(1, 3680, 1, 32, 64, d) for d in ("flat", "peaked", "shifted")])
assert any(n % KEY_BLOCK == KEY_BLOCK - 1 for _, n, *_ in CASES) and any(n % KEY_BLOCK == 0 for _, n, *_ in CASES) and \
    any(n % KEY_BLOCK == 1 for _, n, *_ in CASES) and KEY_BLOCK % QUERY_GROUP == 0, "the cases straddle a key block and a query group"


def groups_per_workgroup(B, N, nh, wgs=0):
    """the launcher's split (attention_stream_split): (workgroups per head, query groups each walks)"""
    target = wgs if wgs > 0 else 256
    ngroups, BH = (N + QUERY_GROUP - 1) // QUERY_GROUP, B * nh
    nsplit = min(ngroups, max(1, (target + BH - 1) // BH))
    gpw = (ngroups + nsplit - 1) // nsplit
    return (ngroups + gpw - 1) // gpw, gpw
