"""Stand-alone cases of the wide-head streaming attention kernel (csrc/attention_stream_wide.hip: bf16, key_dim 36, head_dim 72, YOLOv10-M's
PSA block), shared by test_attention_wide_host.py (CPU: the reference pair alone) and test_gpu_attention_wide.py (the kernel, through
yp_debug_attention_form under the form "stream_wide"). Inputs, reference and bounds are those of attention_ref.py.

The kernel's sizes are attention_stream_kernel's: keys in blocks of KEY_BLOCK, query groups of QUERY_GROUP rows, so the launcher's split is
attention_stream_cases.groups_per_workgroup. There is no resident sibling: the kernel takes every N >= 1. N = 127, 128, 129 lie on both
sides of a key block and of a query group, 1 and 17 leave one ragged block (one and two query tiles), 400 / 401 is where the 32/64 forms
switch (the wide kernel must not care), 513 leaves a last block of 1 key, 2364 / 2365 are the generic kernel's last N and its first refusal
at key_dim 36, 3680 is 2560 x 1472."""
import attention_ref as A
from attention_stream_cases import GENERIC, KEY_BLOCK, MFMA, QUERY_GROUP, STREAM, groups_per_workgroup  # noqa: F401

KD, HD = 36, 72
WIDE = 3                   # kernel_out of attention_stream_wide_kernel
GENERIC_TOKENS = 2364      # (150 KB / 4 - 16 * 36) / 16: the generic kernel's bound at key_dim 36

# (B, N, nh, kd, hd, dist)
CASES = ([(2, n, 2, KD, HD, d) for n in (1, 17, 127, 128, 129, 400, 401, 513) for d in A.DISTS] +
         [(1, n, 4, KD, HD, d) for n in (2364, 2365) for d in ("flat", "peaked", "shifted")] +
         [(1, 3680, 1, KD, HD, d) for d in ("flat", "peaked", "shifted")])
assert any(n % KEY_BLOCK == KEY_BLOCK - 1 for _, n, *_ in CASES) and any(n % KEY_BLOCK == 0 for _, n, *_ in CASES) and \
    any(n % KEY_BLOCK == 1 for _, n, *_ in CASES) and KEY_BLOCK % QUERY_GROUP == 0, "the cases straddle a key block and a query group"
