"""Every device helper of the kernels is defined once (host-only source check).

csrc/kernel_util.h holds the primitives that more than one kernel file uses. This test reads the kernel sources and fails when a
namespace-scope `__device__ __forceinline__` function has the same body in two files, or when the text of the vmcnt encoder or of the
XCD block-id remap turns up in more than one file: the copy belongs in kernel_util.h instead.
"""
import re
from collections import defaultdict
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "yolo-puncture_amd" / "csrc"

# (file name, function name) pairs that may repeat a body found elsewhere. Every entry needs a comment saying why.
EXEMPT = set()
# files besides kernel_util.h that may write a single-definition text out. Every entry needs a comment saying why.
TEXT_EXEMPT = {
    # The device assembly of these two kernels must not change, and through xcd_remap() it does: the helper is optimised on its own before it
    # is inlined, `bid >> 3` moves behind the select, and the kernels' scalar register allocation comes out different (no other kernel's does).
    "xcd < r ?": {"conv_dma_p.hip", "conv_wreg.hip"},
}

_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
_SCOPE = re.compile(r'(?:namespace\s*\w*|extern\s*"C")\s*$')       # braces that open a scope, not a definition
_MARK = "__device__ __forceinline__"


def _sources():
    files = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h"))
    assert len(files) > 30, f"kernel sources not found under {CSRC}"
    return {f.name: _COMMENT.sub(" ", f.read_text()) for f in files}


def _match_brace(text, i):
    depth = 0
    for j in range(i, len(text)):
        if text[j] == "{":
            depth += 1
        elif text[j] == "}":
            depth -= 1
            if depth == 0:
                return j
    raise AssertionError("unbalanced braces")


def _norm(s):
    return " ".join(s.split())


def device_functions(text):
    """(name, template line, signature, body) of each namespace-scope __device__ __forceinline__ definition in comment-free text."""
    out = []
    i, start = 0, 0                     # start: end of the previous namespace-scope item
    while True:
        j = text.find("{", i)
        if j < 0:
            return out
        head = text[start:j]
        if _SCOPE.search(head):         # namespace yp { ... : look inside
            i = start = j + 1
            continue
        end = _match_brace(text, j)     # a definition (function, struct, initialiser): skip it whole
        k = head.rfind(_MARK)
        if k >= 0 and ";" not in head[k:] and "(" in head[k:]:
            sig = _norm(head[k + len(_MARK):])
            tmpl = re.search(r"(template\s*<[^{};]*>)\s*(?:static\s+)?$", head[:k])
            name = re.search(r"([\w:]+(?:\s*<[^()]*>)?)\s*\(", sig).group(1)
            out.append((name, _norm(tmpl.group(1)) if tmpl else "", sig, _norm(text[j:end + 1])))
        i = start = end + 1


def test_device_functions_are_found():
    src = _sources()
    names = {n for n, _, _, _ in device_functions(src["kernel_util.h"])}
    assert {"wait_vmcnt", "xcd_remap", "swz64", "silu4_packed"} <= names, names
    # members of a struct are not namespace scope
    assert "is_cand" not in {n for n, _, _, _ in device_functions(src["contour_large.hip"])}


def test_no_device_helper_is_defined_twice():
    by_body = defaultdict(list)
    for fname, text in _sources().items():
        for name, tmpl, sig, body in device_functions(text):
            if (fname, name) not in EXEMPT:
                by_body[body].append((fname, name))
    copies = {b: sorted(w) for b, w in by_body.items() if len({f for f, _ in w}) > 1}
    assert not copies, "the same device helper body in more than one file (move it to kernel_util.h):\n" + "\n".join(
        f"  {w}: {b[:100]}" for b, w in sorted(copies.items(), key=lambda kv: kv[1]))


def test_vmcnt_encoder_and_xcd_remap_occur_once():
    src = _sources()
    for needle in ("((N >> 4) & 3) << 14", "xcd < r ?"):
        holders = {f for f, t in src.items() if _norm(needle) in _norm(t)}
        assert holders == {"kernel_util.h"} | TEXT_EXEMPT.get(needle, set()), f"`{needle}` is written out in {sorted(holders)}"
