"""The kernel name a plan reports for a dense conv, a depthwise conv or the stem (yp_op_kernel: bench, profiles and rocprof joins use it)
is a kernel symbol that libyolop.so really contains: every conv family, launch_dwconv and launch_stem build it from the template instance
the launcher picks. No GPU needed."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from yolo_puncture_amd.engine import Engine, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"
NM = shutil.which("llvm-nm", path=LLVM) or shutil.which("nm")
CXXFILT = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")


def _kernel_symbols(lib_path):
    # the host stubs HIP registers for every __global__ instance: "void yp::conv_wres_kernel<64, 2, false>(yp::ConvParams, ...)"
    mangled = [ln.split()[-1] for ln in subprocess.run([NM, "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout.splitlines()
               if ln.split() and ln.split()[-1].startswith("_ZN2yp")]
    # (binutils' c++filt does not know the mangling of __bf16, "DF16b", and would leave those instances mangled: spell it as a vendor type)
    mangled = [m.replace("DF16b", "u6__bf16") for m in mangled]
    out = subprocess.run([CXXFILT], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    syms = set()
    for d in out:
        d = d.replace(" ", "")
        if d.startswith("void"):
            d = d[4:]
        d = d.split("(")[0].replace("yp::", "")
        syms.add(d)
        syms.add(d.replace("<__bf16", "<bf16").replace("<float", "<f32"))      # the element type as dwconv_kernel_name / stem_kernel_name spell it
    return syms


@pytest.mark.skipif(NM is None or CXXFILT is None, reason="no nm / c++filt on this machine")
def test_packaged_table_conv_names_are_kernel_symbols(monkeypatch):
    monkeypatch.delenv("YOLOP_TUNE_CACHE", raising=False)
    lib = load_library()
    syms = _kernel_symbols(lib._name)
    files = sorted(glob.glob(os.path.join(ROOT, "yolo-puncture_amd", "tune_tables", "tt_*.txt")))
    assert files, "no packaged tune tables"
    checked = set()
    try:
        for f in files:
            m = re.match(r"tt_f0(\w)(det|seg)_nc(\d+)_dt0_(\d+)x(\d+)x(\d+)_t\d+\.txt$", os.path.basename(f))
            v, task, nc, B, H, W = m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))
            table = {ln.split()[0]: int(ln.split()[1]) for ln in open(f) if ln.strip()}
            e = Engine(v, nc, task == "seg", "bf16", 0)
            # each id of the table forced in turn: the ops the table gives that id report what the table's plan reports for them
            for cfg in sorted(set(table.values())):
                lib.yp_debug_force_conv_cfg(cfg)
                e.plan(1, 64, 64)                      # (a plan of the same shape is kept as it is: re-plan from scratch)
                for o in e.plan(B, H, W):
                    k = o["kernel"]
                    if k.startswith(("dwconv_", "stem_")):          # named by their launchers, whatever id is forced
                        assert k.replace(" ", "") in syms, (os.path.basename(f), o["name"], k)
                        checked.add(k.split("<")[0])
                        continue
                    if table.get(o["name"]) != cfg or not k.startswith("conv_") or k.startswith(("conv_igemm", "conv_dwpw")):
                        continue
                    assert k.replace(" ", "") in syms, (os.path.basename(f), o["name"], cfg, k)
                    checked.add(k.split("<")[0])
            e.close()
    finally:
        lib.yp_debug_force_conv_cfg(-1)
    assert {"conv_dma_p_kernel", "conv_dma_lc_kernel", "conv_halo_s2_kernel", "conv_tile1_kernel", "conv_wres_kernel", "dwconv_row_kernel",
            "stem_mfma_kernel"} <= checked, checked
