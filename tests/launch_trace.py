"""Builds the host-dispatch trace tools of tools/ (gn_launch_trace.cpp, conv_launch_trace.cpp) against the tree's csrc/ without a GPU; used by
tests/test_host_logic.py and tests/test_host_conv_ref.py."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TRACE_TOOLS = {}


def build(tool, sources):
    """tools/<tool>.cpp built against the tree's csrc/<sources>.hip (host objects + tools/launch_trace_stub.cpp as the HIP runtime, no GPU):
    returns run(which, stdin=None, env=None) -> the trace lines.  One hipcc job per source, at most 16 at a time; the kernel-argument
    layout is read from the code object inside each host object.  Built once per session (shared by the test modules)."""
    import atexit
    import shutil
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    if tool in _TRACE_TOOLS:
        return _TRACE_TOOLS[tool]
    csrc = os.path.join(ROOT, "generative_models_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    rocm = Path(os.path.realpath(hipcc)).parent.parent
    llvm = next((d for d in (rocm / "llvm" / "bin", rocm / "lib" / "llvm" / "bin") if (d / "clang++").exists()), None)
    if llvm is None:
        pytest.skip("clang++ of the ROCm toolchain not found")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    tmp = tempfile.mkdtemp(prefix=tool + "_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)

    def compile_one(src):
        obj = os.path.join(tmp, src + ".o")
        r = subprocess.run([hipcc] + flags + ["-c", os.path.join(csrc, src + ".hip"), "-o", obj], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        fat, co = os.path.join(tmp, src + ".hipfb"), os.path.join(tmp, src + ".co")
        r = subprocess.run([str(llvm / "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull], capture_output=True, timeout=120)
        if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
            return obj, ""          # no kernels in this source
        subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                        "--output=" + co], check=True, timeout=120)
        return obj, subprocess.run([str(llvm / "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True, timeout=120).stdout

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        built = list(pool.map(compile_one, sources))
    notes = os.path.join(tmp, "notes.txt")
    with open(notes, "w") as f:
        f.write("".join(n for _, n in built))
    exe = os.path.join(tmp, tool)
    r = subprocess.run([str(llvm / "clang++"), "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + str(rocm / "include"),
                        os.path.join(ROOT, "tools", tool + ".cpp"), os.path.join(ROOT, "tools", "launch_trace_stub.cpp")] + [o for o, _ in built] + ["-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(which, stdin=None, env=None):
        base = {k: v for k, v in os.environ.items() if not k.startswith("GMK_")}
        r = subprocess.run([exe, which], input=stdin, capture_output=True, text=True, timeout=600, env=dict(base, LAUNCH_TRACE_NOTES=notes, **(env or {})))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    _TRACE_TOOLS[tool] = run
    return run


CONV_SOURCES = ("conv_halo", "conv_igemm", "conv_subpixel", "conv_wgrad_slots", "conv_wgrad_subpixel", "conv1x1_stream", "gmk_common")
