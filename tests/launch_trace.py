"""Builds the host-dispatch trace tools of tools/ (gn_launch_trace.cpp, conv_launch_trace.cpp, smallconv_launch_trace.cpp) against the tree's
csrc/ without a GPU; used by tests/test_host_logic.py, tests/test_host_conv_ref.py and tests/test_host_gn_ref.py."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TRACE_TOOLS = {}


def build(tool, sources):
    """tools/<tool>.cpp built against the tree's csrc/<sources>.hip (host objects + tools/launch_trace_stub.cpp as the HIP runtime, no GPU):
    returns run(which, stdin=None, env=None) -> the trace lines (run.notes: the file of the code objects' kernel metadata).  One hipcc job per source, at most 16 at a time; the kernel-argument
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
    run.notes = notes          # the code objects' kernel metadata as text: every kernel symbol the sources instantiate
    _TRACE_TOOLS[tool] = run
    return run


CONV_SOURCES = ("conv_halo", "conv_igemm", "conv_subpixel", "conv_wgrad_slots", "conv_wgrad_subpixel", "conv1x1_stream", "gmk_common")
SMALLCONV_SOURCES = ("smallconv", "gmk_common")      # tools/smallconv_launch_trace.cpp


def check_reported_kernels(lines, kernel_name):
    """The reported name is the launched kernel: on every successful trace line that launched something (rc=0, at least one launch=), the
    profile name of kernel=<id>, up to any '[', is the identifier of one of the line's launches (device names are mangled: <length><identifier>).
    A line that launched with kernel=0, or with an id outside the table, fails.  -> the number of lines checked"""
    checked = 0
    for line in lines:
        tail = line.partition(" -> ")[2]
        launches = re.findall(r" launch=(\S+)", tail)
        if not launches or not tail.startswith("rc=0 "):
            continue
        kid = int(re.findall(r'" kernel=(-?\d+)', tail)[-1])
        name = kernel_name(kid)
        assert name, f"launched with kernel={kid}, which is no id of the kernel table: {line[:400]}"
        plain = name.split("[")[0]
        assert any(f"{len(plain)}{plain}" in dev for dev in launches), f"kernel={kid} ({name}) reported, launched {launches}: {line[:400]}"
        checked += 1
    return checked


# Which kernel the six stem / head entry points of csrc/smallconv.hip launch, written from the launch conditions of launch_expand, launch_wgrad
# and launch_head_contraction as they stood before the launchers reported an id: (entry, storage type, C, image channels, H, W,
# GMK_DEV_VARIANT) -> device function.  B = 2.
F32, BF16, F16 = 0, 1, 2
_AT_8X8 = {      # variant 0, 8 x 8, the same for 1 and 3 image channels: (entry, type, C) -> kernel
    ("stem_fwd", BF16, 128): "expand3x3_tile16_kernel", ("stem_fwd", F16, 128): "expand3x3_tile16_kernel",      # 16-bit results, W <= 128, <= 3 channels: tiled
    ("stem_fwd", F32, 128): "expand3x3_mfma_kernel", ("stem_fwd", BF16, 256): "expand3x3_kernel",              # fp32: the exact chain; C = 256: VALU
    ("head_dgrad", BF16, 128): "expand3x3_tile16_kernel", ("head_dgrad", F32, 128): "expand3x3_mfma_kernel", ("head_dgrad", BF16, 256): "expand3x3_kernel",
    ("stem_wgrad", BF16, 128): "wgrad3x3_tile16_kernel", ("stem_wgrad", F32, 128): "wgrad3x3_mfma_kernel", ("stem_wgrad", BF16, 256): "wgrad3x3_kernel",
    ("head_wgrad", BF16, 128): "wgrad3x3_tile16_kernel", ("head_wgrad", F16, 128): "wgrad3x3_tile16_kernel",
    ("head_wgrad", F32, 128): "wgrad3x3_mfma_kernel", ("head_wgrad", BF16, 256): "wgrad3x3_kernel",
    ("head_fwd", BF16, 128): "head_fwd_mfma_kernel", ("head_fwd", F16, 128): "head_fwd_mfma_kernel",
    ("head_fwd", F32, 128): "head_fwd_kernel", ("head_fwd", BF16, 256): "head_fwd_kernel",                      # the matrix-core form is 16-bit, C = 128 only
    ("stem_dgrad", BF16, 128): "stem_dgrad_mfma_kernel", ("stem_dgrad", F16, 128): "stem_dgrad_mfma_kernel",
    ("stem_dgrad", F32, 128): "stem_dgrad_kernel", ("stem_dgrad", BF16, 256): "stem_dgrad_kernel",
}
SMALLCONV_LANDMARKS = {(entry, dt, C, cs, 8, 8, 0): name for (entry, dt, C), name in _AT_8X8.items() for cs in (1, 3)}
SMALLCONV_LANDMARKS.update({
    ("stem_fwd", F16, 128, 4, 8, 8, 0): "expand3x3_mfma_kernel",            # 4 image channels: no tiled form
    ("stem_fwd", F16, 128, 3, 4, 136, 0): "expand3x3_mfma_kernel",          # rows beyond 128 pixels: no tiled form
    ("stem_fwd", BF16, 128, 1, 8, 8, 41): "expand3x3_kernel",               # variant 41 keeps the VALU kernels,
    ("stem_fwd", BF16, 128, 1, 8, 8, 42): "expand3x3_mfma_kernel",          # 42 the fp32 chains
    ("head_dgrad", BF16, 128, 3, 32, 32, 0): "expand3x3_tile16_kernel",
    ("stem_wgrad", BF16, 128, 1, 6, 7, 0): "wgrad3x3_kernel",               # odd W: the matrix-core forms pair pixels
    ("stem_wgrad", BF16, 128, 3, 28, 28, 42): "wgrad3x3_mfma_kernel",
    ("head_wgrad", F16, 128, 4, 8, 8, 0): "wgrad3x3_kernel",                # 4 image channels: VALU
    ("head_wgrad", BF16, 128, 3, 4, 136, 0): "wgrad3x3_mfma_kernel",
    ("head_wgrad", BF16, 128, 3, 32, 32, 41): "wgrad3x3_kernel",
    ("head_fwd", F16, 128, 4, 8, 8, 0): "head_fwd_kernel",
    ("head_fwd", F16, 128, 3, 28, 28, 0): "head_fwd_mfma_kernel",
    ("head_fwd", F16, 128, 3, 28, 28, 41): "head_fwd_kernel",
    ("stem_dgrad", BF16, 128, 3, 32, 32, 0): "stem_dgrad_mfma_kernel",
    ("stem_dgrad", BF16, 128, 4, 32, 32, 0): "stem_dgrad_kernel",
    ("stem_dgrad", F16, 256, 2, 6, 7, 0): "stem_dgrad_kernel",
})
