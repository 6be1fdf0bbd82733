"""CPU-side checks of the C-ABI boundary: the library loads and exports every symbol that
include/idb_kernels.h declares (no compute calls: there is no GPU here)."""
import os
import re

from faceposegenerator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "idb_kernels.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(idb_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree():
    assert _header_symbols() == sorted(_lib.EXPORTS)


def test_library_exports_every_declared_symbol(lib):
    for name in _header_symbols():
        assert hasattr(lib, name), name
    assert lib.idb_version() >= 100


def test_last_error_is_a_string(lib):
    assert isinstance(lib.idb_last_error(), bytes)


def test_invalid_descriptor_is_rejected_without_gpu(lib):
    # argument validation happens before any HIP call, so it is testable on CPU
    import ctypes as C
    d = _lib.GemmDesc()
    d.dtype = 7
    assert lib.idb_gemm(C.byref(d), None, 0, None) == -1
    assert b"dtype" in lib.idb_last_error()
    d.dtype, d.batch, d.out_h, d.out_w, d.n, d.stride, d.nsrc = 0, 1, 1, 1, 64, 1, 1
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = 0x1000, 100, 1, 1, 1
    assert lib.idb_gemm(C.byref(d), None, 0, None) == -1
    assert b"multiple of 64" in lib.idb_last_error()


def test_product_path_fails_loudly_without_gpu():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from faceposegenerator_amd import spec as S
    from faceposegenerator_amd.engine import HipEngine
    with pytest.raises(_lib.IdbError):
        HipEngine(S.TINY_UNET, S.TINY_VAE, None, None)
    from faceposegenerator_amd.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline(S.TINY_UNET, S.TINY_VAE, {}, {})
    with pytest.raises(ValueError):
        pipe.to("cpu")


def test_no_kernel_uses_scratch_or_spills(lib):
    """The build writes the compiler's kernel-resource-usage remarks to faceposegenerator_amd/kernel_resources.txt (csrc/Makefile).
    No kernel may touch scratch memory or spill VGPRs: a run-time loop bound once put conv_in's input window into 160 bytes of
    scratch per lane (1.4 % of the batch-64 step), invisible to every parity test."""
    path = os.path.join(ROOT, "faceposegenerator_amd", "kernel_resources.txt")
    if not os.path.isfile(path):                      # a library built before this report existed: rebuild in place
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "faceposegenerator_amd", "csrc"), "-j8", "-B"], check=True, capture_output=True)
    txt = open(path).read()
    kernels = re.split(r"remark: [^\n]*Function Name: ", txt)[1:]
    assert len(kernels) >= 100
    bad = []
    for k in kernels:
        name = k.split("\n")[0].split(" ")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", k).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", k).group(1))
        if scratch or vspill:
            bad.append((name, scratch, vspill))
    assert not bad, bad


def test_library_shares_torchs_hip_runtime(lib):
    """Loaded before torch (build() then smoke() in one process), the library must still bind to torch's HIP runtime: a second
    libamdhip64 / libhsa-runtime64 in the process finds no device once torch's has initialised."""
    import subprocess
    import sys
    code = ("from faceposegenerator_amd import _lib; _lib.load(); import torch\n"
            "print(sorted({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l or 'libhsa-runtime64' in l}))")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    maps = eval(p.stdout.strip().splitlines()[-1])
    assert len([m for m in maps if "libamdhip64" in m]) == 1 and len([m for m in maps if "libhsa-runtime64" in m]) == 1, maps
