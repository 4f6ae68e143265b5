"""CPU-side ABI checks: the C-ABI library builds, loads, and exports every
symbol include/taiga_gpu.h declares (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "taiga_amd", "csrc")
LIB = os.path.join(CSRC, "libtaiga_gpu.so")
HDR = os.path.join(REPO, "include", "taiga_gpu.h")


def _build():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)


def test_library_builds_and_loads():
    _build()
    lib = ctypes.CDLL(LIB)
    assert lib is not None


def test_every_header_symbol_exported():
    _build()
    lib = ctypes.CDLL(LIB)
    hdr = open(HDR).read()
    # every declared function: "<ret> tg_name(" at top level
    names = re.findall(r"^\s*(?:int|void|const char\*)\s+(tg_\w+)\s*\(", hdr, re.M)
    assert len(names) >= 15, names
    for n in names:
        assert hasattr(lib, n), f"symbol {n} missing from libtaiga_gpu.so"


def test_gate_path_entry_point():
    """tg_key_gate_path is declared, exported and wrapped; without a context
    it is TG_ERR_BADARG, never a crash"""
    import taiga_amd

    _build()
    hdr = open(HDR).read()
    assert re.search(r"^int tg_key_gate_path\(tg_ctx\* ctx\);", hdr, re.M)
    lib = taiga_amd.api.load_library()
    assert lib.tg_key_gate_path.argtypes == [ctypes.c_void_p]
    assert lib.tg_key_gate_path(None) == -2
    assert callable(taiga_amd.TaigaGpu.key_gate_path)


def test_device_count_callable_without_gpu():
    import taiga_amd

    # may be 0 here (no GPU in the dev container) — must not raise
    n = taiga_amd.api.device_count()
    assert n >= 0


def test_no_silent_fallback():
    """The product API must raise without a usable device, never fall back."""
    import taiga_amd

    if taiga_amd.api.device_count() > 0:
        return  # on a GPU box this is exercised by the gpu tests
    try:
        taiga_amd.TaigaGpu(0)
        assert False, "TaigaGpu() must raise when no HIP device exists"
    except taiga_amd.TaigaGpuError:
        pass
