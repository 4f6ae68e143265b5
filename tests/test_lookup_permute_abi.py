"""CPU-side ABI checks of the lookup-argument diagnostic: the entry point is
declared in include/taiga_gpu.h, exported by the library, given argtypes by
taiga_amd/api.py and wrapped by TaigaGpu; without a context it is
TG_ERR_BADARG, never a crash (no compute without a GPU). The three profiling
names of the lookup stage are in the header's tg_prof_get name list."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "taiga_amd", "csrc")
LIB = os.path.join(CSRC, "libtaiga_gpu.so")
HDR = os.path.join(REPO, "include", "taiga_gpu.h")

C = ctypes
NAME = "tg_lookup_permute_probe"
ARGTYPES = [C.c_uint64] + [C.c_char_p] * 4


@pytest.fixture(scope="module")
def lib():
    import taiga_amd

    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return taiga_amd.api.load_library()


def test_declared_exported_and_typed(lib):
    hdr = open(HDR).read()
    assert re.search(r"^int %s\(tg_ctx\* ctx, uint64_t u,[^;]*\);" % NAME, hdr, re.M), \
        f"{NAME} is not declared in taiga_gpu.h"
    assert hasattr(ctypes.CDLL(LIB), NAME), f"{NAME} missing from libtaiga_gpu.so"
    assert getattr(lib, NAME).argtypes == [C.c_void_p] + ARGTYPES


def test_null_context_is_badarg(lib):
    one = (1).to_bytes(32, "little")
    ap = ctypes.create_string_buffer(32)
    sp = ctypes.create_string_buffer(32)
    assert getattr(lib, NAME)(None, 1, one, one, ap, sp) == -2


def test_wrapper_exists():
    import taiga_amd

    assert callable(taiga_amd.TaigaGpu.lookup_permute_probe)


def test_prof_names_listed():
    """the header's tg_prof_get name list carries the lookup-stage names"""
    hdr = open(HDR).read()
    for name in ("lk_compress", "lk_sort", "lk_permute"):
        assert f'"{name}"' in hdr
