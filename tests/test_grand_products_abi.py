"""CPU-side ABI checks of the grand-product diagnostics: the four entry
points are declared in include/taiga_gpu.h, exported by the library, given
argtypes by taiga_amd/api.py and wrapped by TaigaGpu; without a context each
is TG_ERR_BADARG, never a crash (no compute without a GPU)."""
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
# entry point -> (TaigaGpu method, argtypes after the context)
ENTRIES = {
    "tg_fp_batch_inverse": ("fp_batch_inverse", [C.c_char_p, C.c_size_t]),
    "tg_fp_prefix_product": (
        "fp_prefix_product",
        [C.c_char_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_char_p, C.c_char_p]),
    "tg_perm_product_probe": (
        "perm_product_probe",
        [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_char_p] * 5),
    "tg_lookup_product_probe": (
        "lookup_product_probe", [C.c_uint32, C.c_uint64] + [C.c_char_p] * 7),
}


@pytest.fixture(scope="module")
def lib():
    import taiga_amd

    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return taiga_amd.api.load_library()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_declared_exported_and_typed(lib, name):
    hdr = open(HDR).read()
    assert re.search(r"^int %s\(tg_ctx\* ctx,[^;]*\);" % name, hdr, re.M), \
        f"{name} is not declared in taiga_gpu.h"
    assert hasattr(ctypes.CDLL(LIB), name), f"{name} missing from libtaiga_gpu.so"
    assert getattr(lib, name).argtypes == [C.c_void_p] + ENTRIES[name][1]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_context_is_badarg(lib, name):
    one = (1).to_bytes(32, "little")
    buf = ctypes.create_string_buffer(32 * 64)
    lens = (C.c_uint64 * 1)(1)
    args = {
        "tg_fp_batch_inverse": (buf, 1),
        "tg_fp_prefix_product": (one, lens, 1, one, buf),
        "tg_perm_product_probe": (4, 1, 1, 1, bytes(buf), bytes(buf), one, one, buf),
        "tg_lookup_product_probe": (4, 1) + (bytes(buf),) * 4 + (one, one, buf),
    }[name]
    assert getattr(lib, name)(None, *args) == -2


def test_wrappers_exist():
    import taiga_amd

    for method, _ in ENTRIES.values():
        assert callable(getattr(taiga_amd.TaigaGpu, method))


def test_prof_names_listed():
    """the header's tg_prof_get name list carries the grand-product names"""
    hdr = open(HDR).read()
    for name in ("gp_terms", "gp_inverse", "gp_scan"):
        assert f'"{name}"' in hdr
