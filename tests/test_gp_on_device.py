"""create_proof computes its grand products on the device: with profiling on,
one CS1 proof is byte-identical to the CPU oracle's (obtained the way
tests/test_prover_parity.py obtains it) and the context then reports
launches under each of the grand-product profiling names."""
import ctypes
import os

import pytest

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

INST = bytes(32)
WIT = bytes([1]) + bytes(31)
RNG = bytes([2]) + bytes(31)


def test_cs1_proof_runs_grand_products_on_device(params15):
    import taiga_amd

    desc = open(os.path.join(GOLDEN, "cs1.desc"), "rb").read()
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "liboracle.so"))
    lib.orc_prover_reset()  # other modules init the global PK with other descs
    assert lib.orc_prover_init(desc, len(desc), params15, len(params15)) in (0, 1)
    lib.orc_prove_cs1.restype = ctypes.c_long
    out = ctypes.create_string_buffer(1 << 14)
    m = lib.orc_prove_cs1(INST, WIT, RNG, out, 1 << 14)
    assert m > 0, f"oracle prove failed rc={m}"

    g = taiga_amd.TaigaGpu(0)
    try:
        g.load_srs(params15)
        g.keygen(desc)
        g.prof_enable(True)
        g.prof_reset()
        proof = g.create_proof(INST, WIT, RNG)
        assert proof == out.raw[:m]
        for name in ("gp_terms", "gp_inverse", "gp_scan"):
            ms, count = g.prof_get(name)
            assert count >= 1, f"{name}: no launch recorded"
            assert ms > 0
    finally:
        g.close()
