"""The quotient (h-fold) kernels at the engine's capacity edges, on both
gate-evaluation paths.

k_h_fold (the interpreter in taiga_amd/csrc/prover_gpu.inc) and hf_gates (the
kernel hf_rtc.hpp specializes to a circuit with hipRTC) fold the same gates
into the quotient; which of the two a key uses is reported by
tg_key_gate_path(). The circuits are tools/gen_rand_circuit.gen_edge(): the
smallest shapes that sit on each limit of the engine (16 advice columns, 8
permutation chunks, stack peak 8, 4 lookups of 4+4 expressions, 64 queries,
the hf_gates cluster size, wide rotations, constants and instance cells
inside gates, ext 2^17 and 2^19).

CPU tier: the oracle proves and verifies every case, and the digests of
(desc, instance, advice, proof) equal tests/golden/hfold_edge_pins.json.
GPU tier: the product proves each case once through the interpreter
(TG_NO_RTC=1) and once through the specialized kernel; both proofs must have
the oracle's pinned digest, so the test is exact and runs no oracle."""
import ctypes
import functools
import hashlib
import json
import os
import sys
import time

import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_rand_circuit as grc  # noqa: E402

RNG = bytes([7]) + bytes(31)
PINS = json.load(open(os.path.join(GOLDEN, "hfold_edge_pins.json")))
TG_ERR_BADARG = -2


def sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=1)
def circuit(name):
    """generated once per case and shared by the tests that follow it"""
    desc, inst, adv, meta = grc.gen_edge(name)
    pin = PINS[name]
    assert (sha(desc), sha(inst), sha(adv)) == (pin["desc"], pin["instance"], pin["advice"]), \
        f"{name}: the generator no longer emits the pinned circuit"
    return desc, inst, adv, meta


def test_pin_file_lists_exactly_the_cases():
    assert sorted(PINS) == sorted(grc.EDGE_CASES)
    assert len(grc.EDGE_CASES) == 13
    for pin in PINS.values():
        assert sorted(pin) == ["advice", "desc", "instance", "proof"]
        assert all(len(v) == 64 for v in pin.values())


def test_cases_reach_their_edges():
    """the shape each case is there for, from the desc itself (k = 8: same
    shape, fewer rows)"""
    meta = {nm: grc.gen_edge(nm, k=8)[3] for nm in grc.EDGE_CASES}
    assert meta["adv13"]["n_advice"] == 13 and meta["adv16"]["n_advice"] == grc.MAX_ADVICE
    assert [meta[f"gates{m}"]["n_gates"] for m in (8, 9, 17)] == [8, 9, 17]
    assert meta["depth8"]["stack_peak"] == grc.MAX_STACK
    assert meta["chunks8"]["n_chunks"] == grc.MAX_CHUNKS and meta["chunks8"]["n_perm"] == 16
    assert meta["chunks8"]["chunk_len"] == 2
    assert meta["lookups4x4"]["n_lookups"] == grc.MAX_LOOKUPS
    assert meta["queries64"]["n_queries"] == grc.MAX_QUERIES
    assert meta["ext17"]["ext_k"] - meta["ext17"]["k"] == 2
    assert meta["ext19"]["ext_k"] - meta["ext19"]["k"] == 4
    # circuits without constants and with them
    assert meta["gates9"]["n_consts"] == 0 and meta["const_inst_ops"]["n_consts"] == 3


@pytest.fixture(scope="module")
def oracle():
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "liboracle.so"))
    lib.orc_prove_raw.restype = ctypes.c_long
    yield lib
    lib.orc_prover_reset()


@pytest.mark.parametrize("name", grc.EDGE_CASES)
def test_oracle_proves_edge_case(oracle, params15, name):
    desc, inst, adv, meta = circuit(name)
    oracle.orc_prover_reset()
    assert oracle.orc_prover_init(desc, len(desc), params15, len(params15)) == 0, \
        f"{name}: the oracle refuses the circuit ({meta})"
    out = ctypes.create_string_buffer(1 << 15)
    n = oracle.orc_prove_raw(inst, adv, RNG, out, 1 << 15)
    assert n > 0, f"{name}: oracle prove failed rc={n}"
    proof = out.raw[:n]
    assert oracle.orc_verify_raw(inst, proof, n) == 0
    bad = bytearray(proof)
    bad[-1] ^= 1
    assert oracle.orc_verify_raw(inst, bytes(bad), n) != 0
    assert sha(proof) == PINS[name]["proof"], f"{name}: oracle proof drifted from the pin"


def test_oracle_refuses_one_over(oracle, params15):
    """the oracle's parser carries the product's limits on advice columns,
    permutation chunks and lookup expressions. (A stack peak of 9 and 65
    queries are limits of the device evaluator alone; the oracle has no
    array that they would overrun.)"""
    for name in ("adv17", "chunks9", "ni5"):
        desc = grc.gen_over(name)[0]
        oracle.orc_prover_reset()
        assert oracle.orc_prover_init(desc, len(desc), params15, len(params15)) != 0, name


# ---------------------------------------------------------------- GPU tier

PATHS = {"interpreter": 0, "specialized": 1}


def _new_gpu(params15):
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params15)
    return g


def _set_path(monkeypatch, path, cache_dir):
    if path == "interpreter":
        monkeypatch.setenv("TG_NO_RTC", "1")
    else:
        monkeypatch.delenv("TG_NO_RTC", raising=False)
    # nothing stale is read and nothing is left behind in tests/golden
    monkeypatch.setenv("TG_HF_CACHE", str(cache_dir))


def _assert_path(g, path, what):
    got = g.key_gate_path()
    if path == "specialized":
        assert got == 1, (f"{what}: the key fell back to the interpreter; hipRTC could not "
                          "compile or load hf_gates (its log is on stderr)")
    else:
        assert got == 0, f"{what}: TG_NO_RTC=1 did not select the interpreter"


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))  # varies fastest: one circuit, both paths
@pytest.mark.parametrize("name", grc.EDGE_CASES)
def test_gpu_edge_case(params15, monkeypatch, tmp_path, name, path):
    desc, inst, adv, meta = circuit(name)
    _set_path(monkeypatch, path, tmp_path)
    t0 = time.perf_counter()
    g = _new_gpu(params15)
    try:
        t1 = time.perf_counter()
        g.select_key(g.keygen(desc))
        t2 = time.perf_counter()
        _assert_path(g, path, name)
        proof = g.create_proof_raw(inst, adv, RNG)
        t3 = time.perf_counter()
        ok = g.verify_proof_raw(inst, proof)
        bad = bytearray(proof)
        bad[len(bad) // 2] ^= 1
        tampered_ok = g.verify_proof_raw(inst, bytes(bad))
        t4 = time.perf_counter()
        print(f"\n[hfold-edge] {name}/{path}: ctx+srs {t1 - t0:.2f}s keygen {t2 - t1:.2f}s "
              f"proof {t3 - t2:.2f}s verify x2 {t4 - t3:.2f}s")
        assert sha(proof) == PINS[name]["proof"], \
            f"{name}/{path} ({meta}): proof differs from the oracle's"
        assert ok, f"{name}/{path}: the product verifier rejects its own proof"
        assert not tampered_ok, f"{name}/{path}: a one-bit tamper is accepted"
        if path == "specialized":
            assert [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")], \
                "the specialized kernel was not compiled into TG_HF_CACHE"
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_keygen_refuses_one_over(params15, monkeypatch, tmp_path):
    """one over the limit (advice 17, chunks 9, depth 9, queries 65, ni 5) is
    TG_ERR_BADARG at keygen, and the context proves afterwards"""
    import taiga_amd

    _set_path(monkeypatch, "specialized", tmp_path)
    g = _new_gpu(params15)
    try:
        for name in grc.OVER_CASES:
            desc = grc.gen_over(name)[0]
            with pytest.raises(taiga_amd.TaigaGpuError) as ei:
                g.keygen(desc)
            assert ei.value.rc == TG_ERR_BADARG, (name, ei.value.rc)
        desc, inst, adv, _ = circuit("const_inst_ops")
        g.select_key(g.keygen(desc))
        assert sha(g.create_proof_raw(inst, adv, RNG)) == PINS["const_inst_ops"]["proof"]
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_compliance_both_paths(params15, monkeypatch):
    """the real compliance circuit through the interpreter and through the
    specialized kernel (the code object the build shipped): equal proofs, and
    equal to the frozen oracle proof of tests/test_compliance_circuit.py"""
    import test_compliance_circuit as tcc

    tcc._ensure_artifacts()
    desc = open(os.path.join(GOLDEN, "compliance.desc"), "rb").read()
    tgw = open(os.path.join(GOLDEN, "compliance.tgw"), "rb").read()
    borsh = bytes.fromhex(tcc._load_sample("compliance")["witness_borsh"])
    pin = open(os.path.join(GOLDEN, "compliance_proof_pin.bin"), "rb").read()
    proofs = {}
    for path in PATHS:
        _set_path(monkeypatch, path, GOLDEN)
        g = _new_gpu(params15)
        try:
            g.select_key(g.keygen(desc))
            _assert_path(g, path, "compliance")
            g.witness_program_load(tgw)
            proofs[path], _ = g.compliance_prove(borsh, tcc.RNG)
        finally:
            g.close()
    assert proofs["interpreter"] == proofs["specialized"]
    assert proofs["interpreter"] == pin
