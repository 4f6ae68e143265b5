"""create_proof runs the lookup argument's compress, sort and permute on the
device (taiga_amd/csrc/lookup_argument.hip): proofs stay byte-identical to
the CPU oracle's on CS1 (with the three lookup profiling names reporting
launches), on the four-lookup edge circuit and on two random circuits with
two lookups, and a witness that violates a lookup is refused with
TG_ERR_BADARG, after which the same context proves the valid witness.

The keys take the interpreter gate path (TG_NO_RTC): the lookup stage is the
same on both, and no kernel is compiled at keygen."""
import ctypes
import os
import sys

import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_rand_circuit as grc  # noqa: E402

import pypasta as pp  # noqa: E402

pytestmark = pytest.mark.gpu

INST = bytes(32)
WIT = bytes([1]) + bytes(31)
RNG = bytes([2]) + bytes(31)
N = 1 << 15


@pytest.fixture(scope="module")
def oracle():
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "liboracle.so"))
    lib.orc_prove_raw.restype = ctypes.c_long
    lib.orc_prove_cs1.restype = ctypes.c_long
    yield lib
    lib.orc_prover_reset()


@pytest.fixture(scope="module")
def gpu(params15):
    import taiga_amd

    had = os.environ.get("TG_NO_RTC")
    os.environ["TG_NO_RTC"] = "1"  # read at keygen
    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params15)
    yield g
    g.close()
    if had is None:
        del os.environ["TG_NO_RTC"]
    else:
        os.environ["TG_NO_RTC"] = had


def oracle_init(lib, desc, params15):
    lib.orc_prover_reset()  # other modules init the global PK with other descs
    assert lib.orc_prover_init(desc, len(desc), params15, len(params15)) in (0, 1)


def oracle_prove_raw(lib, inst, adv):
    out = ctypes.create_string_buffer(1 << 15)
    return lib.orc_prove_raw(inst, adv, RNG, out, 1 << 15), out


def test_cs1_proof_runs_lookup_stage_on_device(gpu, oracle, params15):
    desc = open(os.path.join(GOLDEN, "cs1.desc"), "rb").read()
    oracle_init(oracle, desc, params15)
    out = ctypes.create_string_buffer(1 << 14)
    m = oracle.orc_prove_cs1(INST, WIT, RNG, out, 1 << 14)
    assert m > 0, f"oracle prove failed rc={m}"
    gpu.select_key(gpu.keygen(desc))
    gpu.prof_enable(True)
    gpu.prof_reset()
    try:
        proof = gpu.create_proof(INST, WIT, RNG)
        assert proof == out.raw[:m]
        for name in ("lk_compress", "lk_sort", "lk_permute"):
            ms, count = gpu.prof_get(name)
            assert count >= 1, f"{name}: no launch recorded"
            assert ms > 0
    finally:
        gpu.prof_enable(False)


# name -> (generator, lookups); seeds 4 and 5 have bf = 4 and 6: two row counts u
CIRCUITS = {
    "lookups4x4": (lambda: grc.gen_edge("lookups4x4"), 4),
    "gen4": (lambda: grc.gen(4), 2),
    "gen5": (lambda: grc.gen(5), 2),
}


_REFS = {}
_SLOTS = {}


def reference(lib, params15, name):
    """the circuit, its witness and the oracle's proof, computed once"""
    if name not in _REFS:
        make, nlk = CIRCUITS[name]
        desc, inst, adv, meta = make()
        assert meta["n_lookups"] == nlk
        oracle_init(lib, desc, params15)
        n, out = oracle_prove_raw(lib, inst, adv)
        assert n > 0, f"{name}: oracle prove failed rc={n}"
        _REFS[name] = (desc, inst, adv, meta, out.raw[:n])
    return _REFS[name]


def select(gpu, name, desc):
    """one keygen per circuit on the shared context"""
    if name not in _SLOTS:
        _SLOTS[name] = gpu.keygen(desc)
    gpu.select_key(_SLOTS[name])


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_lookup_circuits_match_the_oracle(gpu, oracle, params15, name):
    desc, inst, adv, meta, ref = reference(oracle, params15, name)
    select(gpu, name, desc)
    assert gpu.create_proof_raw(inst, adv, RNG) == ref, \
        f"{name} ({meta}): proof bytes differ from the oracle's"


def test_lookup_violation_is_refused_and_context_recovers(gpu, oracle, params15):
    import taiga_amd

    desc, inst, adv, meta, ref = reference(oracle, params15, "gen4")
    # advice column 1 is every lookup's input: p - 1 is in no table
    bad = bytearray(adv)
    bad[32 * N:2 * 32 * N] = (pp.P - 1).to_bytes(32, "little") * N
    bad = bytes(bad)
    oracle_init(oracle, desc, params15)
    n_bad, _ = oracle_prove_raw(oracle, inst, bad)
    assert n_bad <= 0, "the oracle accepts the violating witness"
    select(gpu, "gen4", desc)
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.create_proof_raw(inst, bad, RNG)
    assert e.value.rc == -2
    assert gpu.create_proof_raw(inst, adv, RNG) == ref
