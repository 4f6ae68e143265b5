"""GPU tests of the resident MSM / NTT entry points, the calls bench.py times:
tg_gen_bases / tg_bases_upload -> tg_scalars_upload -> tg_msm_resident, and
tg_poly_upload -> tg_ntt_resident -> tg_poly_download. The kernels behind them
are covered through tg_msm_pallas / tg_ntt_fp elsewhere; what is pinned here
is the state these calls keep between calls (which buffer is valid, for how
many elements, on which accumulation path) and the contract of
include/taiga_gpu.h for rejected uploads, out-of-range scalars, bad arguments
and the prover sharing the scalar buffer.

Everything is bit-exact against the CPU oracle or Python integers. Sizes are
the smallest that select the path (kernel_shapes.expected_msm_cfg pins the
window width). One context serves the module; a test that needs a context with
nothing resident makes its own. No test relies on what another left behind."""
import ctypes
import os
import random

import pytest

import oracle_ct as oc
import pypasta as pp
from conftest import GOLDEN, REPO
from kernel_shapes import expected_msm_cfg

pytestmark = pytest.mark.gpu

P, Q = pp.P, pp.Q
ID64 = b"\x00" * 64
BASE_SEED = 31337
NB = 4096  # the largest base count any test here uses

OK, BADARG, ENCODING, NOSRS, STATE = 0, -2, -3, -4, -6

INST = bytes(32)
WIT = bytes([1]) + bytes(31)
RNG = bytes([2]) + bytes(31)

# what "canonical" excludes: p itself and everything above, up to the values
# whose top window carries out of the signed-digit recoding
OUT_OF_RANGE = [P, P + 1, (1 << 255) - 1, 1 << 255, (1 << 255) + (1 << 254), (1 << 256) - 1]


@pytest.fixture(scope="module")
def gpu(params15):
    """The module's context: k = 15 SRS loaded and a key for cs1.desc."""
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params15)
    with open(os.path.join(GOLDEN, "cs1.desc"), "rb") as fh:
        g.keygen(fh.read())
    yield g
    g.close()


@pytest.fixture
def fresh():
    """A context that holds nothing."""
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def bases():
    """What tg_gen_bases(n <= NB, BASE_SEED) generates, from the oracle
    (gen_bases(n) is a prefix of gen_bases(m > n); the parity test below
    downloads the device's and compares)."""
    return oc.gen_bases(NB, BASE_SEED)


@pytest.fixture(scope="module")
def oracle_proof(params15):
    """The CPU oracle's proof for (INST, WIT, RNG) over cs1.desc: the bytes
    test_prover_parity.py holds the device prover to."""
    lib = ctypes.CDLL(os.path.join(REPO, "oracle", "liboracle.so"))
    with open(os.path.join(GOLDEN, "cs1.desc"), "rb") as fh:
        desc = fh.read()
    lib.orc_prover_reset()
    assert lib.orc_prover_init(desc, len(desc), params15, len(params15)) in (0, 1)
    lib.orc_prove_cs1.restype = ctypes.c_long
    out = ctypes.create_string_buffer(1 << 14)
    n = lib.orc_prove_cs1(INST, WIT, RNG, out, 1 << 14)
    assert n > 0
    return out.raw[:n]


def gpu_error():
    import taiga_amd

    return taiga_amd.TaigaGpuError


def raises_rc(rc, fn, *args, **kw):
    with pytest.raises(gpu_error()) as e:
        fn(*args, **kw)
    assert e.value.rc == rc, (e.value.rc, rc)


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def rand_canon(rng, n):
    """n canonical field reprs (< 2^254 < p) without a per-element loop."""
    raw = bytearray(rng.getrandbits(n * 256).to_bytes(n * 32, "little"))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    return bytes(raw)


def with_scalar(sc, pos, s):
    return sc[:32 * pos] + b32(s) + sc[32 * (pos + 1):]


# ---------------- resident MSM: parity ----------------

@pytest.mark.parametrize("n,c", [(1, 8), (1024, 8), (2048, 9)])
def test_msm_resident_parity_both_paths(gpu, bases, n, c):
    assert expected_msm_cfg(n).c == c
    sc = rand_canon(random.Random(100 + n), n)
    exp = oc.msm(oc.FQ, sc, bases[:64 * n])
    assert exp != ID64
    # device-generated bases: the branch-free accumulation path
    gpu.gen_bases(n, BASE_SEED)
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    assert gpu.msm(sc) == exp
    dl = gpu.bases_download(n)
    assert dl == bases[:64 * n]
    # the same bytes uploaded: the safe path
    gpu.bases_upload(dl)
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    assert gpu.msm(sc) == exp


def test_msm_resident_srs_sets(gpu, params15):
    n, N = 2048, 1 << 15
    assert expected_msm_cfg(n).c == 9
    sc = rand_canon(random.Random(200), n)
    gpu.scalars_upload(sc)
    g = oc.decompress(oc.FQ, params15[4:4 + 32 * n])
    gl = oc.decompress(oc.FQ, params15[4 + 32 * N:4 + 32 * N + 32 * n])
    assert gpu.msm_resident(n, base_set=1) == oc.msm(oc.FQ, sc, g)
    assert gpu.msm_resident(n, base_set=2) == oc.msm(oc.FQ, sc, gl)


def test_msm_resident_prefix_reupload_growth_and_repeat(gpu, bases):
    assert expected_msm_cfg(1024).c == 8 and expected_msm_cfg(2048).c == 9
    assert expected_msm_cfg(4096).c == 10
    rng = random.Random(300)
    sc2k, sc1k, sc4k = rand_canon(rng, 2048), rand_canon(rng, 1024), rand_canon(rng, 4096)
    assert sc1k != sc2k[:32 * 1024]
    gpu.gen_bases(NB, BASE_SEED)
    gpu.scalars_upload(sc2k)
    exp2k = oc.msm(oc.FQ, sc2k, bases[:64 * 2048])
    # a prefix of the resident scalars, then all of them again
    assert gpu.msm_resident(1024) == oc.msm(oc.FQ, sc2k[:32 * 1024], bases[:64 * 1024])
    assert gpu.msm_resident(2048) == exp2k
    # a shorter upload replaces them: the tail of the old ones is not resident
    gpu.scalars_upload(sc1k)
    assert gpu.msm_resident(1024) == oc.msm(oc.FQ, sc1k, bases[:64 * 1024])
    raises_rc(STATE, gpu.msm_resident, 2048)
    # a longer one grows the buffer
    gpu.scalars_upload(sc4k)
    exp4k = oc.msm(oc.FQ, sc4k, bases[:64 * 4096])
    got = [gpu.msm_resident(4096) for _ in range(3)]
    assert got == [exp4k] * 3


def test_base_set_switching_on_one_context(gpu, bases):
    """generated -> uploaded with degenerate points -> generated: the
    accumulation path has to follow the bases each time."""
    n = 2048
    rng = random.Random(400)
    sc = bytearray(rand_canon(rng, n))
    sc[32 * 6:32 * 7] = sc[32 * 5:32 * 6]  # the duplicate pair, equal scalars
    sc[32 * 8:32 * 9] = sc[32 * 7:32 * 8]  # P and -P, equal scalars
    sc = bytes(sc)
    deg = bytearray(bases[:64 * n])
    deg[64 * 3:64 * 4] = ID64
    deg[64 * 6:64 * 7] = deg[64 * 5:64 * 6]
    x, y = deg[64 * 7:64 * 7 + 32], int.from_bytes(deg[64 * 7 + 32:64 * 8], "little")
    deg[64 * 8:64 * 9] = x + b32(Q - y)
    deg = bytes(deg)
    exp_gen = oc.msm(oc.FQ, sc, bases[:64 * n])
    exp_deg = oc.msm(oc.FQ, sc, deg)
    assert exp_gen != exp_deg
    gpu.scalars_upload(sc)
    gpu.gen_bases(n, BASE_SEED)
    assert gpu.msm_resident(n) == exp_gen
    gpu.bases_upload(deg)
    assert gpu.msm_resident(n) == exp_deg
    assert gpu.msm(sc) == exp_deg
    gpu.gen_bases(n, BASE_SEED)
    assert gpu.msm_resident(n) == exp_gen
    assert gpu.msm(sc) == exp_gen


def test_prof_counts_msm_calls(gpu, bases):
    n = 1024
    sc = rand_canon(random.Random(500), n)
    exp = oc.msm(oc.FQ, sc, bases[:64 * n])
    gpu.gen_bases(n, BASE_SEED)
    gpu.scalars_upload(sc)
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        assert [gpu.msm_resident(n) for _ in range(3)] == [exp] * 3
        assert gpu.msm(sc) == exp
        raises_rc(STATE, gpu.msm_resident, n + 1)  # refused calls do not count
        assert gpu.prof_get("msm_total")[1] == 4
        assert gpu.prof_get("ntt_total")[1] == 0
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()


# ---------------- scalar range ----------------

@pytest.mark.parametrize("s", OUT_OF_RANGE, ids=["p", "p+1", "2^255-1", "2^255",
                                                 "2^255+2^254", "2^256-1"])
def test_out_of_range_scalar_is_an_encoding_error(gpu, s):
    n = 1024
    assert expected_msm_cfg(n).c == 8
    good = rand_canon(random.Random(600), n)
    gpu.gen_bases(n, BASE_SEED)
    for pos in (0, n // 2, n - 1):
        bad = with_scalar(good, pos, s)
        gpu.scalars_upload(good)
        raises_rc(ENCODING, gpu.scalars_upload, bad)
        raises_rc(STATE, gpu.msm_resident, 1)
        gpu.scalars_upload(good)
        raises_rc(ENCODING, gpu.msm, bad)
        raises_rc(STATE, gpu.msm_resident, 1)


def test_largest_canonical_scalar_is_accepted(gpu, bases):
    n = 1024
    good = rand_canon(random.Random(601), n)
    gpu.gen_bases(n, BASE_SEED)
    for pos in (0, n // 2, n - 1):
        sc = with_scalar(good, pos, P - 1)
        exp = oc.msm(oc.FQ, sc, bases[:64 * n])
        gpu.scalars_upload(sc)
        assert gpu.msm_resident(n) == exp
        assert gpu.msm(sc) == exp


def test_single_scalar_p_is_an_encoding_error(gpu):
    gpu.gen_bases(1, BASE_SEED)
    raises_rc(ENCODING, gpu.scalars_upload, b32(P))
    raises_rc(STATE, gpu.msm_resident, 1)
    raises_rc(ENCODING, gpu.msm, b32(P))
    raises_rc(STATE, gpu.msm_resident, 1)


# ---------------- rejected bases ----------------

@pytest.mark.parametrize("n,bad_at", [(1024, 1023), (1, 0)])
def test_rejected_bases_leave_none_resident(gpu, bases, n, bad_at):
    sc = rand_canon(random.Random(700 + n), n)
    pts = bases[64 * 100:64 * (100 + n)]  # not the set gen_bases leaves
    bad = bytearray(pts)
    bad[64 * bad_at] ^= 1  # x moves, y stays: off the curve
    assert not oc.pt_on_curve(oc.FQ, bytes(bad[64 * bad_at:64 * (bad_at + 1)]))
    gpu.gen_bases(1024, BASE_SEED)
    gpu.scalars_upload(sc)
    raises_rc(ENCODING, gpu.bases_upload, bytes(bad))
    raises_rc(STATE, gpu.msm, sc)
    gpu.scalars_upload(sc)
    raises_rc(STATE, gpu.msm_resident, n)
    raises_rc(STATE, gpu.msm_resident, 1)
    raises_rc(BADARG, gpu.bases_download, 1)
    gpu.bases_upload(pts)
    exp = oc.msm(oc.FQ, sc, pts)
    assert gpu.msm_resident(n) == exp
    assert gpu.msm(sc) == exp
    assert gpu.bases_download(n) == pts


# ---------------- the prover shares the scalar buffer ----------------

def test_prover_and_verifier_invalidate_resident_scalars(gpu, bases, oracle_proof):
    n = 2048
    sc = rand_canon(random.Random(800), n)
    exp = oc.msm(oc.FQ, sc, bases[:64 * n])
    gpu.gen_bases(n, BASE_SEED)
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    proof = gpu.create_proof(INST, WIT, RNG)
    assert proof == oracle_proof
    raises_rc(STATE, gpu.msm_resident, n)
    raises_rc(STATE, gpu.msm_resident, 1)
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    assert gpu.create_proof(INST, WIT, RNG) == oracle_proof
    # the same around the verifier
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    assert gpu.verify_proof(INST, proof)
    raises_rc(STATE, gpu.msm_resident, n)
    gpu.scalars_upload(sc)
    assert gpu.msm_resident(n) == exp
    assert gpu.verify_proof(INST, proof)


# ---------------- argument guards ----------------

def test_msm_argument_guards(gpu, fresh):
    n = 1024
    sc = rand_canon(random.Random(900), n)
    gpu.gen_bases(n, BASE_SEED)
    gpu.scalars_upload(sc)
    for base_set in (-1, 3, 7):
        raises_rc(BADARG, gpu.msm_resident, n, base_set=base_set)
        raises_rc(BADARG, gpu.msm, sc, base_set=base_set)
    out = ctypes.create_string_buffer(64)
    for base_set in (0, 1, 2):
        assert gpu._lib.tg_msm_resident(gpu._h, 0, base_set, out) == BADARG
        assert gpu._lib.tg_msm_pallas(gpu._h, sc, 0, base_set, out) == BADARG
    # the refused calls left the resident inputs alone
    assert gpu.msm_resident(n) == gpu.msm(sc)
    # more scalars than the k = 15 SRS has points
    big = rand_canon(random.Random(901), (1 << 15) + 1)
    gpu.scalars_upload(big)
    raises_rc(BADARG, gpu.msm_resident, (1 << 15) + 1, base_set=1)
    raises_rc(BADARG, gpu.msm_resident, (1 << 15) + 1, base_set=2)
    # a context with nothing resident
    raises_rc(STATE, fresh.msm_resident, 1)
    raises_rc(NOSRS, fresh.msm_resident, 1, base_set=1)
    fresh.scalars_upload(sc)
    raises_rc(STATE, fresh.msm_resident, 1)  # scalars but no bases
    raises_rc(NOSRS, fresh.msm_resident, 1, base_set=1)
    raises_rc(NOSRS, fresh.msm_resident, 1, base_set=2)
    raises_rc(NOSRS, fresh.msm, sc, base_set=1)
    raises_rc(BADARG, fresh.bases_download, 1)


# ---------------- resident NTT: parity ----------------

@pytest.mark.parametrize("prof", [False, True], ids=["noprof", "prof"])
@pytest.mark.parametrize("k", [0, 1, 8, 9, 10, 16])
def test_ntt_resident_parity(gpu, k, prof):
    n = 1 << k
    data = rand_canon(random.Random(1000 + k), n)
    a = ints(data)
    fwd = oc.ntt(oc.FP, 0, k, data)
    calls = 0
    gpu.prof_enable(prof)
    try:
        gpu.prof_reset()
        gpu.poly_upload(data, k)
        gpu.ntt_resident(k)
        calls += 1
        first = gpu.poly_download(k)
        assert first == fwd
        assert gpu.poly_download(k) == first
        # the data stays resident: a second forward transform is n * a[-i]
        gpu.ntt_resident(k)
        calls += 1
        assert ints(gpu.poly_download(k)) == [n * a[(-i) % n] % P for i in range(n)]
        # forward then inverse, as the benchmark's step does
        gpu.poly_upload(data, k)
        for _ in range(5):
            gpu.ntt_resident(k, inverse=False)
            gpu.ntt_resident(k, inverse=True)
            calls += 2
        assert gpu.poly_download(k) == data
        # inverse on fresh data
        gpu.poly_upload(data, k)
        gpu.ntt_resident(k, inverse=True)
        calls += 1
        assert gpu.poly_download(k) == oc.ntt(oc.FP, 1, k, data)
        if prof:
            assert gpu.prof_get("ntt_total")[1] == calls == 13
            assert gpu.prof_get("msm_total")[1] == 0
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()


# ---------------- resident NTT: state ----------------

def test_ntt_state_and_argument_guards(gpu, fresh):
    raises_rc(STATE, fresh.ntt_resident, 4)
    raises_rc(STATE, fresh.poly_download, 4)
    raises_rc(STATE, fresh.ntt_resident, 0)
    raises_rc(STATE, fresh.poly_download, 0)

    rng = random.Random(1100)
    d4, d6 = rand_canon(rng, 16), rand_canon(rng, 64)
    gpu.poly_upload(d4, 4)
    raises_rc(STATE, gpu.ntt_resident, 5)
    raises_rc(STATE, gpu.poly_download, 5)
    raises_rc(STATE, gpu.ntt_resident, 3)
    raises_rc(STATE, gpu.poly_download, 3)
    # k above 28 is a bad argument; the raw call for the download, whose
    # wrapper sizes its host buffer from k
    small = ctypes.create_string_buffer(32)
    raises_rc(BADARG, gpu.ntt_resident, 29)
    raises_rc(BADARG, gpu.ntt_resident, 29, inverse=True)
    assert gpu._lib.tg_poly_download(gpu._h, small, 29) == BADARG
    assert gpu._lib.tg_poly_upload(gpu._h, d4, 29) == BADARG
    raises_rc(BADARG, gpu.ntt_resident, 0xFFFFFFFF)
    raises_rc(BADARG, gpu.ntt_resident, 0x80000000)
    assert small.raw == bytes(32)
    # none of that touched the resident polynomial
    assert gpu.poly_download(4) == d4

    # tg_ntt_fp of another size moves the resident size
    f6 = gpu.ntt(d6, 6)
    assert f6 == oc.ntt(oc.FP, 0, 6, d6)
    raises_rc(STATE, gpu.ntt_resident, 4)
    raises_rc(STATE, gpu.poly_download, 4)
    assert gpu.poly_download(6) == f6
    gpu.ntt_resident(6, inverse=True)
    assert gpu.poly_download(6) == d6

    # a rejected upload leaves no polynomial, of the same size or another
    for k_bad in (6, 4):
        n = 1 << k_bad
        good = d6 if k_bad == 6 else d4
        for pos in (0, n - 1):
            gpu.poly_upload(d6, 6)
            raises_rc(ENCODING, gpu.poly_upload, with_scalar(good, pos, P), k_bad)
            for k in (4, 6):
                raises_rc(STATE, gpu.ntt_resident, k)
                raises_rc(STATE, gpu.poly_download, k)
            raises_rc(ENCODING, gpu.ntt, with_scalar(good, pos, P), k_bad)
            raises_rc(STATE, gpu.poly_download, k_bad)

    # coset transforms are refused, and refusing leaves the data alone
    gpu.poly_upload(d4, 4)
    raises_rc(BADARG, gpu.ntt_resident, 4, coset=True)
    raises_rc(BADARG, gpu.ntt_resident, 4, inverse=True, coset=True)
    raises_rc(BADARG, gpu.ntt, d4, 4, coset=True)
    assert gpu.poly_download(4) == d4
    gpu.ntt_resident(4)
    assert gpu.poly_download(4) == oc.ntt(oc.FP, 0, 4, d4)
