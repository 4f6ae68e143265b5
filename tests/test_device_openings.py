"""The opening phase's device kernels (taiga_amd/csrc/openings.hip) on caller
data, through the diagnostic entry points of include/taiga_gpu.h: batched
polynomial evaluation, Kate division, Horner combination of vectors and the
IPA rounds. The reference is Python integers mod p, and the oracle MSM for
points. Everything is exact — there are no tolerances.

The evaluation and division kernels cut a vector into 512 per-thread chunks
(OPN_T); the lengths below sit on both sides of 256 and 512 and of the
production size 2^15, where the chunk length changes."""
import ctypes
import os
import random

import pytest

import oracle_ct as oc
import pypasta as pp
from conftest import REPO

pytestmark = pytest.mark.gpu

P = pp.P
N15 = 1 << 15
LENGTHS = [1, 2, 255, 256, 257, 511, 512, 513, 1000, N15 - 1, N15]


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def rand_canon(rng, n):
    """n canonical field reprs (< 2^254 < p) without a per-element loop"""
    raw = bytearray(rng.getrandbits(n * 256).to_bytes(n * 32, "little"))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    return bytes(raw)


@pytest.fixture(scope="module")
def params():
    return open(os.path.join(REPO, "tests", "golden", "params_15"), "rb").read()


@pytest.fixture(scope="module")
def gpu(params):
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params)
    yield g
    g.close()


@pytest.fixture(scope="module")
def coeffs():
    """2^15 random coefficients shared by the evaluation and division cases"""
    data = rand_canon(random.Random(1501), N15)
    return data, ints(data)


def horner(cs, x):
    acc = 0
    for c in reversed(cs):
        acc = (acc * x + c) % P
    return acc


def eval_batch(gpu, data, queries):
    """queries: (offset, length, point) over the elements of data"""
    nq = len(queries)
    offs = (ctypes.c_uint64 * nq)(*[q[0] for q in queries])
    lens = (ctypes.c_uint64 * nq)(*[q[1] for q in queries])
    pts = b"".join(b32(q[2]) for q in queries)
    out = ctypes.create_string_buffer(32 * nq)
    gpu._ck(gpu._lib.tg_fp_poly_eval_batch(gpu._h, data, len(data) // 32, offs, lens, pts,
                                           nq, out))
    return ints(out.raw)


def kate_div(gpu, data, points):
    buf = ctypes.create_string_buffer(data, len(data))
    gpu._ck(gpu._lib.tg_fp_kate_div(gpu._h, buf, len(data) // 32,
                                    b"".join(b32(p) for p in points), len(points)))
    return ints(buf.raw)


def kate_serial(a, pt):
    """the plain recurrence q[i-1] = a[i] + pt*q[i], remainder dropped; the
    result keeps a's length with a zero in the freed top slot"""
    q = [0] * len(a)
    prev = 0
    for i in range(len(a) - 1, 0, -1):
        prev = (a[i] + pt * prev) % P
        q[i - 1] = prev
    return q


# ---------------- evaluation ----------------

def test_eval_lengths_and_points(gpu, coeffs):
    """every length at every point, all in ONE launch: the batch mixes
    polynomials (different offsets) and lengths"""
    data, vals = coeffs
    rng = random.Random(7)
    points = [0, 1, P - 1, rng.randrange(P), rng.randrange(P)]
    queries = []
    for ln in LENGTHS:
        for i, x in enumerate(points):
            off = 0 if ln == N15 else min(N15 - ln, 37 * i)
            queries.append((off, ln, x))
    got = eval_batch(gpu, data, queries)
    for (off, ln, x), g in zip(queries, got):
        assert g == horner(vals[off:off + ln], x), (off, ln, x)


def test_eval_hundred_queries(gpu, coeffs):
    """100 queries in one call (no per-launch query limit), each its own
    sub-range and point"""
    data, vals = coeffs
    rng = random.Random(8)
    queries = []
    for _ in range(100):
        ln = rng.randrange(1, 700)
        queries.append((rng.randrange(0, N15 - ln), ln, rng.randrange(P)))
    got = eval_batch(gpu, data, queries)
    assert got == [horner(vals[o:o + ln], x) for o, ln, x in queries]


def test_eval_rejects_noncanonical_and_out_of_range(gpu, coeffs):
    import taiga_amd

    data, _ = coeffs
    with pytest.raises(taiga_amd.TaigaGpuError):
        eval_batch(gpu, b32(P) + data[32:64], [(0, 2, 1)])
    with pytest.raises(taiga_amd.TaigaGpuError):
        eval_batch(gpu, data[:64], [(1, 2, 1)])


# ---------------- Kate division ----------------

@pytest.mark.parametrize("ln", LENGTHS + [N15 - 2])
def test_kate_division(gpu, coeffs, ln):
    data, vals = coeffs
    a = vals[:ln]
    for pt in (0, 1, random.Random(ln).randrange(P)):
        q = kate_div(gpu, data[:32 * ln], [pt])
        assert q[ln - 1] == 0
        assert q == kate_serial(a, pt), (ln, pt)
        # q * (X - pt) + r = a, coefficient by coefficient, r = a(pt)
        r = horner(a, pt)
        assert (r - pt * q[0]) % P == a[0]
        for i in range(1, ln):
            assert (q[i - 1] - pt * q[i]) % P == a[i], (ln, pt, i)


def test_kate_constant_polynomial(gpu):
    assert kate_div(gpu, b32(12345), [7]) == [0]


@pytest.mark.parametrize("ln", [3, 257, 513, 1000, N15])
def test_kate_chain_of_three(gpu, coeffs, ln):
    """three divisions, the length dropping by one each time (multiopen)"""
    data, vals = coeffs
    rng = random.Random(100 + ln)
    pts = [rng.randrange(P) for _ in range(3)]
    want = vals[:ln]
    for j, pt in enumerate(pts):
        want = kate_serial(want[:ln - j], pt) + [0] * j
    assert kate_div(gpu, data[:32 * ln], pts) == want


# ---------------- Horner combination ----------------

def comb(gpu, polys, ch):
    n = len(polys[0])
    out = ctypes.create_string_buffer(32 * n)
    flat = b"".join(b32(v) for p in polys for v in p)
    gpu._ck(gpu._lib.tg_fp_horner_comb(gpu._h, flat, len(polys), n, b32(ch), out))
    return ints(out.raw)


@pytest.mark.parametrize("np_", [1, 2, 7])
def test_horner_comb(gpu, np_):
    rng = random.Random(40 + np_)
    n = 1000  # odd size, four blocks
    polys = [ints(rand_canon(rng, n)) for _ in range(np_)]
    for ch in (0, 1, rng.randrange(P)):
        want = [horner([p[i] for p in reversed(polys)], ch) for i in range(n)]
        assert comb(gpu, polys, ch) == want, (np_, ch)


def test_horner_comb_grid_stride(gpu):
    """longer than the launch's 2048 x 256 threads: the stride loop wraps"""
    rng = random.Random(44)
    n = 2048 * 256 + 5
    data = rand_canon(rng, 2 * n)
    vals = ints(data)
    ch = rng.randrange(P)
    out = ctypes.create_string_buffer(32 * n)
    gpu._ck(gpu._lib.tg_fp_horner_comb(gpu._h, data, 2, n, b32(ch), out))
    got = ints(out.raw)
    assert got == [(vals[i] * ch + vals[n + i]) % P for i in range(n)]


# ---------------- IPA rounds ----------------

def ipa_reference(k, poly, x3, us, blinds, blind, g_xy, u_xy, w_xy):
    """restatement of the prover's IPA loop: L_j / R_j as MSMs over the
    original bases with folded scalars, plus the U and W terms"""
    n = 1 << k
    pvec = list(poly)
    bvec = [pow(x3, i, P) for i in range(n)]
    wfold = [1] * n
    bases = g_xy[:64 * n] + u_xy + w_xy
    half = n >> 1
    lr = []
    for rnd in range(k):
        cur = 2 * half
        value_l = sum(pvec[half + i] * bvec[i] for i in range(half)) % P
        value_r = sum(pvec[i] * bvec[half + i] for i in range(half)) % P
        l_rand, r_rand = blinds[2 * rnd], blinds[2 * rnd + 1]
        sl, sr = [0] * n, [0] * n
        for t in range(n):
            ci = t & (cur - 1)
            if ci < half:
                sl[t] = wfold[t] * pvec[half + ci] % P
            else:
                sr[t] = wfold[t] * pvec[ci - half] % P
        for sc, val, rnd_blind in ((sl, value_l, l_rand), (sr, value_r, r_rand)):
            scal = b"".join(b32(v) for v in sc + [val, rnd_blind])
            lr.append(oc.msm(oc.FQ, scal, bases))
        u = us[rnd]
        ui = pow(u, -1, P)
        topbit = 1 << (k - 1 - rnd)
        for t in range(n):
            if t & topbit:
                wfold[t] = wfold[t] * ui % P
        for i in range(half):
            pvec[i] = (pvec[i] + pvec[half + i] * u) % P
            bvec[i] = (bvec[i] + bvec[half + i] * ui) % P
        blind = (blind + u * l_rand + ui * r_rand) % P
        half >>= 1
    return b"".join(lr), pvec[0], blind


@pytest.mark.parametrize("k", [1, 2, 5])
def test_ipa_probe(gpu, params, k):
    """k = 1 runs half = 1; k = 5 runs the topbit masking over several rounds"""
    n = 1 << k
    g_xy = oc.decompress(oc.FQ, params[4:4 + 32 * n])
    wu = oc.decompress(oc.FQ, params[4 + 64 * N15:4 + 64 * N15 + 64])
    w_xy, u_xy = wu[:64], wu[64:]
    rng = random.Random(900 + k)
    poly = [rng.randrange(P) for _ in range(n)]
    x3 = rng.randrange(P)
    us = [rng.randrange(1, P) for _ in range(k)]
    blinds = [rng.randrange(P) for _ in range(2 * k)]
    blind = rng.randrange(P)
    lr = ctypes.create_string_buffer(128 * k)
    a_out = ctypes.create_string_buffer(32)
    b_out = ctypes.create_string_buffer(32)
    gpu._ck(gpu._lib.tg_ipa_open_probe(
        gpu._h, k, b"".join(map(b32, poly)), b32(x3), b"".join(map(b32, us)),
        b"".join(map(b32, blinds)), b32(blind), lr, a_out, b_out))
    want_lr, want_a, want_blind = ipa_reference(k, poly, x3, us, blinds, blind, g_xy,
                                                u_xy, w_xy)
    assert lr.raw == want_lr
    assert ints(a_out.raw) == [want_a]
    assert ints(b_out.raw) == [want_blind]
