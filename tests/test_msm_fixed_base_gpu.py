"""GPU tests of the fixed-base plan of msm_run (msm_plan_fixed): MSMs over the SRS
sets g (base_set 1) and g_lagrange (base_set 2) of tests/golden/params_15 run
over the window-shifted tables [2^(C*w)] G_j that tg_load_srs builds, with all
windows' digits in ONE bucket set. Every case is bit-exact against the CPU
oracle's MSM or scalar multiplication.

C and NWIN restate MSM_FB_C / msm_nwin of msm.hip (the host test
tests/test_msm_recode_host.py reads them from the code and pins them)."""
import ctypes
import random

import pytest

import oracle_ct as oc
import pypasta as pp
from conftest import REPO
from msm_fb_cases import edge_scalars

pytestmark = pytest.mark.gpu

P = pp.P
C = 16
NWIN = 255 // C + 1
NBUCK = 1 << (C - 1)
N15 = 1 << 15
ID64 = b"\x00" * 64
SETS = [1, 2]


def b32(v):
    return v.to_bytes(32, "little")


@pytest.fixture(scope="module")
def params():
    import os

    return open(os.path.join(REPO, "tests", "golden", "params_15"), "rb").read()


@pytest.fixture(scope="module")
def gpu(params):
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params)
    yield g
    g.close()


@pytest.fixture(scope="module")
def srs_xy(params):
    """the two SRS sets as canonical affine x||y, decompressed by the oracle"""
    return {1: oc.decompress(oc.FQ, params[4:4 + 32 * N15]),
            2: oc.decompress(oc.FQ, params[4 + 32 * N15:4 + 64 * N15])}


def check(gpu, srs_xy, bs, scal, exp=None):
    sc = b"".join(map(b32, scal))
    if exp is None:
        exp = oc.msm(oc.FQ, sc, srs_xy[bs][:64 * len(scal)])
    assert gpu.msm(sc, base_set=bs) == exp
    return exp


@pytest.mark.parametrize("bs", SETS)
def test_one_hot_every_window(gpu, srs_xy, bs):
    """scalar 2^(C*w) on base j alone reads table entry T[w][j]"""
    n = 64
    for w in range(NWIN):
        if C * w > 253:
            continue  # no canonical scalar reaches that window
        for j in (0, 1, n - 1):
            k = 1 << (C * w)
            exp = oc.msm(oc.FQ, b32(k), srs_xy[bs][64 * j:64 * j + 64])
            assert exp != ID64
            scal = [0] * n
            scal[j] = k
            check(gpu, srs_xy, bs, scal, exp=exp)
    assert C * (NWIN - 1) <= 253  # the top window was among them


@pytest.mark.parametrize("bs", SETS)
def test_recoding_edges(gpu, srs_xy, bs):
    n = 64
    edges = edge_scalars(C, NWIN)
    # each edge scalar alone (a wrong digit cannot hide behind another), on
    # the last base, then all of them together
    for s in edges:
        exp = ID64 if s == 0 else oc.msm(oc.FQ, b32(s), srs_xy[bs][64 * (n - 1):64 * n])
        check(gpu, srs_xy, bs, [0] * (n - 1) + [s], exp=exp)
    rng = random.Random(6100 + bs)
    scal = (edges + [rng.randrange(P) for _ in range(n)])[:n]
    assert len(edges) <= n
    assert check(gpu, srs_xy, bs, scal) != ID64


@pytest.mark.parametrize("bs", SETS)
def test_every_bucket_index_twice(gpu, srs_xy, bs):
    """point i puts digit i+1 into one window and digit ((i + NBUCK/2) mod
    NBUCK) + 1 into another: every bucket of the single set holds exactly two
    table points, of differing windows, and a wrong weight on any one bucket
    changes the result. Digits are at most 2^(C-1), so never recoded."""
    n = NBUCK
    wins = [w for w in range(NWIN) if C * w + C <= 253]
    assert n <= N15 and len(wins) >= 2
    scal, count = [], [0] * NBUCK
    for i in range(n):
        w1 = wins[i % len(wins)]
        w2 = wins[(i % len(wins) + 1 + (i // len(wins)) % (len(wins) - 1)) % len(wins)]
        assert w1 != w2
        d1, d2 = i + 1, (i + NBUCK // 2) % NBUCK + 1
        count[d1 - 1] += 1
        count[d2 - 1] += 1
        scal.append((d1 << (C * w1)) + (d2 << (C * w2)))
    assert count == [2] * NBUCK and max(scal) < 1 << 253
    assert check(gpu, srs_xy, bs, scal) != ID64


@pytest.mark.parametrize("bs", SETS)
def test_ipa_shape_halves(gpu, srs_xy, bs):
    """the vectors k_ipa_prepare writes: one half of the scalars zero"""
    n = 1 << 12
    rng = random.Random(6200 + bs)
    v = [rng.randrange(P) for _ in range(n)]
    lo = v[:n // 2] + [0] * (n // 2)
    hi = [0] * (n // 2) + v[n // 2:]
    a = check(gpu, srs_xy, bs, lo)
    b = check(gpu, srs_xy, bs, hi)
    assert a != b and ID64 not in (a, b)


def ipa_reference(k, poly, x3, us, blinds, blind, g_xy, u_xy, w_xy):
    """the prover's IPA loop restated: L_j / R_j as MSMs over the original
    bases with folded scalars (complementary halves zero), plus the U and W
    terms"""
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
            scal = b"".join(b32(x) for x in sc + [val, rnd_blind])
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


def test_ipa_rounds_batch_of_two(gpu, params, srs_xy):
    """tg_ipa_open_probe at k = 12: every round is one batch of 2 MSMs over
    the first 2^12 points of g, a prefix of the table's 2^15 stride"""
    k = 12
    n = 1 << k
    wu = oc.decompress(oc.FQ, params[4 + 64 * N15:4 + 64 * N15 + 64])
    w_xy, u_xy = wu[:64], wu[64:]
    rng = random.Random(6300)
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
    want_lr, want_a, want_blind = ipa_reference(k, poly, x3, us, blinds, blind,
                                                srs_xy[1], u_xy, w_xy)
    assert lr.raw == want_lr
    assert int.from_bytes(a_out.raw, "little") == want_a
    assert int.from_bytes(b_out.raw, "little") == want_blind


@pytest.mark.parametrize("bs", SETS)
def test_heavy_duplication(gpu, srs_xy, bs):
    """buckets longer than MSM_BIG_BUCKET = 64 go to k_bucket_acc_big; one
    bucket of exactly 64 stays with k_bucket_acc, one of exactly 65 does not"""
    n = 1 << 12
    rng = random.Random(6400 + bs)
    assert check(gpu, srs_xy, bs, [1] * n) != ID64
    assert check(gpu, srs_xy, bs, [rng.choice((0, 1, 255)) for _ in range(n)]) != ID64
    for equal in (64, 65):
        # the others take distinct single-digit values, one bucket each
        scal = [7] * equal + [8 + i for i in range(n - equal)]
        assert max(scal) <= NBUCK
        rng.shuffle(scal)
        assert check(gpu, srs_xy, bs, scal) != ID64


@pytest.mark.parametrize("bs", SETS)
def test_full_size_and_prefixes(gpu, srs_xy, bs):
    rng = random.Random(6500 + bs)
    scal = [rng.randrange(P) for _ in range(N15)]
    full = check(gpu, srs_xy, bs, scal)
    part = check(gpu, srs_xy, bs, scal[:N15 - 1])
    one = check(gpu, srs_xy, bs, scal[:1])
    assert len({full, part, one, ID64}) == 4


@pytest.mark.parametrize("which", [0, 1])
def test_load_rejects_table_collision(params, which):
    """G_1 = [2^C] G_0 in g (which = 0) or g_lagrange (1): every point is
    valid and the set's x coordinates stay distinct, so the per-set check
    passes, but table entries T[1][0] and T[0][1] are the same point"""
    import taiga_amd

    off = 4 + 32 * N15 * which
    g0 = oc.decompress(oc.FQ, params[off:off + 32])
    g1 = oc.msm(oc.FQ, b32(1 << C), g0)
    enc = oc.compress(oc.FQ, g1)
    assert len(enc) == 32 and oc.decompress(oc.FQ, enc) == g1
    blob = bytearray(params)
    blob[off + 32:off + 64] = enc
    # all 2^15 encodings of the set still differ in x
    xs = {bytes(blob[off + 32 * i:off + 32 * i + 31]) + bytes([blob[off + 32 * i + 31] & 0x7F])
          for i in range(N15)}
    assert len(xs) == N15
    g = taiga_amd.TaigaGpu(0)
    try:
        with pytest.raises(taiga_amd.api.TaigaGpuError) as ei:
            g.load_srs(bytes(blob))
        assert ei.value.rc == -3  # TG_ERR_ENCODING
        with pytest.raises(taiga_amd.api.TaigaGpuError) as ei:
            g.srs_k
        assert ei.value.rc == -4  # TG_ERR_NOSRS
        with pytest.raises(taiga_amd.api.TaigaGpuError) as ei:
            g.msm(b32(1), base_set=1 + which)
        assert ei.value.rc == -4
        # the context is usable again after a good load
        g.load_srs(params)
        assert g.srs_k == 15
        assert g.msm(b32(1), base_set=1 + which) == g0
    finally:
        g.close()
