"""The device's field multiply and squaring (fd_mul_r30 / fd_sqr_r30 of
pasta_device.hpp) through the kernels that use them, on operands that sit on
the multiply's limb edges: batch inverse, batched polynomial evaluation and
the NTT for Fp, the MSM over uploaded bases (the safe addition) and over an
SRS set (the fixed-base chain) for Fq. Only existing entry points; every
expected value comes from Python integers and oracle/pypasta.py, and
everything is exact."""
import ctypes
import random

import pytest

import pypasta as pp
from fd_mul_cases import limb30_edge_values, limb_edge_values

pytestmark = pytest.mark.gpu

P = pp.P


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def seeded(mod, n, seed, nonzero=False):
    """n field elements: limb-edge values first (a spread of both limb
    widths), random ones after"""
    rng = random.Random(seed)
    edge = limb30_edge_values(mod) + limb_edge_values(mod)[::37]
    if nonzero:
        edge = [v for v in edge if v]
    rng.shuffle(edge)
    vals = edge[:n * 3 // 4]
    vals += [rng.randrange(1, mod) for _ in range(n - len(vals))]
    assert len(vals) == n and all(0 <= v < mod for v in vals)
    return vals


@pytest.fixture(scope="module")
def gpu(params15):
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    g.load_srs(params15)
    yield g
    g.close()


def test_batch_inverse_limb_edges(gpu):
    vals = seeded(P, 1024, 8801, nonzero=True)
    got = ints(gpu.fp_batch_inverse(b"".join(map(b32, vals))))
    assert got == [pow(v, -1, P) for v in vals]


def test_poly_eval_batch_limb_edges(gpu):
    coeffs = seeded(P, 64, 8802)
    points = seeded(P, 8, 8803)
    data = b"".join(map(b32, coeffs))
    nq = len(points)
    offs = (ctypes.c_uint64 * nq)(*([0] * nq))
    lens = (ctypes.c_uint64 * nq)(*([len(coeffs)] * nq))
    out = ctypes.create_string_buffer(32 * nq)
    gpu._ck(gpu._lib.tg_fp_poly_eval_batch(gpu._h, data, len(coeffs), offs, lens,
                                           b"".join(map(b32, points)), nq, out))
    exp = []
    for x in points:
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * x + c) % P
        exp.append(acc)
    assert ints(out.raw) == exp


def test_ntt_forward_inverse_limb_edges(gpu):
    k = 10
    vals = seeded(P, 1 << k, 8804)
    data = b"".join(map(b32, vals))
    fwd = gpu.ntt(data, k)
    assert ints(fwd) == pp.ntt(vals, pp.root_of_unity(P, k), P)
    assert gpu.ntt(fwd, k, inverse=True) == data


def xy(pt):
    return bytes(64) if pt.inf else b32(pt.x) + b32(pt.y)


def test_msm_uploaded_bases_limb_edges(gpu):
    """Coordinates in Fq; uploaded bases take the safe addition, which the
    repeated, negated and identity bases here exercise."""
    n = 512
    rng = random.Random(8805)
    G = pp.Point.generator(pp.Q)
    step = G.mul(rng.randrange(1, P))
    pts = [G.mul(rng.randrange(1, P))]
    while len(pts) < n:
        pts.append(pts[-1] + step)
    pts[7] = pts[3]
    pts[8] = -pts[3]
    pts[9] = pp.Point.identity(pp.Q)
    scalars = seeded(P, n, 8806)
    scalars[7] = scalars[3]  # equal points meet in one bucket
    scalars[8] = scalars[3]
    gpu.bases_upload(b"".join(map(xy, pts)))
    got = gpu.msm(b"".join(map(b32, scalars)), base_set=0)
    assert got == xy(pp.msm(scalars, pts))


def test_msm_srs_set_limb_edges(gpu, params15):
    n = 512
    pts = [pp.Point.from_bytes(params15[4 + 32 * i:36 + 32 * i], pp.Q) for i in range(n)]
    assert all(pt is not None and not pt.inf for pt in pts)
    scalars = seeded(P, n, 8807)
    got = gpu.msm(b"".join(map(b32, scalars)), base_set=1)
    assert got == xy(pp.msm(scalars, pts))
