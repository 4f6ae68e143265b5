"""GPU tests of the MSM bucket reduction (k_bucket_segsum, k_window_sum):
scalars built so that every bucket index of a window is occupied and a wrong
weight for any single bucket changes the result, sparse inputs whose partial
sums are mostly the identity, and sequential-multiple bases whose partial
sums collide (P+P, P+(-P)) at the two widest prover windows. At the smallest
n that selects each window width, on both accumulation paths. Bit-exact
against the CPU oracle or against one scalar multiplication."""
import random

import pytest

import oracle_ct as oc
import pypasta as pp
from kernel_shapes import expected_msm_cfg

pytestmark = pytest.mark.gpu

P, Q = pp.P, pp.Q
G = pp.Point.generator(Q)
ID64 = b"\x00" * 64
BASE_SEED = 4242

SHAPES = [(1 << 10, 8), (1 << 11, 9), (1 << 12, 10), (1 << 13, 11), (1 << 14, 12),
          (1 << 15, 13), (1 << 18, 16)]


@pytest.fixture(scope="module")
def gpu():
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def bases(gpu):
    """2^18 device-generated bases, downloaded once; gen_bases(n, seed) is a
    prefix of gen_bases(m > n, seed)."""
    n = 1 << 18
    gpu.gen_bases(n, BASE_SEED)
    return gpu.bases_download(n)


def b32(v):
    return v.to_bytes(32, "little")


def pt_bytes(pt):
    return ID64 if pt.inf else b32(pt.x) + b32(pt.y)


def both_paths(gpu, bases, sc):
    n = len(sc) // 32
    gpu.gen_bases(n, BASE_SEED)
    fast = gpu.msm(sc, base_set=0)
    gpu.bases_upload(bases[:64 * n])
    safe = gpu.msm(sc, base_set=0)
    return fast, safe


def check_both_paths(gpu, bases, sc, exp=None):
    fast, safe = both_paths(gpu, bases, sc)
    if exp is None:
        exp = oc.msm(oc.FQ, sc, bases[:len(sc) * 2])
    assert fast == exp, "branch-free accumulation path"
    assert safe == exp, "safe accumulation path"
    return exp


def low_windows(cfg):
    """windows in which a digit of up to nbuck keeps the scalar below 2^253"""
    return [w for w in range(cfg.nwin) if cfg.c * w + cfg.c <= 253]


def every_bucket_scalars(n, cfg):
    """scalar i = ((i mod nbuck) + 1) << (c * w_i): digit (i mod nbuck) + 1,
    at most 2^(c-1) and so never recoded, lands point i in bucket
    i mod nbuck of window w_i. The n / nbuck runs of indices go to windows
    spread from the lowest to the highest usable one."""
    wins = low_windows(cfg)
    runs = n // cfg.nbuck
    assert runs >= 2 and len(wins) >= runs
    out, used = [], set()
    for i in range(n):
        w = wins[(i // cfg.nbuck) * (len(wins) - 1) // (runs - 1)]
        used.add(w)
        out.append(((i % cfg.nbuck) + 1) << (cfg.c * w))
    assert len(used) == runs and max(out) < 1 << 253
    return out


@pytest.mark.parametrize("n,c", SHAPES)
def test_every_bucket_index_both_paths(gpu, bases, n, c):
    cfg = expected_msm_cfg(n)
    assert cfg.c == c
    scal = every_bucket_scalars(n, cfg)
    exp = check_both_paths(gpu, bases, b"".join(map(b32, scal)))
    assert exp != ID64


@pytest.mark.parametrize("n,c", SHAPES)
def test_sparse_scalars_both_paths(gpu, bases, n, c):
    cfg = expected_msm_cfg(n)
    assert cfg.c == c
    # all zero: every bucket, segment and window sum is the identity
    check_both_paths(gpu, bases, bytes(32 * n), exp=ID64)
    # one non-zero scalar: one bucket per window, the rest identity
    rng = random.Random(3100 + c)
    sc = bytearray(32 * n)
    at = rng.randrange(n)
    k = rng.randrange(1, P)
    sc[32 * at:32 * at + 32] = b32(k)
    one = oc.msm(oc.FQ, b32(k), bases[64 * at:64 * at + 64])
    assert one != ID64
    check_both_paths(gpu, bases, bytes(sc), exp=one)
    # only the top window: all lower windows are whole windows of identities
    shift = cfg.c * (cfg.nwin - 1)
    dmax = (P - 1) >> shift
    assert dmax >= 1
    top = b"".join(b32((1 + i % dmax) << shift) for i in range(n))
    assert check_both_paths(gpu, bases, top) != ID64


@pytest.fixture(scope="module")
def multiples():
    """[i]G for i = 0..2^15 (running addition)."""
    out = [pp.Point.identity(Q)]
    for _ in range(1 << 15):
        out.append(out[-1] + G)
    return out


@pytest.mark.parametrize("n,c", [(1 << 14, 12), (1 << 15, 13)])
def test_sequential_multiples_safe_path(gpu, multiples, n, c):
    """Bases [i+1]G on the safe path: bucket sums, segment sums, plane sums
    and window sums are small multiples of G that keep meeting each other
    (P+P, P+(-P), identity operands). Expected from the known multiples."""
    cfg = expected_msm_cfg(n)
    assert cfg.c == c
    gpu.bases_upload(b"".join(pt_bytes(p) for p in multiples[1:n + 1]))
    rng = random.Random(3200 + c)
    cases = [
        [rng.randrange(1, 300) for _ in range(n)],
        [rng.randrange(P) for _ in range(n)],
        every_bucket_scalars(n, cfg),
    ]
    # scalars summing to zero against the multiples: the identity
    scal = [rng.randrange(1, 300) for _ in range(n - 1)]
    part = sum(s * (i + 1) for i, s in enumerate(scal))
    scal.append(-part * pow(n, -1, P) % P)
    cases.append(scal)
    for j, scal in enumerate(cases):
        total = sum(s * (i + 1) for i, s in enumerate(scal)) % P
        got = gpu.msm(b"".join(map(b32, scal)), base_set=0)
        assert got == pt_bytes(G.mul(total)), j
    assert total == 0
