"""GPU tests aimed at the launch shapes and operand edges the parity suite
(test_gpu_parity.py) does not reach: every MSM window width on both
accumulation paths, digit and bucket-length boundaries, exceptional point
additions, every NTT pass shape, Poseidon's grid-stride loop, and SRS
decompression including degenerate SRS files. Everything is bit-exact.

kernel_shapes.py mirrors msm_cfg() and ntt_run(); test_host_arith.py pins the
MSM mirror to the compiled code, so the asserts on `c` below are meaningful."""
import ctypes
import random
import struct

import pytest

import oracle_ct as oc
import pypasta as pp
from kernel_shapes import (MSM_BIG_BUCKET, MSM_BIG_LANES, edge_values, expected_msm_cfg,
                           expected_ntt_passes, signed_digits)

pytestmark = pytest.mark.gpu

P, Q = pp.P, pp.Q
G = pp.Point.generator(Q)
ID64 = b"\x00" * 64
BASE_SEED = 4242


@pytest.fixture(scope="module")
def gpu():
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)
    yield g
    g.close()


def gpu_error():
    import taiga_amd

    return taiga_amd.TaigaGpuError


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def rand_canon(rng, n):
    """n canonical field reprs: 256 random bits with the top two cleared
    (< 2^254 < p), without a Python loop over the elements."""
    raw = bytearray(rng.getrandbits(n * 256).to_bytes(n * 32, "little"))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    return bytes(raw)


def pt_bytes(pt):
    return ID64 if pt.inf else b32(pt.x) + b32(pt.y)


# ---------------- MSM: shared inputs and references ----------------

MSM_NS = [1 << 11, 1 << 12, 1 << 13, 1 << 14, 1 << 15, (1 << 18) - 1, 1 << 18]
MSM_CS = [9, 10, 11, 12, 13, 13, 16]


@pytest.fixture(scope="module")
def bases(gpu):
    """2^18 device-generated bases, downloaded once. gen_bases(n, seed) is a
    prefix of gen_bases(m > n, seed), so every size slices this."""
    n = 1 << 18
    gpu.gen_bases(n, BASE_SEED)
    return gpu.bases_download(n)


_msm_cases = {}


def msm_case(n, bases):
    """(scalars, oracle result) for the size-n random case; computed once."""
    if n not in _msm_cases:
        sc = rand_canon(random.Random(7000 + n), n)
        _msm_cases[n] = (sc, oc.msm(oc.FQ, sc, bases[:64 * n]))
    return _msm_cases[n]


def both_paths(gpu, bases, sc):
    """MSM over the first len(sc)/32 generated bases on the branch-free path
    (device-generated bases) and on the safe path (the same bytes uploaded)."""
    n = len(sc) // 32
    gpu.gen_bases(n, BASE_SEED)
    fast = gpu.msm(sc, base_set=0)
    gpu.bases_upload(bases[:64 * n])
    safe = gpu.msm(sc, base_set=0)
    return fast, safe


def check_both_paths(gpu, bases, sc):
    fast, safe = both_paths(gpu, bases, sc)
    exp = oc.msm(oc.FQ, sc, bases[:len(sc) * 2])
    assert fast == exp, "branch-free accumulation path"
    assert safe == exp, "safe accumulation path"
    assert exp != ID64


@pytest.mark.parametrize("n,c", list(zip(MSM_NS, MSM_CS)))
def test_msm_every_window_width_both_paths(gpu, bases, n, c):
    assert expected_msm_cfg(n).c == c
    sc, exp = msm_case(n, bases)
    fast, safe = both_paths(gpu, bases, sc)
    assert fast == exp, "branch-free accumulation path"
    assert safe == exp, "safe accumulation path"


def boundary_scalars(c, nwin):
    mask = (1 << 254) - 1
    out = []
    for d in ((1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1):
        v = sum(d << (c * w) for w in range(nwin))
        for rot in (0, 1, c // 2, c - 1):
            out.append((v << rot) & mask)
    out += [P - 1, P - 2, (1 << 254) - 1, 1 << 254]
    for w in range(nwin):
        for bit in (w * c, w * c + c - 1):
            if bit <= 253:
                out.append(1 << bit)
    assert all(0 < s < P for s in out)
    return out


@pytest.mark.parametrize("n,c", [(1 << 10, 8), (1 << 11, 9), (1 << 12, 10), (1 << 13, 11),
                                 (1 << 14, 12), (1 << 15, 13), (1 << 18, 16)])
def test_msm_digit_boundaries(gpu, bases, n, c):
    """Window values 2^(c-1)-1, 2^(c-1), 2^(c-1)+1 and 2^c-1 in every window
    (the last ripples a carry through all of them), the largest canonical
    scalars, and single bits at each window's first and last position, at the
    smallest n that selects each c. The patterns replace the leading scalars
    of the random vector (64 to 84 of them, depending on nwin)."""
    cfg = expected_msm_cfg(n)
    assert cfg.c == c
    pats = boundary_scalars(c, cfg.nwin)
    # the patterns do reach the boundary digits
    digs = {d for s in pats for d in signed_digits(s, c, cfg.nwin)[0]}
    half = 1 << (c - 1)
    assert {half, half - 1, -(half - 1), -1, 1} <= digs
    sc = bytearray(msm_case(n, bases)[0])
    sc[:32 * len(pats)] = b"".join(b32(s) for s in pats)
    check_both_paths(gpu, bases, bytes(sc))


BUCKET_POOLS = {
    # name: (pool size m, repeats of each pool value, extra random scalars,
    #        a bucket length that must occur)
    "len64": (64, 64, 0, 64),
    "len65": (63, 65, 1, 65),
    "len128": (32, 128, 0, 128),
    "len204": (20, 204, 16, 204),
    "len256": (16, 256, 0, 256),
    "len273": (15, 273, 1, 273),
    "len585": (7, 585, 1, 585),
}


@pytest.mark.parametrize("name", sorted(BUCKET_POOLS))
def test_msm_bucket_lengths(gpu, bases, name):
    """n = 4096 (c = 10) with scalars repeated from a small pool, so bucket
    lengths are exact: 64 (the last thread-per-bucket length), 65 (the first
    block-per-bucket length), big buckets shorter than the 256-lane block
    (lanes without a point), exactly 256, and longer."""
    m, rep, extra, want_len = BUCKET_POOLS[name]
    n = 4096
    assert m * rep + extra == n
    cfg = expected_msm_cfg(n)
    assert cfg.c == 10 and MSM_BIG_BUCKET == 64 and MSM_BIG_LANES == 256
    rng = random.Random(8000 + m)
    pool = []
    while len(pool) < m:
        v = rng.randrange(1, P)
        if v not in pool:
            pool.append(v)
    vals = [pool[i % m] for i in range(m * rep)] + [rng.randrange(1, P) for _ in range(extra)]
    counts = {}
    for s in vals:
        for w, d in enumerate(signed_digits(s, cfg.c, cfg.nwin)[0]):
            if d:
                counts[(w, abs(d))] = counts.get((w, abs(d)), 0) + 1
    lens = set(counts.values())
    assert want_len in lens  # (pool values sharing a digit add longer ones)
    check_both_paths(gpu, bases, b"".join(b32(s) for s in vals))


def test_msm_skewed_scalars_safe_path(gpu, params15):
    """test_msm_skewed_scalars on uploaded bases: the safe block-per-bucket
    kernel with one bucket of ~2^15 points per window."""
    n = 1 << 15
    rng = random.Random(555)
    v = rng.randrange(P)
    sc = b"".join(b32(v if i > 100 else rng.randrange(P)) for i in range(n))
    g = oc.decompress(oc.FQ, params15[4:4 + 32 * n])
    gpu.bases_upload(g)
    assert gpu.msm(sc, base_set=0) == oc.msm(oc.FQ, sc, g)


# ---- exceptional additions, checked against one scalar multiplication ----

@pytest.fixture(scope="module")
def multiples():
    """[i]G for i = 0..512 (running addition)."""
    out = [pp.Point.identity(Q)]
    for _ in range(512):
        out.append(out[-1] + G)
    return out


def check_known_multiples(gpu, mults, pts, scal):
    """bases [mults[i]]G are uploaded (safe path); the MSM must be
    [sum scal[i] * mults[i]]G, by one multiplication and by the oracle."""
    pb = b"".join(pt_bytes(p) for p in pts)
    sb = b"".join(b32(s) for s in scal)
    gpu.bases_upload(pb)
    got = gpu.msm(sb, base_set=0)
    total = sum(s * m for s, m in zip(scal, mults)) % P
    want = pt_bytes(G.mul(total))
    assert oc.msm(oc.FQ, sb, pb) == want
    assert got == want
    return total


def test_msm_sequential_multiples(gpu, multiples):
    """Bases [i+1]G make bucket sums collide with later points all the time:
    P+P, P+(-P) and identity operands in the accumulation, the segment
    reduce, the window sums and the host combine."""
    n = 512
    assert expected_msm_cfg(n).c == 8
    mults = list(range(1, n + 1))
    pts = multiples[1:]
    rng = random.Random(91)
    check_known_multiples(gpu, mults, pts, [rng.randrange(1, 300) for _ in range(n)])
    check_known_multiples(gpu, mults, pts, [rng.randrange(P) for _ in range(n)])
    # scalars summing to zero: the result is the identity
    scal = [rng.randrange(P) for _ in range(n - 1)]
    part = sum(s * m for s, m in zip(scal, mults))
    scal.append(-part * pow(n, -1, P) % P)
    assert check_known_multiples(gpu, mults, pts, scal) == 0
    scal = [rng.randrange(1, 300) for _ in range(n - 1)]
    part = sum(s * m for s, m in zip(scal, mults))
    scal.append(-part * pow(n, -1, P) % P)
    assert check_known_multiples(gpu, mults, pts, scal) == 0


def test_msm_point_and_negation_same_scalar(gpu, multiples):
    n = 512
    rng = random.Random(92)
    mults = list(range(1, n + 1))
    pts = list(multiples[1:])
    scal = [rng.randrange(P) for _ in range(n)]
    for i in (0, 100, 510):  # base i+1 := -(base i), under the same scalar
        mults[i + 1] = -mults[i]
        pts[i + 1] = -pts[i]
        scal[i + 1] = scal[i]
    check_known_multiples(gpu, mults, pts, scal)
    # nothing but such pairs: identity
    mults = [(i // 2 + 1) * (-1) ** i for i in range(n)]
    pts = [multiples[i // 2 + 1] if i % 2 == 0 else -multiples[i // 2 + 1] for i in range(n)]
    scal = [scal[i // 2] for i in range(n)]
    assert check_known_multiples(gpu, mults, pts, scal) == 0


def test_msm_all_bases_equal(gpu, multiples):
    n = 512
    rng = random.Random(93)
    check_known_multiples(gpu, [7] * n, [multiples[7]] * n,
                          [rng.randrange(P) for _ in range(n)])
    check_known_multiples(gpu, [7] * n, [multiples[7]] * n,
                          [rng.randrange(1, 300) for _ in range(n)])
    # one scalar everywhere: a single bucket per window holding 512 equal points
    check_known_multiples(gpu, [7] * n, [multiples[7]] * n, [rng.randrange(P)] * n)


def test_msm_workspace_reuse(gpu, bases):
    """c = 16, then c = 9, then c = 16 again on one context: the second large
    run must not see anything the small one left in the shared workspace."""
    big, small = 1 << 18, 1 << 11
    assert expected_msm_cfg(big).c == 16 and expected_msm_cfg(small).c == 9
    sc_big, exp_big = msm_case(big, bases)
    sc_small, exp_small = msm_case(small, bases)
    gpu.gen_bases(big, BASE_SEED)
    first = gpu.msm(sc_big, base_set=0)
    assert gpu.msm(sc_small, base_set=0) == exp_small
    third = gpu.msm(sc_big, base_set=0)
    assert third == first
    assert first == exp_big


# ---------------- NTT ----------------

def omega(k):
    w = int.from_bytes(oc.get_omega(oc.FP, k), "little")
    if k:
        assert pow(w, 1 << (k - 1), P) == P - 1
    else:
        assert w == 1
    return w


@pytest.mark.parametrize("k", range(22))
def test_ntt_every_size_forward_and_inverse(gpu, k):
    # kernel_shapes.py lists what each k launches; the shapes this test is for:
    names = [name for name, _ in expected_ntt_passes(k)]
    if k in (7, 13, 20):
        assert "k_ntt_fused2<4,8>" in names
    if k in (8, 14, 21):
        assert "k_ntt_fused2<5,8>" in names
    if k == 21:  # more than 2048 tiles: the first pass loops over tiles
        assert ("k_ntt_fused_br<9>", True) in expected_ntt_passes(k)
    if k == 20:
        assert ("k_ntt_fused_br<9>", False) in expected_ntt_passes(k)
    data = rand_canon(random.Random(5000 + k), 1 << k)
    assert gpu.ntt(data, k) == oc.ntt(oc.FP, 0, k, data)
    assert gpu.ntt(data, k, inverse=True) == oc.ntt(oc.FP, 1, k, data)


def test_ntt_forward_parity_k22(gpu):
    k = 22
    assert ("k_ntt_fused_br<9>", True) in expected_ntt_passes(k)
    data = rand_canon(random.Random(5022), 1 << k)
    assert gpu.ntt(data, k) == oc.ntt(oc.FP, 0, k, data)


@pytest.mark.parametrize("k", [20, 21, 22])
def test_ntt_geometric_closed_form(gpu, k):
    """a_i = c^i transforms to (c^n - 1) / (c w^j - 1): a full-size check
    that needs no oracle."""
    n = 1 << k
    w = omega(k)
    rng = random.Random(6000 + k)
    c = rng.randrange(2, P)
    data = bytearray()
    x = 1
    for _ in range(n >> 16):  # running product, joined in chunks to bound memory
        chunk = []
        for _ in range(1 << 16):
            chunk.append(x.to_bytes(32, "little"))
            x = x * c % P
        data += b"".join(chunk)
    cn = x  # c^n
    assert cn == pow(c, n, P) and cn != 1
    got = gpu.ntt(bytes(data), k)
    del data
    idx = {0, n - 1}
    idx.update(rng.randrange(n) for _ in range(2000))
    for tile in range(0, n >> 9, 2048):  # 512-element tiles, grid of 2048
        idx.update((tile << 9, (tile << 9) + 511))
    for j in sorted(idx):
        den = (c * pow(w, j, P) - 1) % P
        assert den
        want = (cn - 1) * pow(den, -1, P) % P
        assert int.from_bytes(got[32 * j:32 * j + 32], "little") == want, j


def dft(vals, w):
    n = len(vals)
    pw = [pow(w, i, P) for i in range(n)]
    return [sum(a * pw[i * j % n] for i, a in enumerate(vals)) % P for j in range(n)]


@pytest.mark.parametrize("k", [1, 6, 10])
def test_ntt_edge_operands(gpu, k):
    n = 1 << k
    ev = edge_values(P)
    for shift in (0, 1, 7):
        vals = [ev[(i + shift) % len(ev)] for i in range(n)]
        data = b"".join(map(b32, vals))
        fwd = gpu.ntt(data, k)
        inv = gpu.ntt(data, k, inverse=True)
        assert fwd == oc.ntt(oc.FP, 0, k, data)
        assert inv == oc.ntt(oc.FP, 1, k, data)
        if k <= 6:
            w = omega(k)
            assert ints(fwd) == dft(vals, w)
            ninv = pow(n, -1, P)
            assert ints(inv) == [v * ninv % P for v in dft(vals, pow(w, -1, P))]


def test_ntt_size2_every_edge_pair(gpu):
    ev = edge_values(P)
    half = pow(2, -1, P)
    assert any((a + b) % P == 0 and a for a in ev for b in ev)
    for a in ev:
        for b in ev:
            data = b32(a) + b32(b)
            assert ints(gpu.ntt(data, 1)) == [(a + b) % P, (a - b) % P], (a, b)
            assert ints(gpu.ntt(data, 1, inverse=True)) == [
                (a + b) * half % P, (a - b) * half % P], (a, b)


# ---------------- Poseidon ----------------

def poseidon_ref(msgs, n, L):
    lib = oc.lib()
    out = ctypes.create_string_buffer(32)
    res = bytearray()
    for i in range(n):
        assert lib.orc_poseidon_hash(msgs[32 * L * i:32 * L * (i + 1)], L, out) == 0
        res += out.raw
    return bytes(res)


@pytest.mark.parametrize("L,n", [(1, 257), (2, 1000), (3, 64), (5, 64), (9, 300), (64, 8)])
def test_poseidon_every_digest(gpu, L, n):
    rng = random.Random(9000 + L)
    msgs = b"".join(b32(rng.randrange(P)) for _ in range(n * L))
    assert gpu.poseidon_hash(msgs, n, L) == poseidon_ref(msgs, n, L)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 64])
def test_poseidon_zero_and_pm1_messages(gpu, L):
    rng = random.Random(9100 + L)
    z, m = b32(0), b32(P - 1)
    batch = [z * L, m * L]
    for _ in range(30):
        batch.append(b"".join(rng.choice((z, m)) for _ in range(L)))
    if L <= 3:  # every combination
        batch += [b"".join(m if (bits >> i) & 1 else z for i in range(L))
                  for bits in range(1 << L)]
    msgs = b"".join(batch)
    assert gpu.poseidon_hash(msgs, len(batch), L) == poseidon_ref(msgs, len(batch), L)


def test_poseidon_grid_stride(gpu):
    """tg_poseidon_hash launches at most 16384 blocks of 256 threads, one
    hash per thread per trip: a batch larger than that runs the kernel's
    grid-stride loop. Messages repeat with period 1024."""
    threads = 16384 * 256
    n = threads + 1024 + 37
    period = 1024
    rng = random.Random(9200)
    base = b"".join(b32(rng.randrange(P)) for _ in range(period))
    msgs = base * (n // period) + base[:32 * (n % period)]
    got = gpu.poseidon_hash(msgs, n, 1)
    first = got[:32 * period]
    assert first == poseidon_ref(base, period, 1)
    assert len(set(first[i:i + 32] for i in range(0, len(first), 32))) == period
    assert got == first * (n // period) + first[:32 * (n % period)]


@pytest.mark.parametrize("L", [0, 65])
def test_poseidon_rejects_bad_length(gpu, L):
    with pytest.raises(gpu_error()):
        gpu.poseidon_hash(bytes(32 * max(L, 1)), 1, L)


# ---------------- SRS decompression and degenerate SRS ----------------

def splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


SRS_SEED = 77


@pytest.fixture(scope="module")
def srs_points():
    """1026 distinct points [k_i]G with k_i known (the splitmix64 derivation
    of gen_bases); every third one negated so both signs of y occur."""
    raw = oc.gen_bases(1026, SRS_SEED)
    for i in (0, 513, 1025):
        k = sum(splitmix64((SRS_SEED * 0xD1B54A32D192ED03 + 4 * i + j) & (2**64 - 1)) << (64 * j)
                for j in range(4))
        assert raw[64 * i:64 * i + 64] == pt_bytes(G.mul(k % P))
    pts = []
    for i in range(1026):
        x = int.from_bytes(raw[64 * i:64 * i + 32], "little")
        y = int.from_bytes(raw[64 * i + 32:64 * i + 64], "little")
        pts.append((x, Q - y if i % 3 == 0 else y))
    assert len({x for x, _ in pts}) == len(pts)
    assert {y & 1 for _, y in pts} == {0, 1}
    return pts


def xy_bytes(pts):
    return b"".join(b32(x) + b32(y) for x, y in pts)


def srs_blob(k, g, gl, w, u, k_field=None):
    """the params file format: k (u32 LE), g, g_lagrange, w, u compressed"""
    enc = oc.compress(oc.FQ, xy_bytes(g + gl + [w, u]))
    return struct.pack("<I", k if k_field is None else k_field) + enc


def srs_parts(srs_points, k):
    n = 1 << k
    return (srs_points[:n], srs_points[512:512 + n], srs_points[1024], srs_points[1025])


@pytest.mark.parametrize("k", [0, 1, 4, 9])
def test_srs_synthetic_roundtrip(gpu, srs_points, k):
    n = 1 << k
    g, gl, w, u = srs_parts(srs_points, k)
    gpu.load_srs(srs_blob(k, g, gl, w, u))
    assert gpu.srs_k == k
    for base_set, pts in ((1, g), (2, gl)):
        for i in range(n):
            sc = bytearray(32 * n)
            sc[32 * i] = 1
            assert gpu.msm(bytes(sc), base_set=base_set) == xy_bytes([pts[i]]), (base_set, i)
        sc = rand_canon(random.Random(9300 + k + base_set), n)
        assert gpu.msm(sc, base_set=base_set) == oc.msm(oc.FQ, sc, xy_bytes(pts))


def bad_x_encodings():
    x = 1
    while pow((x**3 + 5) % Q, (Q - 1) // 2, Q) == 1:
        x += 1
    return {"no_sqrt": b32(x), "x_eq_modulus": b32(Q), "zero_with_sign": b32(1 << 255)}


@pytest.mark.parametrize("what", ["no_sqrt", "x_eq_modulus", "zero_with_sign"])
@pytest.mark.parametrize("where", ["g", "g_lagrange", "w", "u"])
def test_srs_rejects_bad_encoding(gpu, srs_points, what, where):
    k, n = 4, 16
    blob = bytearray(srs_blob(k, *srs_parts(srs_points, k)))
    ofs = {"g": 4 + 32 * 5, "g_lagrange": 4 + 32 * (n + 11), "w": 4 + 64 * n,
           "u": 4 + 64 * n + 32}[where]
    blob[ofs:ofs + 32] = bad_x_encodings()[what]
    with pytest.raises(gpu_error()):
        gpu.load_srs(bytes(blob))


def test_srs_rejects_bad_framing(gpu, srs_points):
    k = 4
    blob = srs_blob(k, *srs_parts(srs_points, k))
    for bad in (blob[:-1], blob + b"\x00", blob[:4], blob[:3],
                srs_blob(k, *srs_parts(srs_points, k), k_field=29),
                srs_blob(k, *srs_parts(srs_points, k), k_field=3)):
        with pytest.raises(gpu_error()):
            gpu.load_srs(bad)


def expect_degenerate(gpu, blob):
    with pytest.raises(gpu_error()) as ei:
        gpu.load_srs(blob)
    assert ei.value.rc == -3  # TG_ERR_ENCODING
    with pytest.raises(gpu_error()) as ei:
        gpu.srs_k
    assert ei.value.rc == -4  # TG_ERR_NOSRS: a rejected load leaves no SRS


@pytest.mark.parametrize("where", ["g", "g_lagrange", "w", "u"])
def test_srs_rejects_identity(gpu, srs_points, where):
    """An identity in a base set breaks the branch-free accumulation's
    precondition (MSMs over SRS sets always take it); tg_load_srs rejects."""
    k, n = 4, 16
    good = srs_blob(k, *srs_parts(srs_points, k))
    gpu.load_srs(good)
    assert gpu.srs_k == k
    blob = bytearray(good)
    ofs = {"g": 4 + 32 * 3, "g_lagrange": 4 + 32 * (n + 15), "w": 4 + 64 * n,
           "u": 4 + 64 * n + 32}[where]
    blob[ofs:ofs + 32] = bytes(32)
    expect_degenerate(gpu, bytes(blob))


@pytest.mark.parametrize("where", ["g", "g_lagrange"])
@pytest.mark.parametrize("negated", [False, True])
def test_srs_rejects_repeated_x(gpu, srs_points, where, negated):
    """a repeated point, or a point and its negation, in one base set"""
    k, n = 4, 16
    g, gl, w, u = srs_parts(srs_points, k)
    g, gl = list(g), list(gl)
    tgt = g if where == "g" else gl
    x, y = tgt[2]
    tgt[13] = (x, Q - y if negated else y)
    gpu.load_srs(srs_blob(k, *srs_parts(srs_points, k)))
    expect_degenerate(gpu, srs_blob(k, g, gl, w, u))


def test_srs_same_point_in_both_sets_is_fine(gpu, srs_points):
    """g and g_lagrange are separate MSM base sets: only repeats within one
    set matter."""
    k = 4
    g, gl, w, u = srs_parts(srs_points, k)
    gl = [g[0]] + list(gl[1:])
    gpu.load_srs(srs_blob(k, g, gl, w, u))
    assert gpu.srs_k == k


def test_srs_params15_still_loads(gpu, srs_points, params15):
    k = 4
    blob = bytearray(srs_blob(k, *srs_parts(srs_points, k)))
    blob[4:36] = bytes(32)
    expect_degenerate(gpu, bytes(blob))
    gpu.load_srs(params15)
    assert gpu.srs_k == 15
    n = 1 << 15
    sc = bytearray(32 * n)
    sc[32 * 12345] = 1
    assert gpu.msm(bytes(sc), base_set=1) == oc.decompress(
        oc.FQ, params15[4 + 32 * 12345:4 + 32 * 12346])
