"""The grand-product device kernels (taiga_amd/csrc/grand_products.hip) on
caller data, through the diagnostic entry points of include/taiga_gpu.h:
batch inverse, chained prefix product, and the permutation and lookup
products end to end. The reference is Python integers mod p, with
omega = pypasta.root_of_unity(P, k) and delta = 5^(2^32).
Everything is exact — there are no tolerances.

The lengths sit on both sides of every boundary where the kernels' index
arithmetic changes: the per-thread chunk E and the T elements one block
covers."""
import random

import pytest

import pypasta as pp

pytestmark = pytest.mark.gpu

P = pp.P
# mirrors of the kernels' constants in grand_products.hip
B = 256      # GP_B: threads per block
E = 4        # GP_E: elements per thread
T = B * E    # GP_T: elements one block covers
U15 = (1 << 15) - 6  # the production row count
DELTA = pow(5, 2 ** 32, P)


def inv_index(block, t, m):
    """gp_inv_index: element m of thread t of a batch-inverse block"""
    return block * T + m * B + t


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def pack(vals):
    return b"".join(map(b32, vals))


def rand_vals(rng, n):
    """n canonical values (< 2^254 < p) without a per-element loop"""
    raw = bytearray(rng.getrandbits(n * 256).to_bytes(n * 32, "little"))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    return ints(bytes(raw))


def batch_inv(vals):
    """exact inverses of non-zero values, one pow for all of them"""
    pre, run = [], 1
    for v in vals:
        pre.append(run)
        run = run * v % P
    inv = pow(run, -1, P)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * vals[i] % P
    return out


@pytest.fixture(scope="module")
def gpu():
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)  # no SRS: none of these entry points needs one
    yield g
    g.close()


# ---------------- batch inverse ----------------

INV_LENGTHS = [1, 2, E - 1, E, E + 1, T - 1, T, T + 1, 1000, U15, 1 << 15, 9 * U15]


def check_inverse(gpu, vals):
    out = ints(gpu.fp_batch_inverse(pack(vals)))
    assert len(out) == len(vals)
    bad = [i for i, (x, y) in enumerate(zip(vals, out))
           if (y != 0 if x == 0 else x * y % P != 1)]
    assert not bad, f"wrong at indices {bad[:8]} of {len(vals)}"
    assert all(y < P for y in out)
    if len(vals) <= 1000:
        assert out == [pow(x, -1, P) if x else 0 for x in vals]


@pytest.mark.parametrize("n", INV_LENGTHS)
def test_batch_inverse_mixed(gpu, n):
    """random values with 0, 1 and p - 1 mixed in"""
    rng = random.Random(7000 + n)
    vals = rand_vals(rng, n)
    for i in rng.sample(range(n), min(n, max(3, n // 50))):
        vals[i] = rng.choice((0, 1, P - 1))
    check_inverse(gpu, vals)


@pytest.mark.parametrize("n", INV_LENGTHS)
def test_batch_inverse_zero_placement(gpu, n):
    """zeros at the first and last element of a thread's chunk and of a
    block, and one thread chunk that is all zeros"""
    rng = random.Random(7100 + n)
    vals = [v or 1 for v in rand_vals(rng, n)]
    last_blk = (n - 1) // T
    zeros = {inv_index(0, 5, 0), inv_index(0, 5, E - 1),          # one thread's ends
             inv_index(last_blk, 9, 0), inv_index(last_blk, 9, E - 1),
             0, T - 1, T, last_blk * T, n - 1}                    # block ends
    zeros |= {inv_index(0, 7, m) for m in range(E)}               # a whole chunk
    zeros |= {inv_index(last_blk, 11, m) for m in range(E)}
    for i in zeros:
        if i < n:
            vals[i] = 0
    check_inverse(gpu, vals)


def test_batch_inverse_zero_neighbours(gpu):
    x = 0x1234567890ABCDEF ** 3 % P
    out = ints(gpu.fp_batch_inverse(pack([0, x, 0])))
    assert out == [0, pow(x, -1, P), 0]


def test_batch_inverse_rejects_bad_input(gpu):
    import taiga_amd

    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.fp_batch_inverse(b"")
    assert e.value.rc == -2
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.fp_batch_inverse(b32(P))
    assert e.value.rc == -3


# ---------------- chained prefix product ----------------

def prefix_model(ratios, seg_lens, init):
    out, z, pos = [], init, 0
    for L in seg_lens:
        out.append(z)
        for r in ratios[pos:pos + L]:
            z = z * r % P
            out.append(z)
        pos += L
    return out


@pytest.fixture(scope="module")
def ratios():
    """2 * (2^15 - 6) random non-zero ratios shared by the scan cases"""
    return [v or 1 for v in rand_vals(random.Random(7200), 2 * U15)]


@pytest.mark.parametrize("init_random", [False, True])
@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 1000, U15])
def test_prefix_product_single(gpu, ratios, n, init_random):
    init = random.Random(7300 + n).randrange(1, P) if init_random else 1
    got = ints(gpu.fp_prefix_product(pack(ratios[:n]), [n], b32(init)))
    assert got == prefix_model(ratios, [n], init)


@pytest.mark.parametrize("seg_lens", [[U15, U15], [1000] * 8, [1, T + 1, 2, 999]],
                         ids=["2xU15", "8x1000", "unequal"])
def test_prefix_product_chained(gpu, ratios, seg_lens):
    init = random.Random(7400 + len(seg_lens)).randrange(1, P)
    n = sum(seg_lens)
    got = ints(gpu.fp_prefix_product(pack(ratios[:n]), seg_lens, b32(init)))
    exp = prefix_model(ratios, seg_lens, init)
    assert len(got) == n + len(seg_lens)
    assert got == exp
    # every segment starts where the one before ended
    pos = 0
    for L in seg_lens[:-1]:
        assert got[pos + L] == got[pos + L + 1]
        pos += L + 1


def test_prefix_product_zero_ratio(gpu, ratios):
    """a zero ratio in the middle of a segment: everything after it is zero,
    the next segments' start values included"""
    seg_lens = [1, T + 1, 2, 999]
    n = sum(seg_lens)
    rs = list(ratios[:n])
    local = (T + 1) // 2  # ratio index within the second segment
    rs[1 + local] = 0
    got = ints(gpu.fp_prefix_product(pack(rs), seg_lens, b32(1)))
    assert got == prefix_model(rs, seg_lens, 1)
    first_zero = 2 + local + 1  # after the first segment's two values
    assert all(v != 0 for v in got[:first_zero])
    assert all(v == 0 for v in got[first_zero:])


def test_prefix_product_rejects_bad_input(gpu):
    import taiga_amd

    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.fp_prefix_product(b32(1), [1, 0], b32(1))
    assert e.value.rc == -2
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.fp_prefix_product(b32(1), [1], b32(P))
    assert e.value.rc == -3


# ---------------- permutation probe ----------------

PERM_SHAPES = [(6, 58, 3, 2), (10, 1018, 32, 4), (15, U15, 3, 2)]


def perm_model(k, u, ncols, chunk_len, vals, sigs, beta, gamma):
    """the serial loops of the prover's permutation stage: per chunk the
    num / den products, z chaining from chunk to chunk"""
    n = 1 << k
    omega = pp.root_of_unity(P, k)
    wpow = [1] * u
    for i in range(1, u):
        wpow[i] = wpow[i - 1] * omega % P
    nchunks = (ncols + chunk_len - 1) // chunk_len
    dpow = [pow(DELTA, j, P) for j in range(ncols)]
    nums, dens = [], []
    for ch in range(nchunks):
        for i in range(u):
            pn = pd = 1
            for j in range(ch * chunk_len, min((ch + 1) * chunk_len, ncols)):
                v = vals[j * n + i]
                pn = pn * (v + beta * dpow[j] * wpow[i] + gamma) % P
                pd = pd * (v + beta * sigs[j * n + i] + gamma) % P
            nums.append(pn)
            dens.append(pd)
    assert all(dens)
    dinv = batch_inv(dens)
    out, z = [], 1
    for ch in range(nchunks):
        out.append(z)
        for i in range(u):
            z = z * nums[ch * u + i] % P * dinv[ch * u + i] % P
            out.append(z)
    return out


def identity_sigma(k, ncols):
    n = 1 << k
    omega = pp.root_of_unity(P, k)
    wpow = [1] * n
    for i in range(1, n):
        wpow[i] = wpow[i - 1] * omega % P
    return [pow(DELTA, j, P) * w % P for j in range(ncols) for w in wpow]


@pytest.fixture(scope="module", params=PERM_SHAPES, ids=lambda s: f"k{s[0]}c{s[2]}")
def perm_case(request):
    """values, the identity sigma, and a sigma that swaps pairs of cells
    (rows below u, any columns) whose values were made equal"""
    k, u, ncols, chunk_len = request.param
    n = 1 << k
    rng = random.Random(7500 + k)
    vals = rand_vals(rng, ncols * n)
    ident = identity_sigma(k, ncols)
    swapped = list(ident)
    cells = rng.sample([(j, i) for j in range(ncols) for i in range(u)],
                       2 * min(200, u // 2))
    for (j1, i1), (j2, i2) in zip(cells[0::2], cells[1::2]):
        a, b = j1 * n + i1, j2 * n + i2
        vals[b] = vals[a]
        swapped[a], swapped[b] = swapped[b], swapped[a]
    beta, gamma = rng.randrange(P), rng.randrange(P)
    return k, u, ncols, chunk_len, vals, ident, swapped, beta, gamma


def run_perm(gpu, k, u, ncols, chunk_len, vals, sigs, beta, gamma):
    out = gpu.perm_product_probe(k, u, ncols, chunk_len, pack(vals), pack(sigs),
                                 b32(beta), b32(gamma))
    return ints(out)


def test_perm_probe_identity_sigma(gpu, perm_case):
    k, u, ncols, chunk_len, vals, ident, _, beta, gamma = perm_case
    got = run_perm(gpu, k, u, ncols, chunk_len, vals, ident, beta, gamma)
    nchunks = (ncols + chunk_len - 1) // chunk_len
    assert got == [1] * (nchunks * (u + 1))


def test_perm_probe_true_permutation(gpu, perm_case):
    k, u, ncols, chunk_len, vals, _, swapped, beta, gamma = perm_case
    got = run_perm(gpu, k, u, ncols, chunk_len, vals, swapped, beta, gamma)
    assert got == perm_model(k, u, ncols, chunk_len, vals, swapped, beta, gamma)
    assert got[-1] == 1            # the last chunk's z[u]
    assert any(v != 1 for v in got)


def test_perm_probe_random_sigma(gpu, perm_case):
    k, u, ncols, chunk_len, vals, _, _, beta, gamma = perm_case
    sigs = rand_vals(random.Random(7600 + k), ncols << k)
    got = run_perm(gpu, k, u, ncols, chunk_len, vals, sigs, beta, gamma)
    assert got == perm_model(k, u, ncols, chunk_len, vals, sigs, beta, gamma)


def test_perm_probe_rejects_bad_shapes(gpu):
    import taiga_amd

    n = 1 << 4
    col = pack([1] * n)
    for k, u, ncols, chunk_len in [(3, 1, 1, 1), (16, 1, 1, 1), (4, 0, 1, 1), (4, n, 1, 1),
                                   (4, 1, 0, 1), (4, 1, 33, 4), (4, 1, 9, 1), (4, 1, 1, 0)]:
        with pytest.raises(taiga_amd.TaigaGpuError) as e:
            gpu.perm_product_probe(k, u, ncols, chunk_len, col * 33, col * 33, b32(1),
                                   b32(1))
        assert e.value.rc == -2, (k, u, ncols, chunk_len)


# ---------------- lookup probe ----------------

def permute_pair(a, s):
    """permute_expression_pair over the usable rows: A' is A sorted; S' holds
    A'[i] wherever A' takes a new value, and the table values left over, in
    sorted order, in the other rows"""
    ap = sorted(a)
    counts = {}
    for v in s:
        counts[v] = counts.get(v, 0) + 1
    sp, repeats = [None] * len(a), []
    for i, v in enumerate(ap):
        if i == 0 or v != ap[i - 1]:
            assert counts.get(v, 0) > 0, "input value missing from the table"
            counts[v] -= 1
            sp[i] = v
        else:
            repeats.append(i)
    left = sorted(v for v, cnt in counts.items() for _ in range(cnt))
    assert len(left) == len(repeats)
    for i, v in zip(repeats, left):
        sp[i] = v
    return ap, sp


@pytest.mark.parametrize("k,u", [(6, 58), (15, U15)])
def test_lookup_probe(gpu, k, u):
    n = 1 << k
    rng = random.Random(7700 + k)
    # a table of u values with one repeat; inputs drawn from a small part of
    # it, so that A' has runs of equal values
    table = rand_vals(rng, u)
    table[3] = table[4]
    hot = table[: max(2, u // 64)]
    a = [rng.choice(hot) for _ in range(u)]
    ap, sp = permute_pair(a, table)
    assert sorted(sp) == sorted(table)
    tail = n - u
    cols = [a + rand_vals(rng, tail), table + rand_vals(rng, tail),
            ap + rand_vals(rng, tail), sp + rand_vals(rng, tail)]
    beta, gamma = rng.randrange(P), rng.randrange(P)
    got = ints(gpu.lookup_product_probe(k, u, *map(pack, cols), b32(beta), b32(gamma)))
    dens = [(ap[i] + beta) * (sp[i] + gamma) % P for i in range(u)]
    assert all(dens)
    dinv = batch_inv(dens)
    exp, z = [1], 1
    for i in range(u):
        z = z * ((a[i] + beta) * (table[i] + gamma) % P) % P * dinv[i] % P
        exp.append(z)
    assert got == exp
    assert got[u] == 1
    assert any(v != 1 for v in got)
