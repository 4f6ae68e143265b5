"""permute_expression_pair of the lookup argument on the device
(taiga_amd/csrc/lookup_argument.hip) on caller data, through
tg_lookup_permute_probe: the bitonic sort of A and of the table, and the
parallel construction of S'. The reference is the provers' serial loop
written with Python integers. Everything is exact: there are no tolerances.

T mirrors LK_TILE of lookup_argument.hip, the keys one block sorts in LDS.
The sizes sit on both sides of every boundary where the launch chain
changes: one partial tile, exactly one tile, the first global stage (T + 1
pads to 2 tiles), two merge levels above a tile (2T + 1 and 5000 pad to 4)."""
import random

import pytest

import pypasta as pp

pytestmark = pytest.mark.gpu

P = pp.P
T = 2048  # LK_TILE
SIZES = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 5000]


def b32(v):
    return v.to_bytes(32, "little")


def ints(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def pack(vals):
    return b"".join(map(b32, vals))


def serial_pair(a, s):
    """the serial loop of both provers: sort both, walk A'; a new value
    takes its table entry, skipped table entries are left over and fill the
    repeat slots in order. None when an input value is not in the table."""
    u = len(a)
    ap, t = sorted(a), sorted(s)
    sp, leftover, repeats = [None] * u, [], []
    j = 0
    for i in range(u):
        if i == 0 or ap[i] != ap[i - 1]:
            while j < u and t[j] < ap[i]:
                leftover.append(t[j])
                j += 1
            if j >= u or t[j] != ap[i]:
                return None
            sp[i] = t[j]
            j += 1
        else:
            repeats.append(i)
    leftover.extend(t[j:])
    assert len(leftover) == len(repeats)
    for i, v in zip(repeats, leftover):
        sp[i] = v
    return ap, sp


def distinct(rng, n, lo=0, hi=P):
    """n distinct values in [lo, hi)"""
    out = set()
    while len(out) < n:
        out.add(rng.randrange(lo, hi))
    out = list(out)
    rng.shuffle(out)
    return out


# ---- value families: (u, rng) -> (a, s), every element of a in s ----

def fam_shuffle(u, rng):
    """a is a shuffle of a distinct s: no leftover, S' = A'"""
    s = distinct(rng, u)
    a = list(s)
    rng.shuffle(a)
    return a, s


def fam_all_equal(u, rng):
    """one first slot, every other slot a repeat"""
    v = rng.randrange(P)
    s = [v] + [x for x in distinct(rng, u) if x != v][: u - 1]
    rng.shuffle(s)
    return [v] * u, s


def fam_range_check(u, rng):
    """s = 0..1023 padded with zeros, a random in it"""
    m = min(1024, u)
    s = list(range(m)) + [0] * (u - m)
    return [rng.randrange(m) for _ in range(u)], s


def fam_limb3(u, rng):
    """keys that differ only in limb 3 (the low limbs are one constant)"""
    low = rng.getrandbits(192)
    s = [(k << 192) | low for k in distinct(rng, u, 0, 1 << 60)]
    return [rng.choice(s) for _ in range(u)], s


def fam_limb0(u, rng):
    """keys that differ only in limb 0"""
    high = rng.getrandbits(180) << 64
    s = [high | k for k in distinct(rng, u, 0, 1 << 64)]
    return [rng.choice(s) for _ in range(u)], s


SPECIAL = [0, 1, 1 << 64, 1 << 128, 1 << 192, P - 2, P - 1]


def fam_special(u, rng):
    s = [SPECIAL[i % len(SPECIAL)] for i in range(u)]
    rng.shuffle(s)
    return [rng.choice(s) for _ in range(u)], s


def fam_extras(u, rng):
    """s with extra copies of values of a, and with values below min(a) and
    above max(a)"""
    d = max(1, u // 4)
    pool = distinct(rng, d, P // 4, P // 2)
    rest = u - d
    copies, lows = rest // 3, rest // 3
    s = (pool + [rng.choice(pool) for _ in range(copies)]
         + [rng.randrange(P // 4) for _ in range(lows)]
         + [rng.randrange(P // 2, P) for _ in range(rest - copies - lows)])
    rng.shuffle(s)
    a = pool + [rng.choice(pool) for _ in range(u - d)]
    rng.shuffle(a)
    return a, s


def fam_long_run(u, rng):
    """a run of T + 5 equal keys placed across a tile border, in A' and in
    the sorted table"""
    run = T + 5
    before = T // 2
    v = P // 2
    vals = distinct(rng, before, 0, v) + [v] * run + distinct(rng, u - before - run, v + 1, P)
    a, s = list(vals), list(vals)
    rng.shuffle(a)
    rng.shuffle(s)
    return a, s


FAMILIES = [fam_shuffle, fam_all_equal, fam_range_check, fam_limb3, fam_limb0, fam_special,
            fam_extras]


@pytest.fixture(scope="module")
def gpu():
    import taiga_amd

    g = taiga_amd.TaigaGpu(0)  # no SRS: the probe needs none
    yield g
    g.close()


def check(gpu, a, s):
    exp = serial_pair(a, s)
    assert exp is not None
    ap, sp = gpu.lookup_permute_probe(pack(a), pack(s))
    ap, sp = ints(ap), ints(sp)
    assert ap == exp[0], "A' differs"
    assert sp == exp[1], "S' differs"
    return ap, sp


@pytest.mark.parametrize("u", SIZES)
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__[4:])
def test_permute_pair(gpu, fam, u):
    rng = random.Random(9000 + 31 * FAMILIES.index(fam) + u)
    a, s = fam(u, rng)
    assert len(a) == len(s) == u
    ap, sp = check(gpu, a, s)
    assert sorted(sp) == sorted(s)
    if fam is fam_shuffle:
        assert sp == ap
    if fam is fam_all_equal:
        assert sp[0] == ap[0] and sorted(sp[1:]) == sp[1:]


@pytest.mark.parametrize("u", [2 * T + 1, 5000])
def test_long_run_across_a_tile_border(gpu, u):
    a, s = fam_long_run(u, random.Random(9500 + u))
    ap, _ = check(gpu, a, s)
    assert ap[T - 1] == ap[T] == P // 2  # the run does cross the border


@pytest.mark.parametrize("where", ["below", "above", "between"])
def test_missing_input_is_refused_and_context_recovers(gpu, where):
    import taiga_amd

    u = T + 1
    rng = random.Random(9600)
    s = sorted(distinct(rng, u, 1000, P - 1000))
    a = [rng.choice(s) for _ in range(u)]
    gap = next(i for i in range(u - 1) if s[i + 1] - s[i] > 1)
    bad = {"below": s[0] - 1, "above": s[-1] + 1, "between": s[gap] + 1}[where]
    assert bad not in s
    broken = list(a)
    broken[u // 2] = bad
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.lookup_permute_probe(pack(broken), pack(s))
    assert e.value.rc == -2
    check(gpu, a, s)  # the error flag does not outlive the call


def test_rejects_bad_input(gpu):
    import taiga_amd

    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.lookup_permute_probe(b"", b"")
    assert e.value.rc == -2
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.lookup_permute_probe(pack([1, P]), pack([1, 1]))
    assert e.value.rc == -3
    with pytest.raises(taiga_amd.TaigaGpuError) as e:
        gpu.lookup_permute_probe(pack([1, 1]), pack([1, P]))
    assert e.value.rc == -3
