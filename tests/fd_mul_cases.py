"""Operands that sit on the limb edges of the field multiply's device forms:
the five 52-bit limbs of the FP64-limb experiment and the nine 30-bit limbs of
the radix-2^30 multiply. Shared by test_fd_mul_variants_host.py (CPU, every
form) and test_fd_mul_device_gpu.py (the kernels)."""

M52 = (1 << 52) - 1
LIMB_EDGES = (0, 1, 1 << 51, M52)


def limb_edge_values(mod):
    """Values whose five 52-bit limbs are each one of LIMB_EDGES, read as the
    limbs of a, of 4a (what the multiply cuts) and of 16a mod 2^260."""
    out = []
    for code in range(len(LIMB_EDGES) ** 5):
        v = 0
        for k in range(5):
            v |= LIMB_EDGES[code // 4**k % 4] << (52 * k)
        # a itself, with the top limb cut to the field's width or reduced
        out += [v & ((1 << 254) - 1), v % mod]
        # 4a == v up to the two low bits; 16a == v mod 2^260 up to four
        out += [(v >> 2) & ((1 << 254) - 1), (v >> 2) % mod]
        out += [(v >> 4) & ((1 << 254) - 1), (v >> 4) % mod]
    out = sorted(set(out))
    assert all(0 <= v < mod for v in out)
    return out


def tie_limb_pairs(rng):
    """52-bit limb pairs whose product has low 52 bits exactly 2^51 (the
    rounding tie of the high part), with the high part even and odd."""
    pairs = [(1 << 26, 1 << 25), (1 << 25, 1 << 26), (1 << 51, 1), (1 << 51, M52)]
    for al, be in ((1, 3), (3, 1), (3, 3), (5, 7), (7, 7)):
        pairs.append((al << 26, be << 25))
    for _ in range(40):
        al, be = rng.randrange(1 << 26) | 1, rng.randrange(1 << 26) | 1
        pairs.append((al << 26, be << 25))
    assert all(x <= M52 and y <= M52 and (x * y) & M52 == 1 << 51 for x, y in pairs)
    assert {(x * y) >> 52 & 1 for x, y in pairs} == {0, 1}
    return pairs


def limb30_edge_values(mod):
    """The same for the nine 30-bit limbs of 2^7 a that the radix-2^30
    multiply cuts: every limb one of 0, 1, 2^29, 2^30 - 1, in patterns that
    set all limbs alike, one limb apart, and alternate."""
    edges = (0, 1, 1 << 29, (1 << 30) - 1)
    pats = set()
    for e in edges:
        for o in edges:
            pats.add(tuple([e] * 9))
            pats.add(tuple(e if k % 2 else o for k in range(9)))
            for pos in range(9):
                pats.add(tuple(o if k == pos else e for k in range(9)))
    out = set()
    for pat in pats:
        v = sum(l << (30 * k) for k, l in enumerate(pat))
        out |= {(v >> 7) & ((1 << 254) - 1), (v >> 7) % mod, v % mod}
    return sorted(out)
