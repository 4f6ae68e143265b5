"""CPU-side exactness test of the field multiply's other forms.

fd_mul_r30 / fd_sqr_r30 in pasta_device.hpp (radix 2^30, what the device
multiplies with; the host keeps the CIOS form) and fd_mul_f52 / fd_sqr_f52 in
tools/experiments/fd52.hpp (FP64 limb products, a measured negative result)
are __host__ __device__. Here the same source runs on the CPU
(tests/host/fdmul_probe.cpp, compiled with hipcc) and is compared, bit for
bit and canonically, with Python integers: a * b * R^-1 mod p. Everything is
exact. Skips only when hipcc is absent."""
import os
import random
import shutil
import subprocess

import pytest

import pypasta as pp
from conftest import REPO
from fd_mul_cases import (LIMB_EDGES, M52, limb30_edge_values, limb_edge_values,
                          tie_limb_pairs)
from kernel_shapes import edge_values

HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

MODS = {"p": pp.P, "q": pp.Q}
R = 1 << 256


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("fdmul_probe") / "fdmul_probe"
    subprocess.run(
        [HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950",
         "-I", os.path.join(REPO, "taiga_amd", "csrc"),
         "-I", os.path.join(REPO, "tools", "experiments"),
         os.path.join(REPO, "tests", "host", "fdmul_probe.cpp"), "-o", str(out)],
        check=True)

    def run(lines):
        r = subprocess.run([str(out)], input="\n".join(lines) + "\n",
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-200:], r.stderr[-200:])
        got = r.stdout.split("\n")[:-1]
        assert len(got) == len(lines)
        return got

    return run


def h(v):
    return f"{v:064x}"


def operand_pairs(mod, seed):
    rng = random.Random(seed)
    ev = edge_values(mod)
    assert {0, 1, mod - 1, R % mod} <= set(ev)
    pairs = [(a, b) for a in ev for b in ev]
    pairs += [(rng.randrange(mod), rng.randrange(mod)) for _ in range(2000)]
    le = limb_edge_values(mod)
    for i, v in enumerate(le):
        pairs += [(v, v), (v, le[(i * 7 + 3) % len(le)]), (v, rng.randrange(mod)),
                  (rng.randrange(mod), v)]
    # a tie in the product of limb i of 4a with limb j of 4b, alone and
    # with random bits in the other limbs
    for x, y in tie_limb_pairs(rng):
        for i in range(5):
            for j in range(5):
                a, b = (x << (52 * i)) >> 2, (y << (52 * j)) >> 2
                if a < mod and b < mod:
                    pairs.append((a, b))
                    na = (rng.randrange(mod) & ~(M52 << (52 * i) >> 2)) | a
                    nb = (rng.randrange(mod) & ~(M52 << (52 * j) >> 2)) | b
                    pairs.append((na % mod, nb % mod))
    return pairs


# "f": the FP64-limb form, "r": the radix-2^30 form
@pytest.mark.parametrize("variant", ["f", "r"])
@pytest.mark.parametrize("f", ["p", "q"])
def test_mul_and_sqr_exact(probe, f, variant):
    mod = MODS[f]
    rinv = pow(R, -1, mod)
    pairs = operand_pairs(mod, 81 if f == "p" else 82)
    rng = random.Random(84)
    l30 = limb30_edge_values(mod)
    for i, v in enumerate(l30):
        pairs += [(v, v), (v, l30[(i * 5 + 2) % len(l30)]), (v, rng.randrange(mod))]
    mul, sqr = "mul" + variant, "sqr" + variant
    lines, exp = [], []
    for a, b in pairs:
        want = h(a * b * rinv % mod)
        lines += [f"{mul} {f} {h(a)} {h(b)}", f"{mul} {f} {h(b)} {h(a)}",
                  f"muli {f} {h(a)} {h(b)}"]
        exp += [want, want, want]
    vals = sorted({v for pr in pairs for v in pr})
    for a in vals:
        want = h(a * a * rinv % mod)
        lines += [f"{sqr} {f} {h(a)}", f"{mul} {f} {h(a)} {h(a)}"]
        exp += [want, want]
    got = probe(lines)
    bad = [(l, g, e) for l, g, e in zip(lines, got, exp) if g != e]
    assert not bad, f"{len(bad)} of {len(lines)} wrong; first: {bad[:3]}"


def test_limb_split_identity(probe):
    """x*y == H*2^52 + L with |L| <= 2^51 for the split on its own."""
    rng = random.Random(83)
    pairs = [(x, y) for x in LIMB_EDGES + (2, M52 - 1, (1 << 26) - 1, 1 << 26)
             for y in LIMB_EDGES + (2, M52 - 1, (1 << 26) + 1, 1 << 25)]
    pairs += tie_limb_pairs(rng)
    while len(pairs) < 100_000:
        bits = rng.choice((52, 52, 52, 40, 27, 26, 13))
        pairs.append((rng.getrandbits(52), rng.getrandbits(bits)))
    got = probe([f"split {x:x} {y:x}" for x, y in pairs])
    for (x, y), g in zip(pairs, got):
        H, L = (int(v) for v in g.split())
        assert H * (1 << 52) + L == x * y and abs(L) <= 1 << 51 and H >= 0, (x, y, g)
