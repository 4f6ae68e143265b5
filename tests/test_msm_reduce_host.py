"""CPU-side test of the MSM bucket reduction (msm.hip: msm_seg_sums, the
bit-plane window sum).

tests/host/msm_reduce_probe.cpp runs the kernels' per-lane bodies with loops
in place of lanes, for every row of the msm_cfg() table, and compares each
window sum with the naive sum_d (d+1)*B_d itself. Its buckets are known
multiples of the generator, so this file also recomputes every window sum
from the scalars alone, with Python integers and one multiplication in
oracle/pypasta.py. Everything is exact. Skips only when hipcc is absent."""
import os
import shutil
import subprocess

import pytest

import pypasta as pp
from conftest import REPO
from kernel_shapes import MSM_TABLE

HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

M64 = (1 << 64) - 1
G = pp.Point.generator(pp.Q)


def sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


R = [sm64(0xC0FFEE + i) for i in range(16)]


def walk(seed, n):
    out, k = [], 0
    for d in range(n):
        k += R[sm64((seed * 65536 + d) & M64) & 15]
        out.append(k)
    return out


def wsum(scalars):
    """sum (d+1) * k_d over a window's bucket scalars"""
    return sum((d + 1) * k for d, k in enumerate(scalars))


def expected_scalar(c, name):
    n = MSM_TABLE[c].nbuck
    base, _, win = name.partition(".w")
    if base == "random":
        return wsum(walk(c, n))
    if base == "allid":
        return 0
    if base.startswith("single."):
        d = int(base[7:])
        assert 0 <= d < n
        return (d + 1) * 2 * R[d & 15]
    if base == "allequal":
        return n * (n + 1) // 2 * 2 * R[3]
    if base == "negpairs0":
        return -sum(walk(c + 100, n // 2))
    if base == "negpairs1":
        return 2 * R[5] - sum(walk(c + 101, n // 2 - 1)) + n * 2 * R[7]
    if base == "b2a":
        return wsum(walk(c + 200, n)) if win == "1" else 0
    if base == "b2b":
        return wsum(walk(c + 201, n)) if win == "0" else 0
    raise AssertionError(name)


@pytest.fixture(scope="module")
def probe_lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("msm_reduce_probe") / "msm_reduce_probe"
    subprocess.run(
        [HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950",
         "-I", os.path.join(REPO, "taiga_amd", "csrc"),
         os.path.join(REPO, "tests", "host", "msm_reduce_probe.cpp"), "-o", str(out)],
        check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    rows = {}
    for line in r.stdout.split("\n"):
        if not line or line.startswith("#"):
            continue
        c, name, status, x, y = line.split()
        rows.setdefault(int(c), {})[name] = (status, int(x, 16), int(y, 16))
    return rows


@pytest.mark.parametrize("c", sorted(MSM_TABLE))
def test_window_sum_matches_naive_and_scalars(probe_lines, c):
    cases = probe_lines[c]
    n = MSM_TABLE[c].nbuck
    names = set(cases)
    # the case list itself: dense, degenerate, colliding and batch layouts,
    # and single buckets at both ends and around every power of two
    assert {"random", "allid", "allequal", "negpairs0", "negpairs1",
            "b2a.w0", "b2a.w1", "b2b.w0", "b2b.w1"} <= names
    singles = {int(nm[7:]) for nm in names if nm.startswith("single.")}
    want = {0, 1, 2, 3, n - 2, n - 1}
    p = 1
    while p < n:
        want.update(d for d in (p - 1, p, p + 1) if 0 <= d < n)
        p <<= 1
    assert want <= singles
    for name, (status, x, y) in sorted(cases.items()):
        assert status == "OK", (c, name)  # the probe's own naive sum
        k = expected_scalar(c, name) % pp.P
        if k == 0:
            assert (x, y) == (0, 0), (c, name)
        else:
            pt = G.mul(k)
            assert (x, y) == (pt.x, pt.y), (c, name)
    assert cases["allid"][1:] == (0, 0)
    assert cases["b2a.w0"][1:] == (0, 0) and cases["b2b.w1"][1:] == (0, 0)
    assert cases["random"][1:] != (0, 0)


def test_every_row_ran(probe_lines):
    assert sorted(probe_lines) == sorted(MSM_TABLE)
