"""fd28 experiment (tools/experiments/fd28.hpp): carry-chain-free radix-2^28
Montgomery multiplication — the round-2 candidate for the VCC-hazard-bound
bucket kernel (profiles/r01_bucket_acc_hazard_analysis.txt). The TG_HD
arithmetic runs identically on host and device, so these host checks pin
the numerics: the probe's `mul28 a b` must equal a*b*2^-280 mod p. The
experiment is not part of the product library; it is reached through
tests/host/arith_probe.cpp. Skips only when hipcc is absent."""
import random

import pytest

from test_host_arith import HIPCC, h, probe  # noqa: F401  (probe: fixture)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
RINV = pow(1 << 280, P - 2, P)
NONCANONICAL = "NONCANONICAL"


def check_products(probe, pairs):
    got = probe([f"mul28 {h(a)} {h(b)}" for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g != NONCANONICAL, (a, b)
        assert int(g, 16) == a * b * RINV % P, (a, b)


def test_random_products(probe):
    rng = random.Random(2828)
    check_products(probe, [(rng.randrange(P), rng.randrange(P)) for _ in range(300)])


def test_edge_values(probe):
    edges = [0, 1, 2, P - 1, P - 2, (1 << 255) % P, (1 << 28) - 1, 1 << 28,
             (1 << 252) - 1, P >> 1]
    check_products(probe, [(a, b) for a in edges for b in edges])


def test_worst_case_digit_patterns(probe):
    """all-ones digit patterns maximize the lazy-carry accumulators"""
    ones28 = int("1" * 255, 2) % P  # 255 set bits
    maxd = P - 1
    check_products(probe, [(ones28, ones28), (ones28, maxd), (maxd, maxd)])


def test_rejects_noncanonical(probe):
    assert probe([f"mul28 {h(P)} {h(1)}"]) == [NONCANONICAL]
