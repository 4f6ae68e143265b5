"""Scalars shared by the fixed-base MSM tests (GPU: test_msm_fixed_base_gpu.py,
host recoding: test_msm_recode_host.py). Not a test module."""
import pypasta as pp

P = pp.P


def edge_scalars(C, NWIN):
    """digit values at and around the recoding threshold in the lowest, a
    middle and the top window, the field's ends, and runs of carries. The top
    window of a canonical scalar holds less than C bits (p < 2^255), so a digit
    value too large for it goes to the highest window that holds it as well
    as, reduced to the bits that fit, to the top window."""
    top = NWIN - 1
    out = [0, 1, P - 1, P - 2, 1 << 254, (1 << 254) - 1]
    for v in (1, 1 << (C - 1), (1 << (C - 1)) + 1, (1 << C) - 1):
        for w in (0, NWIN // 2, top):
            while (v << (C * w)) >= P:
                w -= 1
            out.append(v << (C * w))
        topbits = (P - 1).bit_length() - 1 - C * top  # whole bits below p's top bit
        out.append((v & ((1 << topbits) - 1) or 1) << (C * top))
    # all-ones digits: every window recodes and carries into the next
    out.append((1 << 254) - 1)
    out.append(sum(((1 << C) - 1) << (C * w) for w in range(top)))
    # every digit just above the threshold: a carry out of each window
    out.append(sum(((1 << (C - 1)) + 1) << (C * w) for w in range(top)))
    # every digit exactly at the threshold: never recoded
    out.append(sum((1 << (C - 1)) << (C * w) for w in range(top)))
    assert all(0 <= s < P for s in out)
    return out
