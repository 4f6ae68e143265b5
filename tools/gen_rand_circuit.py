#!/usr/bin/env python3
"""Random satisfiable circuit generator for prover parity fuzzing.

Produces (desc_bytes, instance_bytes, advice_bytes) triples: a random TGD1
circuit description (same blob format as tools/gen_cs1.py) together with a
witness that satisfies it BY CONSTRUCTION, fed to both provers through the
raw-witness entries (orc_prove_raw / tg_create_proof_raw) whose proof bytes
must match bit-for-bit and verify through both raw-instance verifiers.

gen_edge(name), further down, builds the fixed shapes that sit ON the engine
limits, by the same satisfiable-by-construction scheme. gen(seed) stays well
inside them (it emits expression stack peaks <= 4; the engine allows 8, the
device evaluator's s0..s7 register stack; advice <= 16, lookups <= 4,
permutation chunks <= 8) and varies per seed:
  - advice column count, gate count/expressions (rotations ±1, degree <= 9)
  - lookup count 0..2 (selector-gated membership in a fixed table)
  - permutation column set and chunk length (1..4 chunks), random equality
    cycles, instance-exposure copies
  - blinding factor count, instance row count

Satisfiability scheme: gate j is sel_j * (E_j - target_j) with a dedicated
0/1 selector fixed column; E_j only references advice columns with index
below target_j's, so targets are assigned left-to-right by evaluating E_j
(free columns are random). Selector-active rows keep every referenced row
below `usable` (rows >= usable are replaced by prover blinding and must
only be touched with zero selectors — the halo2 rule that gates vanish on
the WHOLE domain)."""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001

K = 15
N = 1 << K
EXT_K = 18

OP_CONST, OP_FIXED, OP_ADVICE, OP_INSTANCE, OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_SCALE = range(9)


def enc_expr(ops):
    out = struct.pack("<I", len(ops))
    for tag, a, b in ops:
        out += struct.pack("<IIi", tag, a, b)
    return out


def eval_expr(ops, row, advice, fixed, inst_col, consts, n=N):
    st = []
    for tag, a, b in ops:
        if tag == OP_CONST:
            st.append(consts[a])
        elif tag == OP_FIXED:
            st.append(fixed[a][(row + b) % n])
        elif tag == OP_ADVICE:
            st.append(advice[a][(row + b) % n])
        elif tag == OP_INSTANCE:
            st.append(inst_col[(row + b) % n])
        elif tag == OP_ADD:
            st[-2:] = [(st[-2] + st[-1]) % P]
        elif tag == OP_SUB:
            st[-2:] = [(st[-2] - st[-1]) % P]
        elif tag == OP_MUL:
            st[-2:] = [(st[-2] * st[-1]) % P]
        elif tag == OP_NEG:
            st[-1] = (-st[-1]) % P
        elif tag == OP_SCALE:
            st[-1] = st[-1] * consts[a] % P
    assert len(st) == 1
    return st[0]


def stack_peak(ops):
    d = peak = 0
    for tag, _, _ in ops:
        d += 1 if tag in (OP_CONST, OP_FIXED, OP_ADVICE, OP_INSTANCE) else (
            -1 if tag in (OP_ADD, OP_SUB, OP_MUL) else 0)
        peak = max(peak, d)
    return peak


def gen(seed, inst_override=None):
    """inst_override: optional list of field values replacing the drawn
    instance values (same rng stream is consumed either way, so the DESC
    bytes are identical for any override — only the witness changes).
    Extra override entries beyond n_instance_rows are ignored."""
    rng = random.Random(seed)
    bf = rng.choice([4, 5, 6])
    usable = N - (bf + 1)
    n_gates = rng.randint(2, 6)
    n_free = rng.randint(3, max(3, 10 - n_gates))
    n_advice = n_free + n_gates
    n_lookups = rng.randint(0, 2)
    n_instance_rows = rng.randint(1, 9)
    # fixed columns: one selector per gate, one table+selector per lookup,
    # one constant column
    n_fixed = n_gates + 2 * n_lookups + 1
    fc = n_fixed - 1
    consts = [rng.randrange(P) for _ in range(rng.randint(0, 3))]

    fixed = [[0] * N for _ in range(n_fixed)]
    advice = [[0] * N for _ in range(n_advice)]
    inst_vals = [rng.randrange(P) for _ in range(n_instance_rows)]
    if inst_override is not None:
        assert len(inst_override) >= n_instance_rows
        inst_vals = [v % P for v in inst_override[:n_instance_rows]]
    inst_col = [0] * N
    for r, v in enumerate(inst_vals):
        inst_col[r] = v

    # free columns: random on [0, usable); rows >= usable stay 0 (replaced
    # by prover blinding anyway)
    for c in range(n_free):
        col = advice[c]
        for i in range(usable):
            col[i] = rng.randrange(P)

    # ---- permutation: all advice cols + instance + the const fixed col
    perm_cols = [(0, i) for i in range(n_advice)] + [(2, 0), (1, fc)]
    pc_index = {c: j for j, c in enumerate(perm_cols)}
    sigma = [[(j, i) for i in range(N)] for j in range(len(perm_cols))]

    def copy(c1, r1, c2, r2):
        j1, j2 = pc_index[c1], pc_index[c2]
        a, b = sigma[j1][r1], sigma[j2][r2]
        sigma[j1][r1], sigma[j2][r2] = b, a

    # instance exposure: a0[r] = inst[r] (value + copy)
    for r in range(n_instance_rows):
        advice[0][r] = inst_vals[r]
        copy((2, 0), r, (0, 0), r)
    # const-col copy: a2[0] = fc[0]
    fixed[fc][0] = rng.randrange(P)
    advice[2][0] = fixed[fc][0]
    copy((0, 2), 0, (1, fc), 0)
    # random equality cycles within free column 2 (not used by lookups)
    for _ in range(rng.randint(1, 3)):
        r1 = rng.randrange(1, usable - 1)
        r2 = rng.randrange(1, usable - 1)
        if r1 == r2:
            continue
        advice[2][r2] = advice[2][r1]
        copy((0, 2), r1, (0, 2), r2)
    chunk_len = rng.randint(3, 7)

    # ---- lookups: input [q_lk * a1], table [f_table]. All lookups share
    # one value pool S (their tables hold the same SET in different row
    # arrangements) so overlapping active regions on the shared input
    # column a1 stay members of every table; 0 in S covers idle rows.
    lookups = []
    tset = [0] + [rng.randrange(P) for _ in range(63)]
    for l in range(n_lookups):
        qcol = n_gates + 2 * l
        tcol = n_gates + 2 * l + 1
        off = rng.randrange(64)
        for i in range(N):
            fixed[tcol][i] = tset[(i + off) % 64]
        lo = rng.randrange(0, usable // 2)
        hi = rng.randrange(lo + 1, usable - 1)
        for i in range(lo, hi):
            fixed[qcol][i] = 1
            advice[1][i] = rng.choice(tset)
        lookups.append(([[(OP_FIXED, qcol, 0), (OP_ADVICE, 1, 0), (OP_MUL, 0, 0)]],
                        [[(OP_FIXED, tcol, 0)]]))

    # ---- gates: sel_j * (E_j - target_j), target col = n_free + j
    gates = []
    for j in range(n_gates):
        tcol = n_free + j
        qcol = j
        trot = rng.choice([0, 0, 1])
        # selector-active region: every referenced row (rot in [-1, +1],
        # target rot in [0, +1]) must stay below usable
        lo = rng.randrange(1, usable // 2)
        hi = rng.randrange(lo + 1, usable - 2)
        for i in range(lo, hi):
            fixed[qcol][i] = 1
        # E: left-assoc chain of 1..4 factors over cols < tcol (peak
        # stack: sel + acc + 2 factor operands = 4; the device allows 8)
        nfac = rng.randint(1, 4)
        E = []
        deg = 0
        for f in range(nfac):
            kind = rng.randrange(4 if consts else 3)
            c1 = rng.randrange(tcol)
            r1 = rng.choice([-1, 0, 1])
            if kind == 0:  # single cell
                fac = [(OP_ADVICE, c1, r1)]
                d = 1
            elif kind == 1:  # a +/- b
                c2 = rng.randrange(tcol)
                fac = [(OP_ADVICE, c1, r1), (OP_ADVICE, c2, rng.choice([-1, 0, 1])),
                       (rng.choice([OP_ADD, OP_SUB]), 0, 0)]
                d = 1
            elif kind == 2:  # a * b
                c2 = rng.randrange(tcol)
                fac = [(OP_ADVICE, c1, r1), (OP_ADVICE, c2, rng.choice([-1, 0, 1])),
                       (OP_MUL, 0, 0)]
                d = 2
            else:  # a + const (SCALE exercises the const path)
                fac = [(OP_ADVICE, c1, r1), (OP_SCALE, rng.randrange(len(consts)), 0)]
                d = 1
            if deg + d > 7:
                break
            E += fac
            if f > 0:
                E.append((OP_MUL, 0, 0))
            deg += d
        if rng.random() < 0.3:
            E.append((OP_NEG, 0, 0))
        gate = [(OP_FIXED, qcol, 0)] + E + [(OP_ADVICE, tcol, trot), (OP_SUB, 0, 0),
                                            (OP_MUL, 0, 0)]
        assert stack_peak(gate) <= 4, stack_peak(gate)
        gates.append(gate)
        # assign the target so the gate vanishes on active rows
        for i in range(lo, hi):
            v = eval_expr(E, i, advice, fixed, inst_col, consts)
            advice[tcol][(i + trot) % N] = v

    # ---- queries (first-use order over gates then lookups, then perm
    # cols at rotation 0 — mirrors gen_cs1)
    advice_q, fixed_q, instance_q = [], [], []

    def note(lst, key):
        if key not in lst:
            lst.append(key)

    for ops in gates + [e for ins, tabs in lookups for e in ins + tabs]:
        for tag, a, b in ops:
            if tag == OP_ADVICE:
                note(advice_q, (a, b))
            elif tag == OP_FIXED:
                note(fixed_q, (a, b))
            elif tag == OP_INSTANCE:
                note(instance_q, (a, b))
    for kind, idx in perm_cols:
        note({0: advice_q, 1: fixed_q, 2: instance_q}[kind], (idx, 0))
    if not instance_q:
        note(instance_q, (0, 0))

    # ---- mock check (python-side MockProver equivalent) ----
    for g_i, ops in enumerate(gates):
        for i in range(0, usable, 97):  # stride-sampled; active rows exact below
            assert eval_expr(ops, i, advice, fixed, inst_col, consts) == 0, (g_i, i)
    for ops in gates:
        qcol = ops[0][1]
        for i in range(N):
            if fixed[qcol][i]:
                assert eval_expr(ops, i, advice, fixed, inst_col, consts) == 0
    for (ins, tabs), l in zip(lookups, range(n_lookups)):
        tcol = n_gates + 2 * l + 1
        tvals = set(fixed[tcol][:usable])
        for i in range(usable):
            v = eval_expr(ins[0], i, advice, fixed, inst_col, consts)
            assert v in tvals
    for j, scol in enumerate(sigma):
        for i in range(0, N, 251):
            cj, ri = scol[i]
            kind, idx = perm_cols[j]
            kind2, idx2 = perm_cols[cj]
            src = {0: lambda c, r: advice[c][r], 1: lambda c, r: fixed[c][r],
                   2: lambda c, r: inst_col[r]}
            assert src[kind](idx, i) == src[kind2](idx2, ri)

    # ---- serialize desc ----
    out = b"TGD1"
    out += struct.pack(
        "<15I", K, EXT_K, n_fixed, n_advice, 1, bf, len(gates),
        len(perm_cols), chunk_len, len(lookups), len(consts),
        len(advice_q), len(fixed_q), len(instance_q), n_instance_rows,
    )
    for c in consts:
        out += c.to_bytes(32, "little")
    for col, rot in advice_q:
        out += struct.pack("<Ii", col, rot)
    for col, rot in fixed_q:
        out += struct.pack("<Ii", col, rot)
    for col, rot in instance_q:
        out += struct.pack("<Ii", col, rot)
    for kind, idx in perm_cols:
        out += struct.pack("<II", kind, idx)
    for g in gates:
        out += enc_expr(g)
    for ins, tabs in lookups:
        out += struct.pack("<II", len(ins), len(tabs))
        for e in ins:
            out += enc_expr(e)
        for e in tabs:
            out += enc_expr(e)
    for j in range(len(perm_cols)):
        row = bytearray()
        for i in range(N):
            cj, ri = sigma[j][i]
            row += struct.pack("<II", cj, ri)
        out += bytes(row)
    for c in range(n_fixed):
        col = bytearray()
        for v in fixed[c]:
            col += v.to_bytes(32, "little")
        out += bytes(col)

    inst_bytes = b"".join(v.to_bytes(32, "little") for v in inst_vals)
    adv_bytes = b"".join(v.to_bytes(32, "little") for col in advice for v in col)
    meta = dict(n_advice=n_advice, n_free=n_free, n_gates=n_gates,
                n_lookups=n_lookups, n_fixed=n_fixed, bf=bf, chunk_len=chunk_len,
                n_perm=len(perm_cols), n_instance_rows=n_instance_rows)
    return out, inst_bytes, adv_bytes, meta


# ---------------------------------------------------------------------------
# Edge circuits: the smallest shapes that sit on each engine limit.
#
# Same scheme as gen(): every gate is sel * (E - target) with a 0/1 selector
# of its own; here E reads FREE columns only (random, final before any target
# is assigned), so gates may share a target column as long as their active
# regions are disjoint. Lookups are selector-gated tuples: lookup l has m
# input expressions sel * cell and m table columns holding the tuple pool
# (T_0[j], .., T_m-1[j]) with T_e[0] = 0, so idle rows (all-zero tuple) are
# members. The mirror of the engine's limits below is what pdesc_parse
# (taiga_amd/csrc/prover_impl.hpp) enforces.

MAX_ADVICE, MAX_FIXED, MAX_GATES, MAX_PERM, MAX_CHUNKS = 16, 64, 256, 32, 8
MAX_LOOKUPS, MAX_LK_EXPRS, MAX_QUERIES, MAX_INSTANCE_Q = 4, 4, 64, 2
MAX_STACK, MAX_COL_POINTS, MAX_POINT_SETS, MAX_EXT_RATIO = 8, 4, 16, 32

EDGE_CASES = ("adv13", "adv16", "gates8", "gates9", "gates17", "depth8", "chunks8",
              "lookups4x4", "queries64", "rot_wide", "const_inst_ops", "ext17", "ext19")
# one over a limit each: well-formed blobs that keygen must refuse
OVER_CASES = ("adv17", "chunks9", "depth9", "queries65", "ni5")


def point_sets(advice_q, fixed_q, instance_q, n_chunks, n_lookups, bf):
    """Distinct multiopen point sets as rotation sequences in query order
    (the prover groups polynomials by the exact sequence of their points)."""
    sets = []

    def add(seq):
        if seq and seq not in sets:
            sets.append(seq)

    for qs in (instance_q, advice_q, fixed_q):
        for c in sorted({c for c, _ in qs}):
            add([r for cc, r in qs if cc == c])
    add([0])
    add([0, 1])
    if n_chunks > 1:
        add([0, 1, -(bf + 1)])
    if n_lookups:
        add([0, -1])
    return sets


class _Builder:
    def __init__(self, seed, k, ext_k, n_advice, targets, n_consts=0, bf=5,
                 n_instance_rows=3, check=True):
        self.rng = rng = random.Random(seed)
        self.k, self.ext_k, self.bf, self.check = k, ext_k, bf, check
        self.n = n = 1 << k
        self.usable = usable = n - (bf + 1)
        self.n_advice = n_advice
        self.targets = list(targets)
        self.free = [c for c in range(n_advice) if c not in self.targets]
        assert {0, 1, 2} <= set(self.free)
        self.consts = [rng.randrange(1, P) for _ in range(n_consts)]
        self.advice = [[0] * n for _ in range(n_advice)]
        for c in self.free:
            col = self.advice[c]
            for i in range(usable):
                col[i] = rng.randrange(P)
        self.fixed = []
        self.fc = self.new_fixed()  # the constant column of the permutation
        self.inst_vals = [rng.randrange(P) for _ in range(n_instance_rows)]
        self.inst_col = [0] * n
        for r, v in enumerate(self.inst_vals):
            self.inst_col[r] = v
        self.gates = []    # (ops, qcol, E, tcol, trot, lo, hi)
        self.lookups = []  # (ins, tabs, lo, hi)
        self.copies = []
        # instance exposure a0[r] = inst[r]; a2[0] = fc[0]; one equality
        # cycle inside free column 2
        for r in range(n_instance_rows):
            self.advice[0][r] = self.inst_vals[r]
            self.copies.append(((2, 0), r, (0, 0), r))
        self.fixed[self.fc][0] = rng.randrange(P)
        self.advice[2][0] = self.fixed[self.fc][0]
        self.copies.append(((0, 2), 0, (1, self.fc), 0))
        r1, r2 = usable // 3, usable // 2
        self.advice[2][r2] = self.advice[2][r1]
        self.copies.append(((0, 2), r1, (0, 2), r2))
        self.pinned = {(2, 0), (2, r1), (2, r2)} | {(0, r) for r in range(n_instance_rows)}

    def new_fixed(self, random_fill=False):
        self.fixed.append([self.rng.randrange(P) for _ in range(self.n)] if random_fill
                          else [0] * self.n)
        return len(self.fixed) - 1

    def region(self, j, m, margin=6, length=None):
        """j-th of m disjoint row slices of [margin, usable - margin); at most
        `length` rows of it are used"""
        span = (self.usable - 2 * margin) // m
        assert span > 2 * margin, "k too small for this shape"
        lo = margin + j * span
        hi = lo + span - margin
        if length:
            hi = min(hi, lo + length)
        return lo, hi

    def add_lookup(self, in_cols, lo, hi, in_expr=None):
        """inputs sel * advice[c] for c in in_cols (or in_expr(sel, c) -> (ops,
        rest) with the cell's value set to pool - rest(row)); one table column
        per input"""
        assert not self.gates, "lookups first: they write free columns"
        rng, n = self.rng, self.n
        m = len(in_cols)
        qcol = self.new_fixed()
        pool = [[0] + [rng.randrange(P) for _ in range(63)] for _ in range(m)]
        off = rng.randrange(64)
        tcols = []
        for e in range(m):
            t = self.new_fixed()
            for i in range(n):
                self.fixed[t][i] = pool[e][(i + off) % 64]
            tcols.append(t)
        ins, rests = [], []
        for e, c in enumerate(in_cols):
            assert c in self.free
            if in_expr and e == 0:
                ops, rest = in_expr(qcol, c)
            else:
                ops, rest = [(OP_FIXED, qcol, 0), (OP_ADVICE, c, 0), (OP_MUL, 0, 0)], None
            ins.append(ops)
            rests.append(rest)
        for i in range(lo, hi):
            self.fixed[qcol][i] = 1
            j = rng.randrange(64)
            for e, c in enumerate(in_cols):
                assert (c, i) not in self.pinned
                v = pool[e][j]
                if rests[e]:
                    v = (v - eval_expr(rests[e], i, self.advice, self.fixed, self.inst_col,
                                       self.consts, n)) % P
                self.advice[c][i] = v
        self.lookups.append((ins, [[(OP_FIXED, t, 0)] for t in tcols], lo, hi))

    def add_gate(self, E, tcol, trot, lo, hi):
        assert tcol in self.targets
        qcol = self.new_fixed()
        for i in range(lo, hi):
            self.fixed[qcol][i] = 1
        ops = [(OP_FIXED, qcol, 0)] + E + [(OP_ADVICE, tcol, trot), (OP_SUB, 0, 0),
                                           (OP_MUL, 0, 0)]
        self.gates.append((ops, qcol, E, tcol, trot, lo, hi))

    def finish(self, chunk_len, n_perm_fixed=0):
        n, usable, advice, fixed = self.n, self.usable, self.advice, self.fixed
        inst_col, consts = self.inst_col, self.consts
        # targets: E reads free columns only, so any order works
        for ops, qcol, E, tcol, trot, lo, hi in self.gates:
            if self.check:
                assert all(a in self.free for tag, a, _ in E if tag == OP_ADVICE)
            for i in range(lo, hi):
                advice[tcol][(i + trot) % n] = eval_expr(E, i, advice, fixed, inst_col, consts, n)
        gates = [g[0] for g in self.gates]
        lookups = [(ins, tabs) for ins, tabs, _, _ in self.lookups]
        # permutation: every advice column, the instance column, the constant
        # fixed column (+ n_perm_fixed more fixed columns)
        perm_cols = [(0, i) for i in range(self.n_advice)] + [(2, 0), (1, self.fc)]
        for _ in range(n_perm_fixed):
            perm_cols.append((1, self.new_fixed(random_fill=True)))
        pc_index = {c: j for j, c in enumerate(perm_cols)}
        sigma = [[(j, i) for i in range(n)] for j in range(len(perm_cols))]
        for c1, r1, c2, r2 in self.copies:
            j1, j2 = pc_index[c1], pc_index[c2]
            sigma[j1][r1], sigma[j2][r2] = sigma[j2][r2], sigma[j1][r1]
        # queries: first use over gates then lookups, then the permutation
        # columns at rotation 0 (as gen() does)
        advice_q, fixed_q, instance_q = [], [], []
        by_tag = {OP_ADVICE: advice_q, OP_FIXED: fixed_q, OP_INSTANCE: instance_q}
        for ops in gates + [e for ins, tabs in lookups for e in ins + tabs]:
            for tag, a, b in ops:
                if tag in by_tag and (a, b) not in by_tag[tag]:
                    by_tag[tag].append((a, b))
        for kind, idx in perm_cols:
            lst = {0: advice_q, 1: fixed_q, 2: instance_q}[kind]
            if (idx, 0) not in lst:
                lst.append((idx, 0))
        n_chunks = -(-len(perm_cols) // chunk_len)
        meta = dict(n_advice=self.n_advice, n_gates=len(gates), n_lookups=len(lookups),
                    n_fixed=len(fixed), bf=self.bf, chunk_len=chunk_len,
                    n_perm=len(perm_cols), n_chunks=n_chunks, n_consts=len(consts),
                    n_instance_rows=len(self.inst_vals), k=self.k, ext_k=self.ext_k,
                    n_queries=len(advice_q) + len(fixed_q) + len(instance_q),
                    stack_peak=max(stack_peak(e) for e in gates +
                                   [e for ins, tabs in lookups for e in ins + tabs]),
                    n_point_sets=len(point_sets(advice_q, fixed_q, instance_q, n_chunks,
                                                len(lookups), self.bf)))
        if self.check:
            self._mock(gates, sigma, perm_cols)
            assert self.n_advice <= MAX_ADVICE and len(fixed) <= MAX_FIXED
            assert len(gates) <= MAX_GATES and len(perm_cols) <= MAX_PERM
            assert n_chunks <= MAX_CHUNKS and len(lookups) <= MAX_LOOKUPS
            assert all(1 <= len(x) <= MAX_LK_EXPRS for l in lookups for x in l)
            assert meta["n_queries"] <= MAX_QUERIES and len(instance_q) <= MAX_INSTANCE_Q
            assert meta["stack_peak"] <= MAX_STACK
            for qs in (advice_q, fixed_q, instance_q):
                assert all(sum(1 for c, _ in qs if c == col) <= MAX_COL_POINTS
                           for col, _ in qs)
            assert meta["n_point_sets"] <= MAX_POINT_SETS
            assert (1 << (self.ext_k - self.k)) <= MAX_EXT_RATIO
        out = b"TGD1" + struct.pack(
            "<15I", self.k, self.ext_k, len(fixed), self.n_advice, 1, self.bf, len(gates),
            len(perm_cols), chunk_len, len(lookups), len(consts),
            len(advice_q), len(fixed_q), len(instance_q), len(self.inst_vals))
        out += b"".join(c.to_bytes(32, "little") for c in consts)
        for qs in (advice_q, fixed_q, instance_q):
            out += b"".join(struct.pack("<Ii", col, rot) for col, rot in qs)
        out += b"".join(struct.pack("<II", kind, idx) for kind, idx in perm_cols)
        out += b"".join(enc_expr(g) for g in gates)
        for ins, tabs in lookups:
            out += struct.pack("<II", len(ins), len(tabs))
            out += b"".join(enc_expr(e) for e in ins + tabs)
        out += b"".join(struct.pack("<II", cj, ri) for col in sigma for cj, ri in col)
        out += b"".join(v.to_bytes(32, "little") for col in fixed for v in col)
        inst_bytes = b"".join(v.to_bytes(32, "little") for v in self.inst_vals)
        adv_bytes = b"".join(v.to_bytes(32, "little") for col in advice for v in col)
        return out, inst_bytes, adv_bytes, meta

    def _mock(self, gates, sigma, perm_cols):
        """python-side MockProver equivalent: gates on every active row and a
        stride sample of the rest, lookup tuples on the same rows, copies"""
        n, usable, advice, fixed = self.n, self.usable, self.advice, self.fixed
        inst_col, consts = self.inst_col, self.consts

        def ev(ops, i):
            return eval_expr(ops, i, advice, fixed, inst_col, consts, n)

        for (ops, qcol, E, tcol, trot, lo, hi) in self.gates:
            rows = set(range(lo, hi)) | set(range(0, usable, 97)) | {0, 1, usable - 1}
            for i in rows:
                assert ev(ops, i) == 0, (qcol, i)
            # rows past usable are blinded: the selector must be off, and off
            # wherever a rotation leaves [0, usable)
            rots = [b for tag, _, b in ops if tag in (OP_ADVICE, OP_INSTANCE)]
            for i in range(n):
                if fixed[qcol][i]:
                    assert 0 <= i + min(rots) and i + max(rots) < usable
        for ins, tabs, lo, hi in self.lookups:
            members = {tuple(fixed[t[0][1]][i] for t in tabs) for i in range(usable)}
            for i in set(range(lo, hi)) | set(range(0, usable, 97)):
                assert tuple(ev(e, i) for e in ins) in members, i
        src = {0: lambda c, r: advice[c][r], 1: lambda c, r: fixed[c][r],
               2: lambda c, r: inst_col[r]}
        for j, scol in enumerate(sigma):
            for i in set(range(0, n, 251)) | {r for _, r, _, _ in self.copies} | \
                    {r for _, _, _, r in self.copies}:
                cj, ri = scol[i]
                assert src[perm_cols[j][0]](perm_cols[j][1], i) == \
                    src[perm_cols[cj][0]](perm_cols[cj][1], ri)


def _chain(cells, ops_cycle):
    """left-leaning chain over cells [(col, rot)...]: peak stack 2"""
    E = [(OP_ADVICE, cells[0][0], cells[0][1])]
    for i, (c, r) in enumerate(cells[1:]):
        E += [(OP_ADVICE, c, r), (ops_cycle[i % len(ops_cycle)], 0, 0)]
    return E


def _right(pushes, binops):
    """right-leaning p0 (p1 (p2 ...)): peak stack len(pushes)"""
    assert len(binops) == len(pushes) - 1
    return list(pushes) + [(op, 0, 0) for op in reversed(binops)]


def _gen_shape(name, k, ext_k, check):
    seed = "edge:" + name
    mk = lambda **kw: _Builder(seed, k, ext_k, check=check, **kw)
    act = 256  # active rows per gate/lookup: enough for every code path

    if name in ("adv13", "adv16", "adv17", "chunks9"):
        n_adv = {"adv13": 13, "adv16": 16, "adv17": 17, "chunks9": 16}[name]
        b = mk(n_advice=n_adv, targets=[3, 4, 5, 6, 7], n_consts=2)
        high = list(range(12, n_adv))  # every column from 12 up feeds a lookup
        groups = [high[:2], high[2:4]] if len(high) > 2 else [high, high]
        for l, cols in enumerate(groups):
            b.add_lookup(cols, *b.region(l, 2, length=act))
        share = [b.free[j::5] for j in range(5)]
        for j, cols in enumerate(share):
            E = _chain([(c, 0) for c in cols], [OP_MUL, OP_ADD])
            if j == 0:
                E += [(OP_SCALE, 1, 0)]
            b.add_gate(E, 3 + j, j % 2, *b.region(j, 5, length=act))
        return b.finish(chunk_len=2 if name == "chunks9" else 3)

    if name in ("gates8", "gates9", "gates17"):
        m = int(name[5:])
        b = mk(n_advice=6, targets=[3, 4, 5])  # zero constants
        for j in range(m):
            cells = [(j % 3, 0), ((j + 1) % 3, j % 2), ((j + 2) % 3, 0)]
            E = _chain(cells, [OP_MUL, OP_SUB] if j % 2 else [OP_ADD, OP_MUL])
            b.add_gate(E, 3 + j % 3, 0, *b.region(j, m, length=act))
        return b.finish(chunk_len=4)

    if name in ("depth8", "depth9"):
        peak = int(name[5:])
        b = mk(n_advice=8, targets=[6, 7], n_consts=3)

        def deep_input(qcol, c):
            # sel * (cell + (a3 - (c0 + (a4 - (c1 + (a5 + c2)))))): 8 pushes
            rest = _right([(OP_ADVICE, 3, 0), (OP_CONST, 0, 0), (OP_ADVICE, 4, 0),
                           (OP_CONST, 1, 0), (OP_ADVICE, 5, 0), (OP_CONST, 2, 0)],
                          [OP_SUB, OP_ADD, OP_SUB, OP_ADD, OP_ADD])
            ops = [(OP_FIXED, qcol, 0), (OP_ADVICE, c, 0)] + rest + [(OP_ADD, 0, 0),
                                                                     (OP_MUL, 0, 0)]
            return ops, rest

        b.add_lookup([1], *b.region(0, 2, length=act), in_expr=deep_input)
        # sel + (peak - 1) pushes: a0 + a1 * (a2 + (a3 - (a4 + a5 * a0')))
        cells = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (0, 1), (1, 1)][:peak - 1]
        binops = [OP_ADD, OP_MUL, OP_ADD, OP_SUB, OP_ADD, OP_MUL, OP_ADD][:peak - 2]
        E = _right([(OP_ADVICE, c, r) for c, r in cells], binops)
        b.add_gate(E, 6, 0, *b.region(1, 2, length=act))
        b.add_gate(_chain([(0, 0), (3, 0)], [OP_MUL]), 7, 1, *b.region(0, 2, length=act))
        return b.finish(chunk_len=5)

    if name == "chunks8":
        b = mk(n_advice=14, targets=[12, 13])  # n_perm = 16; zero constants
        b.add_gate(_chain([(c, 0) for c in range(0, 6)], [OP_ADD, OP_MUL]), 12, 0,
                   *b.region(0, 2, length=act))
        b.add_gate(_chain([(c, 0) for c in range(6, 12)], [OP_MUL, OP_SUB]), 13, 1,
                   *b.region(1, 2, length=act))
        return b.finish(chunk_len=2)

    if name in ("lookups4x4", "ni5"):
        m = 5 if name == "ni5" else 4
        b = mk(n_advice=m + 5, targets=[m + 3, m + 4], n_consts=1)
        for l in range(4):  # disjoint regions: the input columns are shared
            b.add_lookup(list(range(3, 3 + m)), *b.region(l, 4, length=act))
        b.add_gate(_chain([(0, 0), (1, 0), (3, 0)], [OP_MUL, OP_ADD]), m + 3, 0,
                   *b.region(0, 2, length=act))
        b.add_gate(_chain([(2, 0), (4, 0)], [OP_SUB]) + [(OP_SCALE, 0, 0)], m + 4, 0,
                   *b.region(1, 2, length=act))
        return b.finish(chunk_len=4)

    if name in ("queries64", "queries65"):
        # 13 free advice columns x {0, +1, -1} + 3 targets = 42, 5 fixed data
        # columns x 3 + one x 2 (x 3 for 65) = 17 (18), 3 selectors + the
        # constant column = 4, instance = 1
        b = mk(n_advice=16, targets=[13, 14, 15])
        data = [b.new_fixed(random_fill=True) for _ in range(6)]
        for j, rot in enumerate((0, 1, -1)):
            E = _chain([(c, rot) for c in b.free], [OP_ADD, OP_MUL, OP_SUB, OP_ADD])
            nd = 6 if (rot != -1 or name == "queries65") else 5
            for f in data[:nd]:
                E += [(OP_FIXED, f, rot), (OP_ADD, 0, 0)]
            b.add_gate(E, 13 + j, 0, *b.region(j, 3, length=act))
        out = b.finish(chunk_len=6)
        assert out[3]["n_queries"] == (65 if name == "queries65" else MAX_QUERIES)
        return out

    if name == "rot_wide":
        b = mk(n_advice=8, targets=[5, 6, 7])  # zero constants
        for j, r in enumerate((5, 4, 3, 2, 1)):
            # a_j[0] + a_j[-r] * a_j[+r]; rows 0..r-1 read below row 0 (the
            # blinded tail) with the selector off
            E = [(OP_ADVICE, j, 0), (OP_ADVICE, j, -r), (OP_ADVICE, j, r), (OP_MUL, 0, 0),
                 (OP_ADD, 0, 0)]
            lo, hi = b.region(j, 5, length=act)
            b.add_gate(E, 5 + j % 3, 0, r if j == 0 else lo, hi)
        return b.finish(chunk_len=5)

    if name == "const_inst_ops":
        b = mk(n_advice=6, targets=[3, 4, 5], n_consts=3, n_instance_rows=5)
        # c0 * inst[0] + a1  (rows 0.. carry the instance values)
        b.add_gate([(OP_CONST, 0, 0), (OP_INSTANCE, 0, 0), (OP_MUL, 0, 0), (OP_ADVICE, 1, 0),
                    (OP_ADD, 0, 0)], 3, 0, 0, 64)
        # (inst[+1] - c1) * (a0 + c2)
        b.add_gate([(OP_INSTANCE, 0, 1), (OP_CONST, 1, 0), (OP_SUB, 0, 0), (OP_ADVICE, 0, 0),
                    (OP_CONST, 2, 0), (OP_ADD, 0, 0), (OP_MUL, 0, 0)], 4, 1, 0, 64)
        # c2 alone as an operand, then SCALE and NEG
        b.add_gate([(OP_ADVICE, 2, 0), (OP_CONST, 2, 0), (OP_MUL, 0, 0), (OP_SCALE, 1, 0),
                    (OP_NEG, 0, 0)], 5, 0, *b.region(1, 2, length=act))
        return b.finish(chunk_len=4)

    if name in ("ext17", "ext19"):
        # ext_n / n = 4 allows degree 5 (lookup: 5; permutation: chunk_len + 2);
        # 16 allows 17: a 12-cell product under its selector is degree 13,
        # more than ext 2^18 could hold
        b = mk(n_advice=6, targets=[4, 5], n_consts=1)
        b.add_lookup([1], *b.region(0, 2, length=act))
        nmul = 3 if name == "ext17" else 12
        cells = [(c % 4, (c // 4) % 2) for c in range(nmul)]
        b.add_gate(_chain(cells, [OP_MUL]), 4, 0, *b.region(1, 2, length=act))
        b.add_gate(_chain([(0, 0), (3, 0)], [OP_ADD]) + [(OP_SCALE, 0, 0)], 5, 1,
                   *b.region(0, 2, length=act))
        return b.finish(chunk_len=3 if name == "ext17" else 7)

    raise KeyError(name)


def _ext_k(name, k):
    return k + {"ext17": 2, "ext19": 4}.get(name, EXT_K - K)


def gen_edge(name, k=K):
    """(desc, instance, advice, meta) of the edge circuit `name` (one of
    EDGE_CASES), satisfiable by construction and mock-checked here. k below
    15 gives the same shape on fewer rows, for tests of the parser alone."""
    assert name in EDGE_CASES, name
    return _gen_shape(name, k, _ext_k(name, k), True)


def gen_over(name, k=K):
    """a well-formed circuit one step over an engine limit (OVER_CASES)"""
    assert name in OVER_CASES, name
    return _gen_shape(name, k, _ext_k(name, k), False)


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["1"]:
        if arg in EDGE_CASES:
            desc, inst, adv, meta = gen_edge(arg)
        else:
            desc, inst, adv, meta = gen(int(arg))
        print(f"{arg}: desc {len(desc)} bytes, {meta}")
