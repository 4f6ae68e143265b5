"""CPU-side test of the TGD1 parser and of the gate-kernel generator's guards.

pdesc_parse (taiga_amd/csrc/prover_impl.hpp) is the only thing between a desc
blob and the engine's fixed-size arrays (HFoldArgs on the device, the host
work arrays), so it must refuse every shape they cannot hold, and must do so
without reading past the blob or throwing. tests/host/desc_probe.cpp calls it
(and hf_rtc_source / the cache key of hf_rtc.hpp); it is compiled with hipcc
and the host AddressSanitizer + UBSan and run as a plain program, so an
over-read, an overflowing index or a signed overflow ends the run with a
report. The blobs come from tools/gen_rand_circuit.py at k = 8: the parser
needs no SRS. Skips only when hipcc is absent."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_rand_circuit as grc  # noqa: E402

HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

K = 8
N = 1 << K
U32 = 0xFFFFFFFF
(H_K, H_EXT_K, H_FIXED, H_ADVICE, H_INSTANCE, H_BF, H_GATES, H_PERM, H_CHUNK, H_LOOKUPS,
 H_CONSTS, H_AQ, H_FQ, H_IQ, H_ROWS) = range(15)
A, F, I = grc.OP_ADVICE, grc.OP_FIXED, grc.OP_INSTANCE


# ---------------- TGD1 in Python: unpack, change, pack ----------------

class Desc:
    """a TGD1 blob taken apart; pack() derives the header counts from the
    parts unless `hdr` overrides a word"""

    def __init__(self, blob):
        assert blob[:4] == b"TGD1"
        h = list(struct.unpack_from("<15I", blob, 4))
        self.k, self.ext_k, self.bf, self.rows = h[H_K], h[H_EXT_K], h[H_BF], h[H_ROWS]
        self.n_advice, self.n_instance, self.chunk_len = h[H_ADVICE], h[H_INSTANCE], h[H_CHUNK]
        p = 64
        n = 1 << self.k

        def take(m):
            nonlocal p
            p += m
            return blob[p - m:p]

        def expr():
            (no,) = struct.unpack("<I", take(4))
            return [struct.unpack("<IIi", take(12)) for _ in range(no)]

        self.consts = [take(32) for _ in range(h[H_CONSTS])]
        self.advice_q = [struct.unpack("<Ii", take(8)) for _ in range(h[H_AQ])]
        self.fixed_q = [struct.unpack("<Ii", take(8)) for _ in range(h[H_FQ])]
        self.instance_q = [struct.unpack("<Ii", take(8)) for _ in range(h[H_IQ])]
        self.perm = [struct.unpack("<II", take(8)) for _ in range(h[H_PERM])]
        self.gates = [expr() for _ in range(h[H_GATES])]
        self.lookups = []
        for _ in range(h[H_LOOKUPS]):
            ni, nt = struct.unpack("<II", take(8))
            self.lookups.append(([expr() for _ in range(ni)], [expr() for _ in range(nt)]))
        self.sigma = [list(struct.unpack(f"<{2 * n}I", take(8 * n))) for _ in range(h[H_PERM])]
        self.fixed = [take(32 * n) for _ in range(h[H_FIXED])]
        assert p == len(blob)
        self.hdr = {}
        self.lk_counts = {}  # lookup index -> (ni, nt) written instead of the true ones
        self.gate_nops = {}  # gate index -> op count written instead of the true one

    def pack(self, upto=None):
        """upto = "first_expr": stop after the first gate expression"""
        h = [self.k, self.ext_k, len(self.fixed), self.n_advice, self.n_instance, self.bf,
             len(self.gates), len(self.perm), self.chunk_len, len(self.lookups),
             len(self.consts), len(self.advice_q), len(self.fixed_q), len(self.instance_q),
             self.rows]
        for i, v in self.hdr.items():
            h[i] = v
        out = [b"TGD1", struct.pack("<15I", *h)] + self.consts
        for qs in (self.advice_q, self.fixed_q, self.instance_q):
            out += [struct.pack("<Ii", c, r) for c, r in qs]
        out += [struct.pack("<II", a, b) for a, b in self.perm]

        def expr(ops, nops=None):
            return struct.pack("<I", len(ops) if nops is None else nops) + b"".join(
                struct.pack("<IIi", *op) for op in ops)

        for gi, g in enumerate(self.gates):
            out.append(expr(g, self.gate_nops.get(gi)))
            if upto == "first_expr":
                return b"".join(out)
        for li, (ins, tabs) in enumerate(self.lookups):
            out.append(struct.pack("<II", *self.lk_counts.get(li, (len(ins), len(tabs)))))
            out += [expr(e) for e in ins + tabs]
        out += [struct.pack(f"<{len(s)}I", *s) for s in self.sigma]
        out += self.fixed
        return b"".join(out)

    def n_point_sets(self):
        n_chunks = -(-len(self.perm) // self.chunk_len)
        return len(grc.point_sets(self.advice_q, self.fixed_q, self.instance_q, n_chunks,
                                  len(self.lookups), self.bf))


@pytest.fixture(scope="module")
def blobs():
    """name -> desc blob at k = 8, edge shapes and the one-over shapes"""
    out = {nm: grc.gen_edge(nm, k=K)[0] for nm in grc.EDGE_CASES}
    out.update({nm: grc.gen_over(nm, k=K)[0] for nm in grc.OVER_CASES})
    return out


def base(blobs, name="depth8"):
    return Desc(blobs[name])


# ---------------- the probe ----------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("desc_probe")
    exe = d / "desc_probe"
    subprocess.run(
        [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950",
         "-Xarch_host", "-fsanitize=address,undefined",
         "-Xarch_host", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(REPO, "taiga_amd", "csrc"),
         os.path.join(REPO, "tests", "host", "desc_probe.cpp"), "-lhiprtc", "-o", str(exe)],
        check=True)
    count = [0]

    def run(records, raw=False):
        """records: bytes each; returns one output line per record, or with
        `raw` the whole output as it is. A sanitizer report is a non-zero exit
        and fails here."""
        count[0] += 1
        path = d / f"in{count[0]}.bin"
        path.write_bytes(b"".join(records))
        env = {k: v for k, v in os.environ.items() if k != "TG_HF_CACHE"}
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True,
                           timeout=600, env=env)
        path.unlink()
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and \
            "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
        if raw:
            return r.stdout
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(records)
        return lines

    return run


def P(blob):
    return b"P" + struct.pack("<I", len(blob)) + blob


def S(blob, gate, ops):
    return (b"S" + struct.pack("<I", len(blob)) + blob + struct.pack("<II", gate, len(ops)) +
            b"".join(struct.pack("<IIi", *op) for op in ops))


def header_line(blob):
    return "accept " + " ".join(str(v) for v in struct.unpack_from("<15I", blob, 4))


def expect(probe, cases):
    """cases: (label, blob, accepted?)"""
    got = probe([P(b) for _, b, _ in cases])
    bad = []
    for (label, blob, ok), line in zip(cases, got):
        if ok:
            if not (line.startswith(header_line(blob) + " src=") and
                    int(line.rsplit("=", 1)[1]) > 0):
                bad.append((label, "accepted expected", line))
        elif line != "reject":
            bad.append((label, "reject expected", line))
    assert not bad, bad


# ---------------- tests ----------------

def test_capacities_match_the_generator(probe):
    """the constants of prover_impl.hpp, as the generator mirrors them"""
    caps = [int(v) for v in probe([b"C"])[0].split()[1:]]
    (max_k, ext_ratio, fixed, advice, instance, gates, perm, chunks, lookups, lk_exprs,
     queries, instance_q, stack, col_points, point_sets) = caps
    assert (advice, fixed, gates, perm, chunks) == (
        grc.MAX_ADVICE, grc.MAX_FIXED, grc.MAX_GATES, grc.MAX_PERM, grc.MAX_CHUNKS)
    assert (lookups, lk_exprs, queries, instance_q) == (
        grc.MAX_LOOKUPS, grc.MAX_LK_EXPRS, grc.MAX_QUERIES, grc.MAX_INSTANCE_Q)
    assert (stack, col_points, point_sets, ext_ratio) == (
        grc.MAX_STACK, grc.MAX_COL_POINTS, grc.MAX_POINT_SETS, grc.MAX_EXT_RATIO)
    assert instance == 1 and max_k >= 15


def test_repack_is_identity(blobs):
    for nm, blob in blobs.items():
        assert Desc(blob).pack() == blob, nm


def test_edge_shapes_accepted_one_over_rejected(probe, blobs):
    """each limit at its exact value and one above, as whole generated
    circuits: advice 16/17, chunks 8/9, stack 8/9, queries 64/65, lookup
    expressions 4/5 (and 4 lookups, 2 instance queries)"""
    cases = [(nm, blobs[nm], True) for nm in grc.EDGE_CASES]
    cases += [(nm, blobs[nm], False) for nm in grc.OVER_CASES]
    expect(probe, cases)
    hdr = {nm: struct.unpack_from("<15I", blobs[nm], 4) for nm in blobs}
    assert hdr["adv16"][H_ADVICE] == 16 and hdr["adv17"][H_ADVICE] == 17
    assert -(-hdr["chunks8"][H_PERM] // hdr["chunks8"][H_CHUNK]) == 8
    assert -(-hdr["chunks9"][H_PERM] // hdr["chunks9"][H_CHUNK]) == 9
    assert sum(hdr["queries64"][H_AQ:H_IQ + 1]) == 64
    assert sum(hdr["queries65"][H_AQ:H_IQ + 1]) == 65
    assert hdr["lookups4x4"][H_LOOKUPS] == 4 and hdr["const_inst_ops"][H_IQ] == 2
    peak = lambda nm: max(grc.stack_peak(e) for e in Desc(blobs[nm]).gates)  # noqa: E731
    assert peak("depth8") == 8 and peak("depth9") == 9
    assert all(len(x) == 4 for l in Desc(blobs["lookups4x4"]).lookups for x in l)
    assert all(len(x) == 5 for l in Desc(blobs["ni5"]).lookups for x in l)


def grown(blobs, n_gates=None, n_fixed=None, n_perm=None):
    """the base circuit with more gates / fixed columns / permutation columns"""
    d = base(blobs)
    if n_gates:
        d.gates = [d.gates[i % 2] for i in range(n_gates)]
    if n_fixed:
        d.fixed += [bytes(32 * N)] * (n_fixed - len(d.fixed))
    if n_perm:
        col = 0
        while len(d.perm) < n_perm:  # fixed columns not yet in the permutation
            if (1, col) not in d.perm:
                j = len(d.perm)
                d.perm.append((1, col))
                if (col, 0) not in d.fixed_q:
                    d.fixed_q.append((col, 0))
                d.sigma.append([v for i in range(N) for v in (j, i)])
            col += 1
    return d


def test_count_limits_exact_and_one_above(probe, blobs):
    cases = []
    for n, ok in ((256, True), (257, False)):
        cases.append((f"gates {n}", grown(blobs, n_gates=n).pack(), ok))
    for n, ok in ((64, True), (65, False)):
        cases.append((f"fixed {n}", grown(blobs, n_fixed=n).pack(), ok))
    for n, ok in ((32, True), (33, False)):
        cases.append((f"perm {n}", grown(blobs, n_fixed=40, n_perm=n).pack(), ok))
    for lk, ok in ((4, True), (5, False)):
        d = base(blobs)
        d.lookups = d.lookups * lk
        cases.append((f"lookups {lk}", d.pack(), ok))
    for extra, ok in ((5, True), (6, False)):  # ext_n / n = 32, 64
        d = base(blobs)
        d.ext_k = d.k + extra
        cases.append((f"ext ratio 2^{extra}", d.pack(), ok))
    for nq, ok in ((2, True), (3, False)):  # instance queries
        d = base(blobs)
        d.instance_q = [(0, r) for r in range(nq)]
        cases.append((f"instance_q {nq}", d.pack(), ok))
    for npts, ok in ((4, True), (5, False)):  # rotations on one column
        d = base(blobs)
        have = sum(1 for c, _ in d.advice_q if c == 7)
        d.advice_q += [(7, 10 + r) for r in range(npts - have)]
        cases.append((f"column points {npts}", d.pack(), ok))
    for nsets, ok in ((16, True), (17, False)):  # distinct multiopen point sets
        d = base(blobs)
        col = 0
        while d.n_point_sets() < nsets:  # a new rotation sequence per column
            (d.advice_q if col < 8 else d.fixed_q).append((col % 8, 20 + col))
            col += 1
        assert d.n_point_sets() == nsets and col <= 13
        cases.append((f"point sets {nsets}", d.pack(), ok))
    for cl, ok in ((1, False), (2, True)):  # 10 permutation columns: 10 and 5 chunks
        d = base(blobs)
        d.chunk_len = cl
        cases.append((f"chunk_len {cl}", d.pack(), ok))
    for cl, ok in ((0, False), (1 << 20, True), ((1 << 20) + 1, False), (U32, False)):
        d = base(blobs, "chunks8")
        d.chunk_len = cl
        cases.append((f"chunk_len {cl}", d.pack(), ok))
    expect(probe, cases)


def test_header_words_out_of_range(probe, blobs):
    """a header word alone over its limit (the body no longer matches, but the
    word must be refused before anything is sized or shifted by it)"""
    cases = []
    over = {H_K: 25, H_EXT_K: 14, H_FIXED: 65, H_ADVICE: 17, H_INSTANCE: 2, H_GATES: 257,
            H_PERM: 33, H_LOOKUPS: 5, H_AQ: 65, H_FQ: 65, H_IQ: 3}
    for word in range(15):
        for v in {over.get(word, U32), U32, 0x80000000, 0x7FFFFFFF}:
            d = base(blobs)
            d.hdr[word] = v
            cases.append((f"hdr[{word}] = {v:#x}", d.pack(), False))
    for word, v in ((H_K, 0), (H_EXT_K, K - 1), (H_INSTANCE, 0), (H_PERM, 0), (H_CHUNK, 0),
                    (H_BF, N - 1), (H_BF, N), (H_ROWS, N - 5), (H_CONSTS, 1 << 20),
                    (H_CONSTS, 4), (H_CONSTS, 2), (H_GATES, 1), (H_GATES, 3)):
        d = base(blobs)
        d.hdr[word] = v
        cases.append((f"hdr[{word}] = {v}", d.pack(), False))
    d = base(blobs)
    cases.append(("magic", b"TGD2" + d.pack()[4:], False))
    expect(probe, cases)


def test_bad_indices_tags_and_postfix(probe, blobs):
    cases = []

    def mut(label, fn, name="depth8"):
        d = base(blobs, name)
        fn(d)
        cases.append((label, d.pack(), False))

    def set_q(lst, i, col=None, rot=None):
        def fn(d):
            q = getattr(d, lst)
            q[i] = (q[i][0] if col is None else col, q[i][1] if rot is None else rot)
        return fn

    # query columns
    mut("advice_q col", set_q("advice_q", 0, col=8))
    mut("advice_q col huge", set_q("advice_q", 0, col=U32))
    mut("fixed_q col", set_q("fixed_q", 0, col=5))
    mut("instance_q col", set_q("instance_q", 0, col=1))
    mut("query rot n", lambda d: d.advice_q.append((7, N)))
    mut("query rot -n", lambda d: d.advice_q.append((7, -N)))
    mut("query rot min", lambda d: d.advice_q.append((7, -(1 << 31))))
    mut("duplicate query", lambda d: d.advice_q.append(d.advice_q[0]))
    # permutation columns and sigma
    mut("perm kind", lambda d: d.perm.__setitem__(0, (3, 0)))
    mut("perm advice idx", lambda d: d.perm.__setitem__(0, (0, 8)))
    mut("perm fixed idx", lambda d: d.perm.__setitem__(9, (1, 5)))
    mut("perm instance idx", lambda d: d.perm.__setitem__(8, (2, 1)))
    mut("perm column without its query", lambda d: d.fixed_q.remove((0, 0)))
    mut("sigma column", lambda d: d.sigma[3].__setitem__(2 * 17, 10))
    mut("sigma column huge", lambda d: d.sigma[0].__setitem__(0, U32))
    mut("sigma row", lambda d: d.sigma[9].__setitem__(2 * (N - 1) + 1, N))
    mut("sigma row huge", lambda d: d.sigma[5].__setitem__(1, U32))
    # ops: indices, tags
    a0 = (A, 0, 0)

    def gate(ops, gi=1):
        return lambda d: d.gates.__setitem__(gi, ops)

    def lk_in(ops):
        return lambda d: d.lookups[0][0].__setitem__(0, ops)

    def lk_tab(ops):
        return lambda d: d.lookups[0][1].__setitem__(0, ops)

    for where, put in (("gate", gate), ("first gate", lambda ops: gate(ops, 0)),
                       ("lookup input", lk_in), ("lookup table", lk_tab)):
        mut(f"{where}: const index", put([(grc.OP_CONST, 3, 0)]))
        mut(f"{where}: scale index", put([a0, (grc.OP_SCALE, 3, 0)]))
        mut(f"{where}: scale index huge", put([a0, (grc.OP_SCALE, U32, 0)]))
        mut(f"{where}: advice column", put([(A, 8, 0)]))
        mut(f"{where}: fixed column", put([(F, 5, 0)]))
        mut(f"{where}: instance column", put([(I, 1, 0)]))
        mut(f"{where}: unlisted advice query", put([(A, 0, 3)]))
        mut(f"{where}: unlisted fixed query", put([(F, 0, 1)]))
        mut(f"{where}: unlisted instance query", put([(I, 0, 1)]))
        mut(f"{where}: tag 9", put([a0, (9, 0, 0)]))
        mut(f"{where}: tag huge", put([(U32, 0, 0)]))
        mut(f"{where}: tag 9 alone", put([(9, 0, 0)]))
        # postfix shape
        mut(f"{where}: empty", put([]))
        mut(f"{where}: add underflows", put([(grc.OP_ADD, 0, 0)]))
        mut(f"{where}: mul on one", put([a0, (grc.OP_MUL, 0, 0)]))
        mut(f"{where}: sub underflows late", put([a0, a0, (grc.OP_SUB, 0, 0),
                                                  (grc.OP_SUB, 0, 0)]))
        mut(f"{where}: neg on none", put([(grc.OP_NEG, 0, 0)]))
        mut(f"{where}: scale on none", put([(grc.OP_SCALE, 0, 0)]))
        mut(f"{where}: ends at 2", put([a0, a0]))
        mut(f"{where}: ends at 3", put([a0, a0, a0, a0, (grc.OP_ADD, 0, 0)]))
        mut(f"{where}: peak 9", put([a0] * 9 + [(grc.OP_ADD, 0, 0)] * 8))
    # the same positions with well-formed replacements are accepted
    ok = []
    for label, fn in (("peak 8", gate([a0] * 8 + [(grc.OP_ADD, 0, 0)] * 7)),
                      ("one cell", gate([a0])),
                      ("neg scale const", gate([(grc.OP_CONST, 2, 0), (grc.OP_NEG, 0, 0),
                                                (grc.OP_SCALE, 0, 0)])),
                      ("lookup input peak 8", lk_in([a0] * 8 + [(grc.OP_MUL, 0, 0)] * 7))):
        d = base(blobs)
        fn(d)
        ok.append((label, d.pack(), True))
    # lookup expression counts
    for ni, nt in ((0, 1), (1, 0), (5, 1), (1, 5), (U32, 1), (1, U32)):
        mut(f"lookup counts {ni} {nt}", lambda d, c=(ni, nt): d.lk_counts.__setitem__(0, c))
    # op counts that the blob cannot hold
    for nops in (U32, 1 << 30, 0x15555556, 100000):
        mut(f"gate op count {nops}", lambda d, c=nops: d.gate_nops.__setitem__(0, c))
        mut(f"last gate op count {nops}", lambda d, c=nops: d.gate_nops.__setitem__(1, c))
    # a circuit that pushes constants and reads the instance column inside gates
    mut("const_inst: const index", lambda d: d.consts.pop(), "const_inst_ops")
    mut("const_inst: instance query unlisted", lambda d: d.instance_q.pop(1),
        "const_inst_ops")
    expect(probe, cases + ok)
    assert len(cases) > 100


def test_truncation_and_trailing_bytes(probe, blobs):
    """every prefix through the header and the first expression, 50 sampled
    lengths beyond, and blobs with bytes after the end: all refused, none read
    past its own heap block"""
    for name in ("depth8", "const_inst_ops"):
        d = base(blobs, name)
        blob = d.pack()
        assert blob == blobs[name]
        first = len(d.pack(upto="first_expr"))
        assert 64 < first < 1024
        lengths = list(range(first + 1))
        rng = random.Random(5)
        lengths += sorted(rng.sample(range(first + 1, len(blob)), 47))
        lengths += [len(blob) - 1, len(blob) - 4, len(blob) - 32]
        assert len(lengths) == first + 1 + 50
        cases = [(f"{name}[:{n}]", blob[:n], False) for n in lengths]
        cases += [(f"{name} + {len(t)}", blob + t, False)
                  for t in (b"\0", b"\0\0\0\0", bytes(32), blob[:64])]
        cases.append((name, blob, True))
        expect(probe, cases)


def test_generator_refuses_what_the_parser_would(probe, blobs):
    """hf_rtc_source on postfix and tags changed BEHIND the parser: the empty
    string or a whole kernel, never an access outside its stack or tables"""
    blob = blobs["depth8"]
    a0 = (A, 0, 0)
    bad = [
        [(grc.OP_ADD, 0, 0)], [a0, (grc.OP_MUL, 0, 0)], [(grc.OP_NEG, 0, 0)],
        [(grc.OP_SCALE, 0, 0)], [a0, a0], [], [(9, 0, 0)], [a0, (U32, 0, 0)],
        [a0, a0, (grc.OP_SUB, 0, 0), (grc.OP_SUB, 0, 0)],
        [(grc.OP_CONST, 3, 0)], [a0, (grc.OP_SCALE, 3, 0)], [(grc.OP_CONST, U32, 0)],
        [(A, 8, 0)], [(A, U32, 0)], [(F, 5, 0)], [(I, 1, 0)],
    ]
    good = [
        [a0], [(A, 0, -(1 << 31))], [(A, 7, (1 << 31) - 1), (grc.OP_NEG, 0, 0)],
        [a0] * 12 + [(grc.OP_ADD, 0, 0)] * 11,  # deeper than the device stack: still text
        [(grc.OP_CONST, 2, 0), a0, (grc.OP_MUL, 0, 0), (grc.OP_SCALE, 0, 0)],
    ]
    recs = [S(blob, g, ops) for ops in bad + good for g in (0, 1)]
    got = probe(recs)
    nbad = 2 * len(bad)
    assert got[:nbad] == ["src 0 0"] * nbad, got[:nbad]
    for line in got[nbad:]:
        _, size, whole = line.split()
        assert int(size) > 3000 and whole == "1", line


def test_cache_key_follows_the_generated_source(probe):
    """the .hsaco cache path of cs1.desc changes when one character of the
    generator's prelude changes, so an object compiled from older text is
    never loaded; the same text gives the same path"""
    blob = open(os.path.join(GOLDEN, "cs1.desc"), "rb").read()
    line = probe([b"K" + struct.pack("<I", len(blob)) + blob])[0]
    tag, default, changed, again = line.split()
    assert tag == "key"
    assert default == again and default != changed
    for p in (default, changed):
        d, f = os.path.split(p)
        assert d == "tests/golden" and f.startswith("hf_") and f.endswith(".hsaco")
        assert len(f) == len("hf_") + 16 + len(".hsaco")


CSRC = os.path.join(REPO, "taiga_amd", "csrc")


def test_prelude_is_the_field_header(probe):
    """the generated program's prelude holds the bytes of pasta_field.hpp
    exactly once, and nothing with a body besides: what is left around them
    (two typedefs, a define, using-declarations) has no '{', so no function
    the header defines can be stated a second time"""
    header = open(os.path.join(CSRC, "pasta_field.hpp"), "rb").read().decode()
    pre = probe([b"R"], raw=True)
    assert len(header) > 5000 and pre.count(header) == 1
    rest = pre.replace(header, "")
    assert "{" not in rest and len(rest) < 400, rest


def test_generated_program_compiles(blobs, tmp_path):
    """hf_cache_tool, the plain build's, turns the smallest edge circuit into
    a code object: a field header that the runtime compiler refuses fails
    here, not as a quiet fall-back to the interpreter on the GPU"""
    subprocess.run(["make", "-C", CSRC, "hf_cache_tool", f"HIPCC={HIPCC}"], check=True,
                   capture_output=True)
    desc = tmp_path / "depth8.desc"
    desc.write_bytes(blobs["depth8"])
    r = subprocess.run([os.path.join(CSRC, "hf_cache_tool"), str(desc)], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, TG_HF_CACHE=str(tmp_path)))
    assert r.returncode == 0 and "compile failed" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert " -> " in r.stdout, r.stdout
    path = r.stdout.split(" -> ")[1].split(" (")[0]
    assert os.path.dirname(path) == str(tmp_path) and os.path.getsize(path) > 0


def test_gen_output_is_unchanged():
    """gen(seed) stays byte-identical next to gen_edge(): two seeds of the
    GPU parity fuzz, by digest of (desc, instance, advice)"""
    import hashlib

    want = {
        21: "1e6781e25ee42b0505948586f017e3c74d3ace3365a30fa5ecd76169cff6f63e",
        69: "c58a36b20cce1366eaf09b6e297bf36d7891245103c4445230f8f71d223a7e7d",
    }
    for seed, digest in want.items():
        desc, inst, adv, _ = grc.gen(seed)
        h = hashlib.sha256()
        for part in (desc, inst, adv):
            h.update(hashlib.sha256(part).digest())
        assert h.hexdigest() == digest, seed
