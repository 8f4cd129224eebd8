"""Identity of reads to their simulated truth (DESIGN.md section 4 [A19]): tool rtk_identity (plain and --gpu), library entries rtk_identity_begin / _chunk / _end,
api.identity_reads, `Ratatosk correct -s ... --truth-ref REF --truth-tsv TRUTH`. Parity is to tests/identity_restatement.py: integers exactly, error_rate and
identity as the table prints them (the bytes of both files are compared). Distances are the reference's own edlib's (ref_edlib, NW, k = -1, no IUPAC table);
pairs of at most 2 000 x 2 000 are checked with the restatement's DP too.

Without a GPU: the plain route on rtk_simulate --lr-truth output (two records, a multi-line gzip reference, a raw and a mutated -l file, FASTA reads, a read that
is not in the truth, an empty read, lower case, N / IUPAC bytes), every refusal, the exported symbols, common/edit_distance.hpp on the shapes of the GPU list.
On the GPU: k_identity on those shapes through api.identity_reads, more pairs than waves with one read of 100 000 among them, two threads, the refusals of the
chunk entry, the --gpu route's bytes, the one-command run."""
import ctypes
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import identity_restatement as ir
from conftest import BIN, ROOT, SIM_LIB
from rescue_restatement import read_fastx

EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
TOOL = os.path.join(BIN, "rtk_identity")
LIB = os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so")
GPU_STEP_TIMEOUT = 600  # seconds, every child process that opens the GPU
TOOL_MAX_LEN = 262144   # kMaxLen of csrc/tools/identity.cpp
if not os.path.exists(TOOL):  # (a tree built before the tool existed)
    import __graft_entry__
    __graft_entry__.build()


def _tool(args, env=None, timeout=None):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_THREADS="4", **(env or {})), timeout=timeout)


def _write_fastq(path, records):
    with open(path, "w") as f:
        for n, s in records:
            f.write("@%s extra words\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _write_fasta(path, records, width=70):
    with open(path, "w") as f:
        for n, s in records:
            f.write(">%s some description\n%s\n" % (n, "\n".join(s[i:i + width] for i in range(0, len(s), width))))


def _random_text(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _mutate(rng, s, rate):
    """Substitutions, insertions and deletions at about `rate` per base, 4 : 3 : 3."""
    if rate <= 0 or not s:
        return s
    out, u = [], rng.random(len(s))
    kind, base = rng.integers(0, 10, len(s)), rng.integers(0, 4, len(s))
    for i, c in enumerate(s):
        if u[i] >= rate:
            out.append(c)
        elif kind[i] < 4:
            out.append("ACGT"[(("ACGT".index(c) if c in "ACGT" else 0) + 1 + base[i] % 3) % 4])
        elif kind[i] < 7:
            out.append(c); out.append("ACGT"[base[i]])
    return "".join(out)


def _put(s, i, c):
    return s[:i] + c + s[i + 1:]


# ---------------------------------------------------------------------------------------------------------------- the simulated set (CPU tier, --gpu bytes)
class Data:
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """rtk_simulate --lr-truth: a diploid reference (two records) and 14 reads with where they come from. The reference is rewritten on lines of 60 with a
    lower-case stretch, an N and an R inside stretches that reads cover, and gzipped. l1 = the raw reads as FASTQ -- one in lower case, one with N / IUPAC bytes,
    one emptied, one that the truth does not know; l2 = a copy as multi-line FASTA in which every other read is closer to its truth and the rest further off."""
    d = Data(); d.tmp = str(tmp_path_factory.mktemp("identity"))
    pre = os.path.join(d.tmp, "sim")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "17", "--ref-len", "20000", "--het", "0.004", "--sr-cov", "1", "--lr-n", "14",
                           "--lr-len", "2000", "--lr-profile", "ont", "--lr-err", "0.08", "--lr-truth"], stderr=subprocess.DEVNULL)
    d.truth_fn = pre + ".lr.truth.tsv"
    d.truth = ir.parse_truth(d.truth_fn)
    recs = read_fastx(pre + ".ref.fa")
    assert len(recs) == 2 and len(d.truth) == 14 and {e[0] for e in d.truth.values()} == {0, 1} and {e[3] for e in d.truth.values()} == {False, True}
    raw = read_fastx(pre + ".lr.fq")
    rec0, s0, l0, _ = d.truth[raw[0][0]]
    seq = recs[rec0][1]
    seq = seq[:s0 + 10] + seq[s0 + 10:s0 + 200].lower() + seq[s0 + 200:]  # case is folded
    seq = _put(_put(seq, s0 + 300, "N"), s0 + 301, "R")                    # other bytes stay: an N equals an N only
    recs[rec0] = (recs[rec0][0], seq)
    d.records = [s for _, s in recs]
    d.ref_plain = pre + ".ref.fa"  # (as simulated: one line per record, no other bytes)
    d.ref = os.path.join(d.tmp, "ref60.fa.gz")
    with gzip.open(d.ref, "wt") as f:
        for n, s in recs:
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    rng = np.random.default_rng(20261021)
    raw[1] = (raw[1][0], raw[1][1].lower())
    raw[2] = (raw[2][0], _put(_put(_put(raw[2][1], 50, "N"), 51, "n"), 700, "Y"))
    raw[3] = (raw[3][0], "")
    d.rec1 = raw[:5] + [("ghost", "ACGTACGT" * 20)] + raw[5:]
    d.rec2 = []
    for i, (n, s) in enumerate(raw):
        t = ir.truth_of(d.records, d.truth[n])
        d.rec2.append((n, _mutate(rng, t, 0.01) if i % 2 == 0 else _mutate(rng, s, 0.02)))
    d.rec2.insert(2, ("ghost2", "TTTT"))
    d.l1, d.l2 = os.path.join(d.tmp, "l1.fq"), os.path.join(d.tmp, "l2.fa")
    _write_fastq(d.l1, d.rec1); _write_fasta(d.l2, d.rec2)
    d.want = ir.tables([(d.l1, d.rec1), (d.l2, d.rec2)], d.records, d.truth)
    return d


def _check_files(out, want, per_read=True):
    assert open(out + ".identity.tsv").read() == want[0]
    if per_read:
        assert open(out + ".identity.reads.tsv").read() == want[1]
    else:
        assert not os.path.exists(out + ".identity.reads.tsv")


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("chunk", [None, "4096"], ids=["one-chunk", "chunks-of-4096"])
def test_plain_two_files_against_the_restatement(data, tmp_path, chunk):
    out = str(tmp_path / "o")
    r = _tool(["-r", data.ref, "-t", data.truth_fn, "-l", data.l1, "-l", data.l2, "-o", out, "--per-read", "-v"], env={"RTK_INDEX_CHUNK": chunk} if chunk else None)
    assert r.returncode == 0, r.stderr
    _check_files(out, data.want)
    rows = [line.split("\t") for line in data.want[0].split("\n")[1:3]]
    assert rows[0][1:4] == ["15", "14", "1"] and rows[1][1:4] == ["15", "14", "1"] and rows[0][9] == "-"
    assert 0 < int(rows[1][9]) < 14                                # some reads of the second file are further from the truth, some are not
    assert 0.05 < float(rows[0][7]) < 0.5 and float(rows[1][8]) > float(rows[0][8])
    assert 0 in [len(s) for n, s in data.rec1 if n in data.truth]  # the empty read is aligned: its distance is the length of its truth
    for lap in ("reference", "truth", "distances"):
        assert re.search(r"rtk_identity: \[ *[0-9.]+ s\] %s" % lap, r.stderr), r.stderr
    assert r.stderr.endswith(data.want[0])  # the table is shown as well
    assert sorted(os.listdir(str(tmp_path))) == ["o.identity.reads.tsv", "o.identity.tsv"]


def test_plain_the_order_of_the_files_decides_further_and_a_list_file_works(data, tmp_path):
    out = str(tmp_path / "o")
    lst = str(tmp_path / "reads.txt")
    open(lst, "w").write(data.l2 + "\n" + data.l1 + "\n" + data.l2 + "\n")
    r = _tool(["-r", data.ref, "-t", data.truth_fn, "-l", lst, "-o", out])
    assert r.returncode == 0, r.stderr
    want = ir.tables([(data.l2, data.rec2), (data.l1, data.rec1), (data.l2, data.rec2)], data.records, data.truth)
    _check_files(out, want, per_read=False)
    further = [line.split("\t")[9] for line in want[0].split("\n")[1:4]]
    assert further[0] == "-" and int(further[1]) + int(further[2]) <= 14 and int(further[1]) > 0 and int(further[2]) > 0


def test_plain_reference_as_simulated_and_reads_without_any_truth(data, tmp_path):
    """The reference on one line per record; a -l file none of whose reads is in the truth: nan figures, like an empty file."""
    out = str(tmp_path / "o")
    ghosts, empty = str(tmp_path / "ghosts.fq"), str(tmp_path / "empty.fq")
    _write_fastq(ghosts, [("g1", "ACGT"), ("g2", "")]); open(empty, "w").close()
    r = _tool(["-r", data.ref_plain, "-t", data.truth_fn, "-l", ghosts, "-l", empty, "-l", data.l2, "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    records = [s for _, s in read_fastx(data.ref_plain)]
    want = ir.tables([(ghosts, [("g1", "ACGT"), ("g2", "")]), (empty, []), (data.l2, data.rec2)], records, data.truth)
    _check_files(out, want)
    lines = want[0].split("\n")
    assert lines[1].split("\t")[1:] == ["2", "0", "2", "0", "0", "0", "nan", "nan", "-"] and lines[2].split("\t")[1:] == ["0", "0", "0", "0", "0", "0", "nan", "nan", "0"]
    assert lines[3].split("\t")[9] == "0"  # no earlier file aligned any of its names


def test_refusals_exit_1_and_name_the_line_or_the_read(data, tmp_path):
    out = str(tmp_path / "o")
    good = open(data.truth_fn).read().split("\n")[:-1]
    name0 = good[0].split("\t")[0]
    cases = {"four columns": ("\t".join(good[1].split("\t")[:4]), r"line 2: malformed"),
             "a start that is no number": ("\t".join(good[1].split("\t")[:2] + ["12x"] + good[1].split("\t")[3:]), r"line 2: malformed"),
             "a strand that is neither": (good[1][:-1] + "*", r"line 2: malformed"),
             "a record that is not there": ("r\t2\t0\t10\t+", r"line 2: record 2 is not in"),
             "a stretch past its record": ("r\t1\t19990\t500\t+", r"line 2: the stretch 19990 \+ 500 lies outside record 1"),
             "a name twice": (name0 + "\t0\t0\t10\t-", r"line 2: the name %s is listed twice" % re.escape(name0))}
    for what, (line, msg) in cases.items():
        fn = str(tmp_path / "bad.tsv")
        open(fn, "w").write(good[0] + "\n" + line + "\n" + "\n".join(good[2:]) + "\n")
        r = _tool(["-r", data.ref, "-t", fn, "-l", data.l1, "-o", out, "--per-read"])
        assert r.returncode == 1 and re.search(msg, r.stderr), (what, r.returncode, r.stderr)
    big = str(tmp_path / "big.fa")
    open(big, "w").write(">big\n" + "ACGTTGCA" * 40000 + "\n")
    fn = str(tmp_path / "long.tsv")
    open(fn, "w").write("a\t0\t0\t%d\t+\nb\t0\t5\t%d\t-\n" % (TOOL_MAX_LEN, TOOL_MAX_LEN + 1))
    r = _tool(["-r", big, "-t", fn, "-l", data.l1, "-o", out])
    assert r.returncode == 1 and re.search(r"line 2: the stretch of %d characters is longer than the limit of %d" % (TOOL_MAX_LEN + 1, TOOL_MAX_LEN), r.stderr), r.stderr
    open(fn, "w").write("a\t0\t0\t100\t+\nb\t0\t5\t100\t-\n")
    reads = str(tmp_path / "long.fq")
    _write_fastq(reads, [("a", "ACGT" * 25), ("b", "A" * (TOOL_MAX_LEN + 1))])
    r = _tool(["-r", big, "-t", fn, "-l", reads, "-o", out, "--per-read"])
    assert r.returncode == 1 and re.search(r"read b of \S+ has %d characters, more than the limit of %d" % (TOOL_MAX_LEN + 1, TOOL_MAX_LEN), r.stderr), r.stderr
    r = _tool(["-r", data.ref, "-t", data.truth_fn, "-l", str(tmp_path / "missing.fq"), "-o", out])
    assert r.returncode == 1 and "missing.fq" in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]  # no run above left an output file


def test_usage_errors_exit_2(data, tmp_path):
    out = str(tmp_path / "o")
    full = ["-r", data.ref, "-t", data.truth_fn, "-l", data.l1, "-o", out]
    for args in (full[2:], full[:2] + full[4:], full[:4] + full[6:], full[:6], full + ["--frobnicate"], full[:-1], full + ["-k", "31"]):
        r = _tool(args)
        assert r.returncode == 2 and ("usage: rtk_identity" in r.stderr or "missing value" in r.stderr), (args, r.returncode, r.stderr)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("exe", [EXE, SIM_EXE], ids=["Ratatosk", "Ratatosk_sim"])
def test_cli_truth_options_go_together_and_belong_to_the_one_command_run(data, tmp_path, exe):
    out = str(tmp_path / "out")
    for args in (["-s", "x", "--truth-ref", data.ref], ["-s", "x", "--truth-tsv", data.truth_fn]):
        r = subprocess.run([exe, "correct"] + args + ["-l", "c", "-o", out], capture_output=True, text=True)
        assert r.returncode == 1 and "--truth-ref and --truth-tsv go together" in r.stderr, (args, r.stderr)
    r = subprocess.run([exe, "correct", "-s", "x", "--truth-ref", str(tmp_path / "none.fa"), "--truth-tsv", data.truth_fn, "-l", "c", "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "none.fa" in r.stderr
    r = subprocess.run([exe, "correct", "-1", "-g", "a", "-d", "b", "--truth-ref", data.ref, "--truth-tsv", data.truth_fn, "-l", "c", "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "rtk_identity --gpu -r" in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []
    assert "--truth-ref" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr


def test_header_and_libraries_hold_the_identity_entries():
    txt = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    for name in ("rtk_identity_begin", "rtk_identity_chunk", "rtk_identity_end"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        for path in (LIB, SIM_LIB):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    sim = ctypes.CDLL(SIM_LIB)
    job = ctypes.c_void_p()
    off = (ctypes.c_uint64 * 2)(0, 4)
    assert sim.rtk_identity_begin(0, b"ACGT", ctypes.c_uint64(4), off, 1, 16, ctypes.byref(job)) != 0  # as the QV entries there: not part of the simulator build
    assert sim.rtk_identity_chunk(None, None, ctypes.c_uint64(0), None, 0, None, None, None, None, None) != 0 and sim.rtk_identity_end(None, None, None) != 0


# ---------------------------------------------------------------------------------------------------------------- the shapes at which an aligner can go wrong
class Shapes:
    pass


@pytest.fixture(scope="module")
def shapes():
    """(read, truth, strand) triples and a reference of three records made of the truths laid end to end (a '-' truth lies there as its reverse complement), so
    that the first stretch of a record starts at offset 0 and the last one ends on the record's last byte. Distances from ref_edlib, once."""
    rng = np.random.default_rng(20261022)
    pairs = []  # (read, truth)
    for n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193):  # around a word, a row block (the last one-row-block sweep is 4096) and two
        for rate in (0.0, 0.07, 0.30):
            t = _random_text(rng, n)
            pairs.append((_mutate(rng, t, rate), t))
    a, b = _random_text(rng, 6000), _random_text(rng, 11000)
    pairs += [(a, b), (b, a)]                                            # a band far from the diagonal, both ways
    pairs += [(_random_text(rng, 5000), _random_text(rng, 10)), (_random_text(rng, 10), _random_text(rng, 5000)), ("", _random_text(rng, 300)), (_random_text(rng, 300), "")]
    pairs.append((_random_text(rng, 10000), _random_text(rng, 10000)))   # unrelated: the distance exceeds the first guess and the ring's widest band
    t = _random_text(rng, 8000)
    pairs.append((_mutate(rng, t, 0.02), t))                             # the ring
    t = _random_text(rng, 9000)
    pairs.append((_mutate(rng, t, 0.07), _put(_put(_put(t, 100, "N"), 5000, "R"), 8999, "*")))  # other bytes in the reference, several row blocks
    t = _random_text(rng, 3000)
    pairs.append((_put(_put(_put(_mutate(rng, t, 0.05), 7, "N"), 8, "Y"), 1500, "-"), _put(_put(t, 7, "N"), 2000, "N")))  # ... in read and reference, one row block
    s = Shapes(); s.reads, s.truths, s.entries = [], [], []
    records = [[], [], []]
    for i, (r, t) in enumerate(pairs):
        rev = i % 3 == 1
        rec = 0 if i < 12 else (1 if i < 30 else 2)
        start = sum(len(x) for x in records[rec])
        records[rec].append(ir.revcomp(t) if rev else t)
        s.reads.append(r); s.truths.append(t); s.entries.append((rec, start, len(t), rev))
    s.records = ["".join(x) for x in records]
    assert s.entries[0][1] == 0 and all(s.entries[i][1] + s.entries[i][2] == len(s.records[s.entries[i][0]]) for i in (11, 29, len(pairs) - 1))
    assert all(ir.truth_of(s.records, e) == t for e, t in zip(s.entries, s.truths))
    s.want = [ir.distance(r, t) for r, t in pairs]
    assert s.want[pairs.index((a, b))] >= 5000 and s.want[-4] > 4000 + 900  # (rtk_band_guess of a 10 000 pair is 3 900, RTK_RING_MAX_BAND 4 000)
    return s


def test_plain_edit_distance_on_the_shapes(shapes, tmp_path):
    """common/edit_distance.hpp through the tool: every shape of the GPU list, each read under its own name."""
    ref, tsv, fq, out = (str(tmp_path / n) for n in ("ref.fa", "truth.tsv", "reads.fq", "o"))
    _write_fasta(ref, [("rec%d" % i, s) for i, s in enumerate(shapes.records)], width=80)
    names = ["p%d" % i for i in range(len(shapes.reads))]
    open(tsv, "w").write("".join("%s\t%d\t%d\t%d\t%s\n" % (n, e[0], e[1], e[2], "-" if e[3] else "+") for n, e in zip(names, shapes.entries)))
    _write_fastq(fq, list(zip(names, shapes.reads)))
    r = _tool(["-r", ref, "-t", tsv, "-l", fq, "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    got = [int(line.split("\t")[4]) for line in open(out + ".identity.reads.tsv").read().split("\n")[1:-1]]
    assert got == shapes.want, [(i, len(shapes.reads[i]), len(shapes.truths[i]), g, w) for i, (g, w) in enumerate(zip(got, shapes.want)) if g != w]
    truth = {n: e for n, e in zip(names, shapes.entries)}
    known = dict(zip(zip(shapes.reads, shapes.truths), shapes.want))
    want = ir.tables([(fq, list(zip(names, shapes.reads)))], shapes.records, truth, dist=lambda s, t: known[(s, t)])
    _check_files(out, want)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_shapes_against_edlib(shapes):
    from ratatosk_amd import api
    st = {}
    got = api.identity_reads(shapes.records, shapes.reads, shapes.entries, stats=st)
    assert got == shapes.want, [(i, len(shapes.reads[i]), len(shapes.truths[i]), g, w) for i, (g, w) in enumerate(zip(got, shapes.want)) if g != w]
    assert st == {"n_chunks": 1, "n_pairs": len(shapes.reads), "sum_dist": sum(shapes.want)}
    low = api.identity_reads([r.lower() for r in shapes.records], [r.lower() for r in shapes.reads][::-1], shapes.entries[::-1])  # case is folded; other places in the chunk
    assert low == shapes.want[::-1]


@pytest.mark.gpu
def test_gpu_more_pairs_than_waves_and_one_read_of_100000_among_them():
    from ratatosk_amd import api
    rng = np.random.default_rng(20261023)
    ref = _random_text(rng, 400000)
    big_t = ref[150000:250000]
    big = _mutate(rng, big_t, 0.03)
    reads, entries, want = [], [], []
    for i in range(2000):
        start = (197 * i) % (len(ref) - 300)
        t = ref[start:start + 300]
        rev = i % 2 == 1
        reads.append(_mutate(rng, ir.revcomp(t) if rev else t, 0.08)); entries.append((0, start, 300, rev))
        want.append(ir.distance(reads[-1], ir.revcomp(t) if rev else t, dp=False))
    assert ir.dp_distance_batch(reads, [ir.revcomp(ref[e[1]:e[1] + 300]) if e[3] else ref[e[1]:e[1] + 300] for e in entries]) == want  # (the second checker, all pairs at once)
    reads.insert(1000, big); entries.insert(1000, (0, 150000, 100000, False)); want.insert(1000, ir.distance(big, big_t))
    st = {}
    got = api.identity_reads([ref], reads, entries, stats=st)
    assert got == want and st["n_chunks"] == 1 and st["n_pairs"] == 2001 > 1024 and 2000 < want[1000] < 3900  # (more pairs than the 1 024 waves of a chunk)


@pytest.mark.gpu
def test_gpu_two_threads_feed_the_chunks(shapes):
    from ratatosk_amd import api
    st1, st2 = {}, {}
    one = api.identity_reads(shapes.records, shapes.reads, shapes.entries, max_chunk=20000, threads=1, stats=st1)
    two = api.identity_reads(shapes.records, shapes.reads, shapes.entries, max_chunk=20000, threads=2, stats=st2)
    assert st1["n_chunks"] == st2["n_chunks"] >= 8 and st1 == st2
    assert one == two == shapes.want


@pytest.mark.gpu
def test_gpu_a_stretch_outside_its_record_or_a_length_above_max_len_is_refused(shapes):
    from ratatosk_amd import api
    recs = ["ACGT" * 25, "TTGCA" * 10]
    ok = api.identity_reads(recs, ["ACGTACGT", "TGCAA"], [(0, 0, 8, False), (1, 45, 5, True)])
    assert ok == [0, 0]
    for entries, msg in (([(0, 0, 8, False), (1, 46, 5, False)], "the stretch of read 1 lies outside record 1"), ([(0, 96, 8, False), (1, 0, 5, False)], "the stretch of read 0 lies outside record 0"),
                         ([(2, 0, 8, False), (1, 0, 5, False)], "read 0 names record 2 of 2")):
        with pytest.raises(api.RtkError, match=msg):
            api.identity_reads(recs, ["ACGTACGT", "TGCAA"], entries)
    with pytest.raises(api.RtkError, match="longer than the job's max_len 6"):
        api.identity_reads(recs, ["ACGTACGT", "TGCAA"], [(0, 0, 6, False), (1, 0, 5, False)], max_len=6)
    assert api.identity_reads(recs, ["ACGTACGT", "TGCAA"], [(0, 0, 8, False), (1, 45, 5, True)]) == [0, 0]  # the device answers as before


@pytest.mark.gpu
def test_gpu_tool_writes_the_plain_routes_bytes(data, tmp_path):
    args = ["-r", data.ref, "-t", data.truth_fn, "-l", data.l1, "-l", data.l2, "--per-read"]
    plain = str(tmp_path / "plain")
    assert _tool(args + ["-o", plain]).returncode == 0
    for name, chunk, least in (("dev", None, 2), ("dev_chunks", "4096", 8)):  # (a chunk holds the reads of one file)
        dev = str(tmp_path / name)
        r = _tool(["--gpu"] + args + ["-o", dev], env=dict({"RTK_INDEX_TRACE": "1"}, **({"RTK_INDEX_CHUNK": chunk} if chunk else {})), timeout=GPU_STEP_TIMEOUT)
        assert r.returncode == 0, r.stderr
        assert int(re.search(r"characters in (\d+) chunks", r.stderr).group(1)) >= least, r.stderr
        for ext in (".identity.tsv", ".identity.reads.tsv"):
            assert open(dev + ext, "rb").read() == open(plain + ext, "rb").read(), (name, ext)
    _check_files(str(tmp_path / "dev_chunks"), data.want)


@pytest.mark.gpu
def test_gpu_one_command_run_with_the_truth(tmp_path):
    pre = str(tmp_path / "small")  # the ds_small set, with its truth
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "40", "--sr-err", "0.01",
                           "--lr-n", "12", "--lr-len", "3000", "--lr-profile", "ont", "--lr-err", "0.08", "--lr-truth"], stderr=subprocess.DEVNULL)
    sr, lr, ref, tsv = pre + ".sr.fq", pre + ".lr.fq", pre + ".ref.fa", pre + ".lr.truth.tsv"
    b = str(tmp_path / "b"); os.mkdir(b)
    out = os.path.join(b, "out")
    r = subprocess.run([EXE, "correct", "-c", "2", "-s", sr, "-l", lr, "-o", out, "--truth-ref", ref, "--truth-tsv", tsv], capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(b)) == ["out.fastq", "out.identity.tsv"]
    table = open(out + ".identity.tsv").read()
    lines = table.split("\n")
    assert lines[0] == ir.HEADER and len(lines) == 4 and table in r.stderr
    before, after = lines[1].split("\t"), lines[2].split("\t")
    assert before[0] == lr and after[0] == out + ".fastq" and before[1:4] == after[1:4] == ["12", "12", "0"]
    assert float(after[7]) < float(before[7]) and before[9] == "-" and 0 <= int(after[9]) < 12
    other = str(tmp_path / "other")
    assert _tool(["-r", ref, "-t", tsv, "-l", lr, "-l", out + ".fastq", "-o", other]).returncode == 0  # a separate run, on the host
    assert open(other + ".identity.tsv").read() == table
    records = [s for _, s in read_fastx(ref)]
    want = ir.tables([(lr, read_fastx(lr)), (out + ".fastq", read_fastx(out + ".fastq"))], records, ir.parse_truth(tsv))
    assert want[0] == table
