"""Graph reuse in the index build (DESIGN.md section 4 [A15]): `rtk_build_index --graph-only` writes the unitig FASTA of a build and stops;
`--graph-from FILE` takes the graph of a build from such a file -- every all-A/C/G/T window of length k of its records, each once, whatever k the file
was written with -- and lets `-s` / `--colour-reads` only colour and cover it; `Ratatosk correct -s ... --k1-from-k2` chains them the way the reference's
one-command run does (src/Ratatosk.cpp:1062-1068, 1092-1101, 1194: the short reads counted once at k2, the k1 graph from the text of the k2 unitigs,
the same k2 graph for the second pass). Held to the tool's own full build where the two must write the same bytes (equal k), and to the independent
oracle (oracle/oracle_index.py) where they must not (k1 from k2). The small helpers are copies of those of tests/test_index_build.py."""
import gzip
import os
import random
import re
import subprocess

import pytest

from conftest import BIN

TOOL = os.path.join(BIN, "rtk_build_index")
EXE = os.path.join(BIN, "Ratatosk")
MODES = ([], ["--fast"])
# 20 kb diploid, 0.5 % read errors: 31-mers that recur only inside erroneous 63-mers exist (test 3 asserts it)
K1K2_SET = ["--seed", "3", "--ref-len", "20000", "--het", "0.004", "--sr-cov", "30", "--sr-err", "0.005"]
# 30 kb diploid with two-copy repeats (ORACLE_SETS[0] of tests/test_index_build.py): branching graph, SNP bubbles, global colour sets
MAIN_SET = ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "30", "--sr-err", "0.01"]
# GPU tier: 70 kb, nearly haploid, few read errors: unitigs of more than two 4 kb chunks (the longest 12 kb) next to a few SNP bubbles
GPU_SET = ["--seed", "5", "--ref-len", "70000", "--het", "0.0001", "--sr-cov", "30", "--sr-err", "0.002", "--lr-n", "30", "--lr-len", "3000", "--lr-err", "0.08"]
# the set of tests/test_cli_one_command.py
SIM_ARGS = ["--seed", "17", "--ref-len", "60000", "--het", "0.003", "--repeat-frac", "0.05", "--sr-cov", "30", "--sr-err", "0.005",
            "--lr-n", "40", "--lr-len", "3000", "--lr-err", "0.08"]
GPU_TIMEOUT = 120


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _simulated(tmp, name, args):
    pre = os.path.join(tmp, name)
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + args + ([] if "--lr-n" in args else ["--lr-n", "6", "--lr-len", "1500"]), stderr=subprocess.DEVNULL)
    return pre + ".sr.fq", pre + ".lr.fq"


def _self_meeting_genomes(tmp):
    """Reads tiling (a) a circular 600 bp sequence -- a closed loop without an end -- and (b) W + reverse complement of W (hairpin)."""
    rnd = random.Random(5)
    circ = "".join(rnd.choice("ACGT") for _ in range(600))
    w = "".join(rnd.choice("ACGT") for _ in range(300))
    hair = w + _rc(w)
    sr = os.path.join(tmp, "self.sr.fq")
    with open(sr, "w") as f:
        n = 0
        for rep in range(3):
            for start in range(0, 600, 7):
                s = (circ + circ)[start:start + 100]
                f.write("@c%d\n%s\n+\n%s\n" % (n, s, "I" * 100)); n += 1
            for start in range(0, len(hair) - 100 + 1, 5):
                s = hair[start:start + 100]
                f.write("@h%d\n%s\n+\n%s\n" % (n, s, "I" * 100)); n += 1
    return sr


def _tool(args, env=None, timeout=None):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})), timeout=timeout)


def _ok(args, env=None, timeout=None):
    r = _tool(args, env, timeout)
    assert r.returncode == 0, (args, r.stderr)
    return r


def _fasta(prefix, k):
    return prefix + ".index.k%d.fasta.gz" % k


def _rtsk(prefix, k):
    return prefix + ".index.k%d.rtsk" % k


def _files(prefix, k):
    return open(_fasta(prefix, k), "rb").read(), open(_rtsk(prefix, k), "rb").read()


def _unitigs(path):
    return [l for l in gzip.open(path, "rt").read().split("\n") if l and l[0] != ">"]


@pytest.fixture(scope="module")
def main_set(tmp_path_factory):
    return _simulated(str(tmp_path_factory.mktemp("graph_reuse")), "main", MAIN_SET)


# ---------------------------------------------------------------------------------------------------------------- 1. --graph-only
@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_graph_only_writes_the_fasta_of_the_full_build_and_no_rtsk(tmp_path, main_set, mode):
    tmp = str(tmp_path); sr = main_set[0]
    for k in (21, 31, 63):
        full, only, stale = os.path.join(tmp, "full"), os.path.join(tmp, "only"), os.path.join(tmp, "stale")
        _ok(["-s", sr, "-k", str(k), "-o", full] + mode)
        r = _ok(["-s", sr, "-k", str(k), "-o", only, "--graph-only"] + mode)
        assert open(_fasta(only, k), "rb").read() == open(_fasta(full, k), "rb").read(), k
        assert not os.path.exists(_rtsk(only, k))
        assert "unitigs built" in r.stderr and "files written" in r.stderr and "colours and coverage done" not in r.stderr, r.stderr
        assert "graph from the reads of -s" in r.stderr, r.stderr
        open(_rtsk(stale, k), "wb").write(b"an index of an earlier run\n")
        _ok(["-s", sr, "-k", str(k), "-o", stale, "--graph-only", "--no-short-cycles"] + mode)  # (--no-short-cycles: accepted, nothing to do)
        assert open(_rtsk(stale, k), "rb").read() == b"an index of an earlier run\n"
        assert open(_fasta(stale, k), "rb").read() == open(_fasta(full, k), "rb").read(), k
    # --min-count is the full build's too
    _ok(["-s", sr, "-k", "31", "--min-count", "3", "-o", os.path.join(tmp, "full3")] + mode)
    _ok(["-s", sr, "-k", "31", "--min-count", "3", "-o", os.path.join(tmp, "only3"), "--graph-only"] + mode)
    assert open(_fasta(os.path.join(tmp, "only3"), 31), "rb").read() == open(_fasta(os.path.join(tmp, "full3"), 31), "rb").read()
    assert open(_fasta(os.path.join(tmp, "only3"), 31), "rb").read() != open(_fasta(os.path.join(tmp, "full"), 31), "rb").read()


# ---------------------------------------------------------------------------------------------------------------- 2. equal-k round trip
def _round_trip(tmp, sr, k, mode, extra=()):
    """--graph-only, then --graph-from that file with -s: the two files of the build from the reads"""
    g, a, b = os.path.join(tmp, "g"), os.path.join(tmp, "from_reads"), os.path.join(tmp, "from_graph")
    _ok(["-s", sr, "-k", str(k), "-o", g, "--graph-only"] + mode)
    _ok(["-s", sr, "-k", str(k), "-o", a, "--snps"] + list(extra) + mode)
    r = _ok(["--graph-from", _fasta(g, k), "-s", sr, "-k", str(k), "-o", b, "--snps"] + list(extra) + mode)
    assert "graph from --graph-from " + _fasta(g, k) in r.stderr, r.stderr
    want, got = _files(a, k), _files(b, k)
    assert got[0] == want[0], (k, mode, extra, "unitig FASTA differs")
    assert got[1] == want[1], (k, mode, extra, ".rtsk differs")
    return len(_unitigs(_fasta(b, k)))


@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_a_graph_survives_its_own_fasta(tmp_path, main_set, mode):
    tmp = str(tmp_path)
    for k in (31, 63):
        assert _round_trip(tmp, main_set[0], k, mode) > 10
    assert _round_trip(tmp, main_set[0], 31, mode, ["--merge-duplicates", "--subsample-colours"]) > 10


@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_round_trip_of_chains_that_meet_themselves_and_of_microsatellites(tmp_path, mode):
    tmp = str(tmp_path)
    sr = _self_meeting_genomes(tmp)
    for k in (31, 63):
        assert _round_trip(tmp, sr, k, mode) >= 2  # the loop (written as 600 + k - 1 characters, read back whole) and the hairpin
    import hard_genomes as hg
    pre = os.path.join(tmp, "micro")
    hg.write_set(pre, seed=102, kind="microsatellite")
    for k in (31, 63):
        assert _round_trip(tmp, pre + ".sr.fq", k, mode) > 10


@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_second_pass_index_from_a_graph_file_needs_no_short_reads(tmp_path, main_set, mode):
    tmp = str(tmp_path); sr, lr = main_set
    for k in (31, 63):
        g, a, b, c = (os.path.join(tmp, x) for x in ("g", "with_s", "without_s", "from_reads"))
        _ok(["-s", sr, "-k", str(k), "-o", g, "--graph-only"] + mode)
        colour = ["--colour-reads", lr, "--colour-min-conf", "0", "--colour-min-len", "500", "-k", str(k)]
        _ok(["--graph-from", _fasta(g, k), "-s", sr, "-o", a] + colour + mode)
        _ok(["--graph-from", _fasta(g, k), "-o", b] + colour + mode)
        _ok(["-s", sr, "-o", c] + colour + mode)
        assert _files(a, k) == _files(b, k) == _files(c, k), (k, mode)


# ---------------------------------------------------------------------------------------------------------------- 3. k1 from k2, against the oracle
def _index_is(prefix, k, want, n_kmers):
    """the index files at `prefix` hold exactly the unitigs (up to strand; loops up to rotation), colour sets and coverages of `want`
    ({unitig key: (ids, coverage)} of oracle_index) -- the comparison of tests/test_index_build.py::_index_vs_oracle"""
    from oracle import oracle_index as oi
    from oracle import oracle_py as op
    g = op.Graph(_fasta(prefix, k), _rtsk(prefix, k), k)
    assert g.n_kmers == n_kmers, (g.n_kmers, n_kmers)
    got = {}
    for u in range(g.n_unitigs):
        d = g.unitig(u)
        ids = sorted(set(d["local"]) | (set(g.global_set(d["global_id"])) if d["global_id"] >= 0 else set()))
        got[oi.canonical(d["seq"])] = (ids, (d["kmcov"] >> 31) & 0x7FFFFFFF, d["seq"])
    assert len(got) == g.n_unitigs == len(want), (g.n_unitigs, len(want))
    missing = [key for key in want if key not in got]
    if missing:
        rot = {oi.unitig_key(v[2], k, True): v for key, v in got.items() if key not in want}
        for key in missing:
            assert key in rot, ("unitig of the oracle not in the index", key[:80])
            got[key] = rot[key]
    bad = [(key[:50], want[key][1], got[key][1]) for key in want if want[key][1] != got[key][1]]
    assert not bad, ("coverage differs", bad[:5])
    bad = [key[:50] for key in want if want[key][0] != got[key][0]]
    assert not bad, ("colour sets differ", bad[:5])


def _oracle_composition(sr, k_graph, k_index, graph_min_count=2):
    """the oracle's index at k_index of the graph that the unitigs of the reads' k_graph graph spell: (want, its k-mers, the k_index-mers solid in the reads)"""
    from oracle import oracle_index as oi
    recs = oi.read_fastx(sr)
    seqs = [s for _, s in recs]
    s_graph = oi.solid_kmers(seqs, k_graph, graph_min_count)
    u_graph, _ = oi.build_unitigs(s_graph, k_graph)
    s_index = oi.solid_kmers(u_graph, k_index, 1)
    unitigs, circ = oi.build_unitigs(s_index, k_index)
    col, cov = oi.colour_and_cover(unitigs, k_index, seqs, oi.pair_ids([n for n, _ in recs]))
    want = {oi.unitig_key(u, k_index, c): (col[i], cov[i]) for i, (u, c) in enumerate(zip(unitigs, circ))}
    return want, s_index, oi.solid_kmers(seqs, k_index, 2)


def test_k1_graph_from_the_k2_unitigs_is_the_oracles(tmp_path):
    """S63 = the 63-mers seen twice, U63 their unitigs, S31 = every 31-mer of the text of U63: the index `--graph-only -k 63` + `--graph-from ... -k 31 -s SR`
    writes is the oracle's index over S31 -- which is NOT the graph of the 31-mers seen twice (asserted: a proper subset of it on this set)"""
    tmp = str(tmp_path)
    sr, _ = _simulated(tmp, "k1k2", K1K2_SET)
    want, s31, from_reads = _oracle_composition(sr, 63, 31)
    assert s31 <= from_reads and len(s31) < len(from_reads), (len(s31), len(from_reads))  # else the test shows nothing
    outs = []
    for mode in MODES:
        g, out = os.path.join(tmp, "g" + "".join(mode)), os.path.join(tmp, "k1" + "".join(mode))
        _ok(["-s", sr, "-k", "63", "-o", g, "--graph-only"] + mode)
        _ok(["--graph-from", _fasta(g, 63), "-s", sr, "-k", "31", "-o", out] + mode)
        _index_is(out, 31, want, len(s31))
        outs.append(_files(out, 31))
    assert outs[0] == outs[1]  # plain == --fast, byte for byte
    # and it is another index than the one from the reads
    _ok(["-s", sr, "-k", "31", "-o", os.path.join(tmp, "reads")])
    assert _files(os.path.join(tmp, "reads"), 31)[0] != outs[0][0]


def test_k2_graph_from_a_k1_file_is_the_windows_inside_its_unitigs(tmp_path):
    """a k above the file's own: defined by the same sentence (the windows of 63 inside the unitigs of the 31-mer graph), and runs"""
    tmp = str(tmp_path)
    sr, _ = _simulated(tmp, "k2k1", K1K2_SET)
    want, s63, _ = _oracle_composition(sr, 31, 63)
    assert len(s63) > 1000
    for mode in MODES:
        g, out = os.path.join(tmp, "g"), os.path.join(tmp, "k2")
        _ok(["-s", sr, "-k", "31", "-o", g, "--graph-only"] + mode)
        _ok(["--graph-from", _fasta(g, 31), "-s", sr, "-k", "63", "-o", out] + mode)
        _index_is(out, 63, want, len(s63))


# ---------------------------------------------------------------------------------------------------------------- 4. refusals and edges
def test_option_clashes_are_refused_by_name(tmp_path, main_set):
    tmp = str(tmp_path); sr, lr = main_set
    out = os.path.join(tmp, "out")
    g = os.path.join(tmp, "g")
    _ok(["-s", sr, "-o", g, "--graph-only"])
    gf = _fasta(g, 31)
    for clash, extra in (("--snps", ["--snps"]), ("--colour-reads", ["--colour-reads", lr]), ("--colour-reads", ["--colour-reads", lr, "--colour-min-conf", "0.5"]),
                         ("--colour-min-conf", ["--colour-min-conf", "0.5"]), ("--colour-max-qual", ["--colour-max-qual", "30"]), ("--colour-min-len", ["--colour-min-len", "5"]),
                         ("--merge-duplicates", ["--merge-duplicates"]), ("--subsample-colours", ["--subsample-colours"]), ("--graph-from", ["--graph-from", gf])):
        r = _tool(["-s", sr, "-o", out, "--graph-only"] + extra)
        assert r.returncode == 2, (extra, r.stderr)
        lines = r.stderr.strip().split("\n")
        assert len(lines) == 1 and "--graph-only" in lines[0] and clash in lines[0], (extra, r.stderr)
    r = _tool(["--graph-from", gf, "-s", sr, "--min-count", "1", "-o", out])
    assert r.returncode == 2 and "--min-count" in r.stderr and "--graph-from" in r.stderr and len(r.stderr.strip().split("\n")) == 1, r.stderr
    r = _tool(["--graph-from", gf, "-o", out])
    assert r.returncode == 2 and "--graph-from" in r.stderr and "-s" in r.stderr and "--colour-reads" in r.stderr and len(r.stderr.strip().split("\n")) == 1, r.stderr
    r = _tool(["-o", out])  # (neither -s nor a graph: the usage text, as before)
    assert r.returncode == 2 and r.stderr.startswith("usage:") and "--graph-only" in r.stderr and "--graph-from" in r.stderr
    r = _tool(["--colour-reads", lr, "-o", out])  # --colour-reads alone gives no graph
    assert r.returncode == 2 and r.stderr.startswith("usage:")
    assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)


@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_graph_files_without_a_kmer_or_without_a_file(tmp_path, main_set, mode):
    tmp = str(tmp_path); sr, lr = main_set
    out = os.path.join(tmp, "out")
    short = os.path.join(tmp, "short.fa")
    open(short, "w").write(">a\n%s\n>b\n%s\n>c\n%s\n" % ("ACGT" * 7, "ACGTTGCA" * 3 + "N" + "ACGGT" * 5, "acgtn" * 40))  # 28, 24 + N + 25, and an n every five
    for colour in (["-s", sr], ["--colour-reads", lr]):
        r = _tool(["--graph-from", short, "-k", "31", "-o", out] + colour + mode)
        assert r.returncode == 1 and "no k-mer of length 31 in " + short in r.stderr, r.stderr
        r = _tool(["--graph-from", os.path.join(tmp, "missing.fa.gz"), "-k", "31", "-o", out] + colour + mode)
        assert r.returncode == 1 and "cannot open" in r.stderr and "missing.fa.gz" in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)
    r = _ok(["--graph-from", short, "-k", "21", "-s", sr, "-o", out] + mode)  # at k = 21 the same file has k-mers
    assert len(_unitigs(_fasta(out, 21))) >= 1


@pytest.mark.parametrize("mode", MODES, ids=["plain", "fast"])
def test_graph_file_with_n_lower_case_and_several_lines(tmp_path, mode):
    """no window across an N (or any other letter); lower case is a base as in -s; multi-line FASTA, gzip of several members and a second
    --graph-from: the graph is the oracle's k-mer set of the texts, its unitigs the oracle's"""
    from oracle import oracle_index as oi
    tmp = str(tmp_path); rnd = random.Random(9)
    rand = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    a, b, c, d = rand(400), rand(300), rand(250), rand(200)
    texts = [a[:200] + "N" + a[200:], b.lower(), c[:100] + "R" + c[100:130] + "n" + c[130:], d, _rc(d)[50:120], a[150:260]]  # (the last: the window the N breaks; a record twice)
    f1, f2 = os.path.join(tmp, "one.fa"), os.path.join(tmp, "two.fa.gz")
    with open(f1, "w") as f:
        for i, t in enumerate(texts[:3]):
            f.write(">r%d some text\n" % i + "".join(t[j:j + 60] + "\n" for j in range(0, len(t), 60)))
    open(f2, "wb").write(b"".join(gzip.compress((">m%d\n%s\n" % (i, t)).encode()) for i, t in enumerate(texts[3:])))
    sr = os.path.join(tmp, "sr.fq")
    with open(sr, "w") as f:
        for i in range(0, 340, 9):
            f.write("@p%d/1\n%s\n+\n%s\n@p%d/2\n%s\n+\n%s\n" % (i, a[i:i + 60], "I" * 60, i, _rc(b[i % 240:i % 240 + 60]), "I" * 60))
    for k in (31, 21):
        solid = oi.solid_kmers([t.upper() for t in texts], k, 1)
        assert oi.canonical(a[190:190 + k]) in solid and oi.canonical(c[95:95 + k]) not in solid and oi.canonical(b[0:k]) in solid  # (from the last record only; across the R; the lower-case record)
        unitigs, circ = oi.build_unitigs(solid, k)
        recs = oi.read_fastx(sr)
        col, cov = oi.colour_and_cover(unitigs, k, [s for _, s in recs], oi.pair_ids([n for n, _ in recs]))
        want = {oi.unitig_key(u, k, x): (col[i], cov[i]) for i, (u, x) in enumerate(zip(unitigs, circ))}
        out = os.path.join(tmp, "out")
        _ok(["--graph-from", f1, "--graph-from", f2, "-s", sr, "-k", str(k), "-o", out] + mode)
        _index_is(out, k, want, len(solid))


# ---------------------------------------------------------------------------------------------------------------- 5. the driver, without a GPU
def test_driver_refuses_the_flag_next_to_a_prebuilt_index_and_names_the_graph_step(tmp_path):
    tmp = str(tmp_path)
    out = os.path.join(tmp, "out")
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    for mode in (["-1"], ["-2", "-L", lr]):
        r = subprocess.run([EXE, "correct", "--k1-from-k2", "-g", "a", "-d", "b", "-l", lr, "-o", out] + mode, capture_output=True, text=True)
        assert r.returncode == 1 and "--k1-from-k2" in r.stderr and "pre-built index" in r.stderr, r.stderr
    for mode in ([], ["-1"]):
        r = subprocess.run([EXE, "correct", "--k1-from-k2"] + mode + ["-s", os.path.join(tmp, "missing.fq"), "-l", lr, "-o", out], capture_output=True, text=True, timeout=GPU_TIMEOUT)
        assert r.returncode != 0, (mode, r.stderr)
        assert "step 1a (k2 graph, rtk_build_index) failed" in r.stderr, (mode, r.stderr)
        assert "step 1 (" not in r.stderr and "step 2" not in r.stderr, (mode, r.stderr)  # nothing is tried after it
        assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)
    # -2 alone builds its graph from the short reads in the reference as well: the flag is accepted, the chain is the one of before
    r = subprocess.run([EXE, "correct", "--k1-from-k2", "-2", "-L", lr, "-s", os.path.join(tmp, "missing.fq"), "-l", lr, "-o", out], capture_output=True, text=True, timeout=GPU_TIMEOUT)
    assert r.returncode != 0 and "step 3 (k2 index, rtk_build_index) failed" in r.stderr and "step 1a" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--k1-from-k2" in r.stderr + r.stdout


# ---------------------------------------------------------------------------------------------------------------- 6. --gpu writes the plain tool's bytes
def _gpu(args, env=None):
    r = _ok(["--gpu"] + args, env, timeout=GPU_TIMEOUT)
    # counted and walked on the device, not on the host threads behind a failed call
    assert "rtk_index_count_kmers:" in r.stderr and "rtk_index_unitigs:" in r.stderr, r.stderr
    assert "unitigs on the host threads" not in r.stderr and "colours on the host threads" not in r.stderr, r.stderr
    return r.stderr


@pytest.fixture(scope="module")
def gpu_set(tmp_path_factory):
    """the set, and the files the plain tool writes for the three commands (computed once)"""
    tmp = str(tmp_path_factory.mktemp("graph_reuse_gpu"))
    sr, lr = _simulated(tmp, "g", GPU_SET)
    g, i1, i2 = (os.path.join(tmp, x) for x in ("plain_g", "plain_i1", "plain_i2"))
    _ok(["-s", sr, "-k", "63", "-o", g, "--graph-only"])
    _ok(["--graph-from", _fasta(g, 63), "-k", "31", "-s", sr, "--snps", "-o", i1])
    _ok(["--graph-from", _fasta(g, 63), "-k", "63", "--colour-reads", lr, "-o", i2])
    assert max(len(u) for u in _unitigs(_fasta(g, 63))) > 2 * 4096  # else RTK_INDEX_CHUNK=4096 cuts no unitig twice
    return dict(tmp=tmp, sr=sr, lr=lr, graph=open(_fasta(g, 63), "rb").read(), i1=_files(i1, 31), i2=_files(i2, 63))


@pytest.mark.gpu
@pytest.mark.parametrize("env,min_parts", [({}, 1), ({"RTK_INDEX_CHUNK": "4096"}, 1), ({"RTK_INDEX_CAP": "1048576"}, 2)], ids=["default", "chunk4096", "partitions"])
def test_gpu_graph_reuse_writes_the_plain_tools_bytes(tmp_path, gpu_set, env, min_parts):
    """the three commands of the chain with --gpu; again with the unitigs of the graph file cut into 4 kb pieces on their way to the k-mer kernel (a window
    lost at a cut would be a lost vertex: every k-mer is there once), and with the k-mer space counted in two or more partitions"""
    tmp = str(tmp_path); s = gpu_set
    g, i1, i2 = (os.path.join(tmp, x) for x in ("g", "i1", "i2"))
    traces = [_gpu(["-s", s["sr"], "-k", "63", "-o", g, "--graph-only"], env)]
    assert open(_fasta(g, 63), "rb").read() == s["graph"] and not os.path.exists(_rtsk(g, 63))
    traces.append(_gpu(["--graph-from", _fasta(g, 63), "-k", "31", "-s", s["sr"], "--snps", "-o", i1], env))
    assert _files(i1, 31) == s["i1"]
    traces.append(_gpu(["--graph-from", _fasta(g, 63), "-k", "63", "--colour-reads", s["lr"], "-o", i2], env))
    assert _files(i2, 63) == s["i2"]
    for t in traces:
        n_part = int(re.search(r"solid k-mers from (\d+) partition\(s\)", t).group(1))
        assert n_part >= min_parts, t
        if not env:
            assert n_part == 1, t  # a graph file of this size is counted in one pass, without a restart
            assert t.count("partition 1 of 1 starts") == 1, t


# ---------------------------------------------------------------------------------------------------------------- 7. one command = the five by hand
def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=GPU_TIMEOUT)
    assert r.returncode == 0, (args, r.stderr)
    return r


@pytest.mark.gpu
def test_gpu_one_command_with_k1_from_k2_equals_the_five_steps(tmp_path):
    tmp = str(tmp_path)
    pre = os.path.join(tmp, "s")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + SIM_ARGS, stderr=subprocess.DEVNULL)
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    hand = os.path.join(tmp, "hand")
    _run([TOOL, "--gpu", "--graph-only", "-k", "63", "-s", sr, "-o", hand + "_g"])
    graph = hand + "_g.index.k63.fasta.gz"
    _run([TOOL, "--gpu", "--graph-from", graph, "-k", "31", "-s", sr, "--snps", "-o", hand + "_i1"])
    _run([EXE, "correct", "-1", "-c", "2", "-g", hand + "_i1.index.k31.fasta.gz", "-d", hand + "_i1.index.k31.rtsk", "-l", lr, "-o", hand])
    _run([TOOL, "--gpu", "--graph-from", graph, "-k", "63", "--colour-reads", hand + ".2.fastq", "--snps", "-o", hand + "_i2"])
    _run([EXE, "correct", "-2", "-c", "2", "-g", hand + "_i2.index.k63.fasta.gz", "-d", hand + "_i2.index.k63.rtsk", "-l", hand + ".2.fastq", "-L", lr, "-o", hand])
    want = open(hand + ".fastq", "rb").read()
    assert want.count(b"\n") >= 4 * 40
    # one command
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = _run([EXE, "correct", "-v", "-c", "2", "-s", sr, "-l", lr, "-o", out, "--k1-from-k2"])
    assert r.stderr.index("Building graph from short reads (1/2).") < r.stderr.index("step 1a (k2 graph, rtk_build_index)") < r.stderr.index("step 1 (k1 index")
    assert "--graph-only" in r.stderr and r.stderr.count("--graph-from") == 2, r.stderr
    step3 = [l for l in r.stderr.split("\n") if l.startswith("Ratatosk::correct: step 3")][0]
    assert " -s " not in step3 and "--graph-from" in step3 and "--colour-reads" in step3, step3
    assert open(out + ".fastq", "rb").read() == want
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)  # the graph file, the indexes and OUT.2.fastq removed
    # two steps: -1 with the flag, then -2
    subt = os.path.join(tmp, "two"); os.mkdir(subt)
    out = os.path.join(subt, "out")
    _run([EXE, "correct", "-1", "-c", "2", "-s", sr, "-l", lr, "-o", out, "--k1-from-k2"])
    assert open(out + ".2.fastq", "rb").read() == open(hand + ".2.fastq", "rb").read()
    assert sorted(os.listdir(subt)) == ["out.2.fastq"], os.listdir(subt)
    _run([EXE, "correct", "-2", "-c", "2", "-s", sr, "-l", out + ".2.fastq", "-L", lr, "-o", out])
    assert open(out + ".fastq", "rb").read() == want
    assert sorted(os.listdir(subt)) == ["out.2.fastq", "out.fastq"], os.listdir(subt)
