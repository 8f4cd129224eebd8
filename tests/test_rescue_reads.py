"""Rescue of unmapped short reads before the index build (`Ratatosk correct -u`, tools rtk_rescue_reads, library entries rtk_rescue_begin / _chunk /
_end; reference: retrieveMissingReads, src/Graph.cpp:3857-4131). Parity is to the exact restatement of DESIGN.md section 4 [A11], written out in
tests/rescue_restatement.py: a -u read is kept when at least 31 of its start positions spell a k-mer seen twice in the long reads and not twice in the -s reads.

Data: genome A (60 kb) with its short reads as -s; genome B (20 kb, the novel sequence) and genome C (20 kb, contamination without long reads); long reads of A
and B at 40x / 5 % error (an error-free 31-mer of a read has probability ~0.2, so ~8 clean copies per position: nearly every k-mer of B is seen twice; at a few x
the long-read set would be empty and every test here vacuous). -u: the short reads of B and C and a slice of A's, interleaved, plus reads shorter than k, in
lower case, with N, and with exactly 30 and exactly 31 qualifying positions."""
import ctypes
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rescue_restatement as rr
from conftest import BIN, ROOT, SIM_LIB

EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
TOOL = os.path.join(BIN, "rtk_rescue_reads")
LIB = os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so")
GPU_STEP_TIMEOUT = 600  # seconds, every child process that opens the GPU

if not os.path.exists(TOOL):  # (a tree built before the tool existed)
    import __graft_entry__
    __graft_entry__.build()


def _sim(tmp, name, seed, ref_len, extra=()):
    pre = os.path.join(tmp, name)
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", str(seed), "--ref-len", str(ref_len), "--sr-cov", "30"] + list(extra), stderr=subprocess.DEVNULL)
    return pre


def _write_fastq(path, records):
    with open(path, "w") as f:
        for n, s in records:
            f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class Data:
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("rescue"))
    d = Data(); d.tmp = tmp
    lr_args = ["--lr-cov", "40", "--lr-len", "3000", "--lr-err", "0.05", "--lr-truth"]
    a = _sim(tmp, "A", 101, 60000, lr_args); b = _sim(tmp, "B", 202, 20000, lr_args); c = _sim(tmp, "C", 303, 20000, ["--lr-n", "1"])
    d.sr = a + ".sr.fq"
    d.genome = {"A": rr.read_fastx(a + ".ref.fa")[0][1], "B": rr.read_fastx(b + ".ref.fa")[0][1]}
    d.truth = {}
    lr = []
    for tag, pre in (("A", a), ("B", b)):
        lr += [(tag + "_" + n, s) for n, s in rr.read_fastx(pre + ".lr.fq")]
        for line in open(pre + ".lr.truth.tsv"):
            n, _, start, length, strand = line.split()
            t = d.genome[tag][int(start):int(start) + int(length)]
            d.truth[tag + "_" + n] = _rc(t) if strand == "-" else t
    d.lr = os.path.join(tmp, "LR.fq"); _write_fastq(d.lr, lr)
    d.n_lr = len(lr)
    sr_seqs = [s for _, s in rr.read_fastx(d.sr)]
    lr_seqs = [s for _, s in lr]
    d.sets = {k: (rr.seen_twice(lr_seqs, k), rr.seen_twice(sr_seqs, k)) for k in (21, 31)}
    ub = [("B_" + n, s) for n, s in rr.read_fastx(b + ".sr.fq")]
    uc = [("C_" + n, s) for n, s in rr.read_fastx(c + ".sr.fq")]
    ua = [("A_" + n, s) for n, s in rr.read_fastx(a + ".sr.fq")[:1200]]
    # boundary reads: stretches of B with exactly T and exactly T - 1 qualifying positions, found with the restatement's sets
    special = []
    g = d.genome["B"]
    for k in (21, 31):
        lr2, sr2 = d.sets[k]
        length = k + rr.T - 1
        cands = [g[o:o + length] for o in range(500, len(g) - length, 997)]
        counts, _ = rr.qualifying_positions(cands, k, lr2, sr2)
        full = [s for s, n in zip(cands, counts) if n == rr.T]
        assert full, "no stretch of B with all of its k-mers in the long reads only"
        special += [("edge_k%d_T" % k, full[0]), ("edge_k%d_Tm1" % k, full[0][:-1])]
    special += [("short10", g[1000:1010]), ("short20", g[1000:1020]), ("short30", g[1000:1030]),
                ("lower_b", ub[3][1].lower()), ("mixed_b", ub[5][1][:70].lower() + ub[5][1][70:]), ("lower_c", uc[3][1].lower()),
                ("n_mid_b", ub[7][1][:75] + "N" + ub[7][1][76:]), ("n_every_25_b", "".join("N" if i % 25 == 24 else ch for i, ch in enumerate(ub[9][1]))), ("n_lower_b", ub[11][1][:40].lower() + "n" + ub[11][1][41:])]
    u = []
    for i in range(max(len(ub), len(uc), len(ua))):  # fixed interleaving; a special read after every 50th round
        for src in (ub, uc, ua):
            if i < len(src):
                u.append(src[i])
        if i % 50 == 49 and special:
            u.append(special.pop(0))
    u += special
    d.u_records = u
    d.u = os.path.join(tmp, "U.fq"); _write_fastq(d.u, u)
    # the conditions that keep the tests from passing vacuously, on the restatement alone
    for k in (21, 31):
        lr2, sr2 = d.sets[k]
        keep = dict(zip([n for n, _ in u], rr.keep_mask([s for _, s in u], k, lr2, sr2)))
        frac = lambda names: sum(keep[n] for n in names) / float(len(names))
        assert frac([n for n, _ in ub]) >= 0.90, (k, frac([n for n, _ in ub]))
        assert frac([n for n, _ in uc]) == 0.0
        assert frac([n for n, _ in ua]) < 0.05
        assert keep["edge_k%d_T" % k] and not keep["edge_k%d_Tm1" % k]
        assert not keep["short10"] and not keep["short20"] and keep["lower_b"] and not keep["lower_c"] and keep["n_mid_b"] and not keep["n_every_25_b"]
    d.want = {k: rr.rescue_bytes(u, k, *d.sets[k]) for k in (21, 31)}
    return d


def _tool(args, env=None, timeout=None):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_THREADS="4", **(env or {})), timeout=timeout)


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("k", [31, 21])
def test_plain_tool_writes_the_restatements_bytes(data, tmp_path, k):
    out = str(tmp_path / "o")
    r = _tool(["-s", data.sr, "-l", data.lr, "-u", data.u, "-k", str(k), "-o", out], env={"RTK_INDEX_TRACE": "1", "RTK_INDEX_CHUNK": "100000"})
    assert r.returncode == 0, r.stderr
    got = open(out + "_extra_sr.fasta", "rb").read()
    assert got == data.want[k]
    assert got.count(b">") > 2000 and b">lower_b\n" in got and b">edge_k%d_T\n" % k in got and b"edge_k%d_Tm1" % k not in got
    assert all(ln == ln.upper() for ln in got.split(b"\n") if not ln.startswith(b">"))  # lower_b, mixed_b, n_lower_b come out in upper case
    for lap in ("count LR", "count SR", "build D", "filter", "reads in"):
        assert lap in r.stderr, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["o_extra_sr.fasta"]


def test_plain_tool_gzip_bgzf_list_and_two_unmapped_files(data, tmp_path):
    tmp = str(tmp_path)
    half = len(data.u_records) // 2
    u1, u2 = os.path.join(tmp, "u1.fq"), os.path.join(tmp, "u2.fa")
    _write_fastq(u1, data.u_records[:half])
    with open(u2, "w") as f:  # the second file as FASTA with a description after the name
        for n, s in data.u_records[half:]:
            f.write(">%s some description\n%s\n" % (n, s))
    u1z = u1 + ".gz"
    with open(u1, "rb") as fi, gzip.open(u1z, "wb") as fo:
        fo.write(fi.read())
    u2b = u2 + ".bgz"
    subprocess.check_call([os.path.join(BIN, "rtk_bgzip"), u2, u2b])
    lrz = os.path.join(tmp, "LR.fq.gz")
    with open(data.lr, "rb") as fi, gzip.open(lrz, "wb") as fo:
        fo.write(fi.read())
    srb = os.path.join(tmp, "sr.bgz")
    subprocess.check_call([os.path.join(BIN, "rtk_bgzip"), data.sr, srb])
    out = os.path.join(tmp, "o")
    r = _tool(["-s", srb, "-l", lrz, "-u", u1z, "-u", u2b, "-o", out])
    assert r.returncode == 0, r.stderr
    assert open(out + "_extra_sr.fasta", "rb").read() == data.want[31]
    os.remove(out + "_extra_sr.fasta")
    lst = os.path.join(tmp, "unmapped.txt")
    open(lst, "w").write(u1 + "\n" + u2 + "\n")
    r = _tool(["-s", data.sr, "-l", data.lr, "-u", lst, "-o", out])
    assert r.returncode == 0, r.stderr
    assert open(out + "_extra_sr.fasta", "rb").read() == data.want[31]


def test_no_long_read_kmer_seen_twice_leaves_no_file(data, tmp_path):
    """Long reads at 1x -- B cut into pieces that do not overlap: no k-mer is seen twice, nothing can qualify; status 0, no file (src/Graph.cpp:3890, 4124-4128)."""
    tmp = str(tmp_path)
    g = data.genome["B"]
    tiles = [("tile%d" % i, g[o:o + 3000]) for i, o in enumerate(range(0, len(g), 3000))]
    assert len(rr.seen_twice([s for _, s in tiles], 31)) == 0
    one = os.path.join(tmp, "one.fq")
    _write_fastq(one, tiles)
    out = os.path.join(tmp, "o")
    open(out + "_extra_sr.fasta", "w").write(">stale\nACGT\n")  # a file of an earlier run does not survive
    r = _tool(["-s", data.sr, "-l", one, "-u", data.u, "-o", out])
    assert r.returncode == 0 and "0 reads kept" in r.stderr, r.stderr
    assert os.listdir(tmp) == ["one.fq"]
    # long reads that hold B, unmapped reads that are all contamination: the scan runs, keeps nothing, and no file remains
    only_c = os.path.join(tmp, "c.fq")
    _write_fastq(only_c, [(n, s) for n, s in data.u_records if n.startswith("C_")])
    r = _tool(["-s", data.sr, "-l", data.lr, "-u", only_c, "-o", out])
    assert r.returncode == 0 and "0 reads kept of 4000" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp)) == ["c.fq", "one.fq"]


def test_tool_failures_leave_no_file(data, tmp_path):
    out = str(tmp_path / "o")
    r = _tool(["-s", data.sr, "-l", data.lr, "-u", str(tmp_path / "missing.fq"), "-o", out])
    assert r.returncode != 0 and "missing.fq" in r.stderr
    bad = str(tmp_path / "cut.fq.gz")
    with gzip.open(bad, "wb") as fo:
        fo.write(open(data.u, "rb").read())
    blob = open(bad, "rb").read()
    open(bad, "wb").write(blob[:len(blob) // 2])  # a gzip stream cut short is not the end of the reads
    r = _tool(["-s", data.sr, "-l", data.lr, "-u", bad, "-o", out])
    assert r.returncode != 0, r.stderr
    assert r.returncode != 2 and _tool(["-s", data.sr, "-l", data.lr, "-u", data.u, "-k", "33", "-o", out]).returncode == 2  # one-word k-mers only
    assert os.listdir(str(tmp_path)) == ["cut.fq.gz"]


@pytest.mark.parametrize("exe", [EXE, SIM_EXE], ids=["Ratatosk", "Ratatosk_sim"])
def test_cli_unmapped_option(data, tmp_path, exe):
    tmp = str(tmp_path)
    out = os.path.join(tmp, "out")
    for mode in ([], ["-1"], ["-2", "-L", data.lr]):
        r = subprocess.run([exe, "correct"] + mode + ["-s", data.sr, "-u", os.path.join(tmp, "missing.fq"), "-l", data.lr, "-o", out], capture_output=True, text=True)
        assert r.returncode != 0, (mode, r.stderr)
        assert "rescue" in r.stderr and "step" in r.stderr, (mode, r.stderr)
        assert "k1 index" not in r.stderr  # the run ended at the rescue
        assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)
    # next to a pre-built index the rescue has no place, wherever -u stands on the command line
    for args in (["-1", "-u", "x.fq", "-g", "a", "-d", "b"], ["-1", "-g", "a", "-d", "b", "-u", "x.fq"], ["-2", "-u", "x.fq", "-u", "y.fq", "-g", "a", "-d", "b", "-L", "r"]):
        r = subprocess.run([exe, "correct"] + args + ["-l", "c", "-o", out], capture_output=True, text=True)
        assert r.returncode == 1 and "not in scope" in r.stderr and "index build" in r.stderr, (args, r.stderr)
    r = subprocess.run([exe, "correct", "-s", data.sr, "-a", "x", "-l", data.lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "not in scope" in r.stderr
    for flag in ("-p", "-P"):
        r = subprocess.run([exe, "correct", "-s", data.sr, flag, "x", "-l", data.lr, "-o", out], capture_output=True, text=True)
        assert r.returncode == 1 and "not in scope" in r.stderr
    r = subprocess.run([exe, "correct", "-u", "x.fq", "-l", data.lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "-s" in r.stderr
    assert "-u, --in-unmapped-short" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr


def test_header_and_libraries_agree_on_revision_10_and_the_rescue_and_sets_entries():
    txt = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    assert re.search(r"#define\s+RTK_API_REVISION\s+10\b", txt)
    for name in ("rtk_rescue_begin", "rtk_rescue_chunk", "rtk_rescue_end", "rtk_sets_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    for path in (LIB, SIM_LIB):
        L = ctypes.CDLL(path)
        assert L.rtk_api_revision() == 10, path
        for name in ("rtk_rescue_begin", "rtk_rescue_chunk", "rtk_rescue_end", "rtk_sets_batch"):
            assert hasattr(L, name), (path, name)


def test_no_rescue_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from ratatosk_amd import api
    with pytest.raises(api.RtkError) as e:
        api.rescue_reads([1, 2, 3], [2], ["ACGT" * 20])
    assert "no such HIP device" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _run(args, env=None):
    r = subprocess.run(args, capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.returncode, r.stderr[-4000:])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 21])
def test_gpu_tool_writes_the_plain_paths_bytes(data, tmp_path, k):
    plain, dev = str(tmp_path / "plain"), str(tmp_path / "dev")
    assert _tool(["-s", data.sr, "-l", data.lr, "-u", data.u, "-k", str(k), "-o", plain]).returncode == 0
    r = _tool(["--gpu", "-s", data.sr, "-l", data.lr, "-u", data.u, "-k", str(k), "-o", dev], env={"RTK_INDEX_TRACE": "1", "RTK_INDEX_CHUNK": "65536"}, timeout=GPU_STEP_TIMEOUT)
    assert r.returncode == 0, r.stderr
    n_chunks = int(re.search(r"characters in (\d+) chunks", r.stderr).group(1))
    assert n_chunks >= 8, r.stderr  # the -u text arrived in several chunks
    got = open(dev + "_extra_sr.fasta", "rb").read()
    assert got == open(plain + "_extra_sr.fasta", "rb").read() and got == data.want[k]
    _, probed = rr.qualifying_positions([s for _, s in data.u_records], k, *data.sets[k])
    assert "%d positions probed" % probed in r.stderr, r.stderr


_API_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r)
from ratatosk_amd import api
z = np.load(sys.argv[1])
seqs = json.load(open(sys.argv[2]))
out = {}
for k in (21, 31):
    st = {}
    mask = api.rescue_reads(z["lr%%d" %% k], z["sr%%d" %% k], seqs, k=k, min_positions=31, stats=st)
    out[str(k)] = {"mask": [int(x) for x in mask], "probed": st["n_positions_probed"], "hits": st["n_hits"]}
st = {}
out["t1"] = {"mask": [int(x) for x in api.rescue_reads(z["lr31"], z["sr31"], seqs, k=31, min_positions=1, stats=st)], "hits": st["n_hits"]}
out["empty"] = [int(x) for x in api.rescue_reads([], z["sr31"], seqs[:50], k=31)]
try:
    api.rescue_reads(z["lr31"], z["sr31"], seqs[:5], k=33)
    out["k33"] = "accepted"
except api.RtkError as e:
    out["k33"] = str(e)
json.dump(out, open(sys.argv[3], "w"))
"""


@pytest.mark.gpu
def test_gpu_entries_through_the_python_layer(data, tmp_path):
    """rtk_rescue_begin / _chunk / _end through api.rescue_reads, in a child process: keep mask and hit count against the restatement."""
    tmp = str(tmp_path)
    seqs = [s for _, s in data.u_records]
    np.savez(os.path.join(tmp, "sets.npz"), lr21=data.sets[21][0], sr21=data.sets[21][1], lr31=data.sets[31][0], sr31=data.sets[31][1])
    json.dump(seqs, open(os.path.join(tmp, "seqs.json"), "w"))
    open(os.path.join(tmp, "child.py"), "w").write(_API_CHILD % ROOT)
    _run([sys.executable, os.path.join(tmp, "child.py"), os.path.join(tmp, "sets.npz"), os.path.join(tmp, "seqs.json"), os.path.join(tmp, "out.json")])
    got = json.load(open(os.path.join(tmp, "out.json")))
    for k in (21, 31):
        counts, probed = rr.qualifying_positions(seqs, k, *data.sets[k])
        assert got[str(k)]["mask"] == [int(x) for x in rr.keep_mask(seqs, k, *data.sets[k])]
        assert got[str(k)]["hits"] == int(counts.sum()) and got[str(k)]["probed"] == probed
        assert sum(got[str(k)]["mask"]) > 2000
    counts, _ = rr.qualifying_positions(seqs, 31, *data.sets[31])
    assert got["t1"]["mask"] == [int(len(s) >= 31 and c >= 1) for s, c in zip(seqs, counts)] and got["t1"]["hits"] == int(counts.sum())
    assert got["empty"] == [0] * 50
    assert "k <= 31" in got["k33"]


def _edit_distance(a, b):
    from oracle import oracle_py as op
    return op.myers(a, b, -1, 0)[0]


@pytest.fixture(scope="module")
def runs(data):
    """The correction runs of the GPU tests, each a chain of child processes: with -u, by hand (the tool's file as a second -s), and without -u."""
    tmp = data.tmp
    r = Data()
    hand = os.path.join(tmp, "hand"); os.mkdir(hand)
    _run([TOOL, "--gpu", "-s", data.sr, "-l", data.lr, "-u", data.u, "-o", os.path.join(hand, "x")])
    r.extra = os.path.join(hand, "x_extra_sr.fasta")
    assert open(r.extra, "rb").read() == data.want[31]
    _run([EXE, "correct", "-c", "2", "-s", data.sr, "-s", r.extra, "-l", data.lr, "-o", os.path.join(hand, "out")])
    r.hand = os.path.join(hand, "out.fastq")
    _run([EXE, "correct", "-1", "-c", "2", "-s", data.sr, "-s", r.extra, "-l", data.lr, "-o", os.path.join(hand, "p1")])
    r.hand1 = os.path.join(hand, "p1.2.fastq")
    r.with_u = os.path.join(tmp, "with_u"); os.mkdir(r.with_u)
    r.with_u_log = _run([EXE, "correct", "-v", "-c", "2", "-s", data.sr, "-u", data.u, "-l", data.lr, "-o", os.path.join(r.with_u, "out")]).stderr
    r.with_u1 = os.path.join(tmp, "with_u1"); os.mkdir(r.with_u1)
    _run([EXE, "correct", "-1", "-c", "2", "-s", data.sr, "-u", data.u, "-l", data.lr, "-o", os.path.join(r.with_u1, "out")])
    r.without = os.path.join(tmp, "without"); os.mkdir(r.without)
    _run([EXE, "correct", "-c", "2", "-s", data.sr, "-l", data.lr, "-o", os.path.join(r.without, "out")])
    return r


@pytest.mark.gpu
def test_gpu_correct_with_unmapped_reads_equals_the_steps_by_hand(data, runs):
    assert open(os.path.join(runs.with_u, "out.fastq"), "rb").read() == open(runs.hand, "rb").read()
    assert sorted(os.listdir(runs.with_u)) == ["out.fastq"], os.listdir(runs.with_u)  # the rescued reads, the indexes and OUT.2.fastq are removed
    for msg in ("Creating index of short reads", "Creating index of long reads", "Querying full short read set for missing reads", "Added "):
        assert "Ratatosk::retrieveMissingReads(): " + msg in runs.with_u_log, runs.with_u_log
    assert "Added %d short reads to dataset." % data.want[31].count(b">") in runs.with_u_log
    assert open(os.path.join(runs.with_u1, "out.2.fastq"), "rb").read() == open(runs.hand1, "rb").read()
    assert sorted(os.listdir(runs.with_u1)) == ["out.2.fastq"], os.listdir(runs.with_u1)


@pytest.mark.gpu
def test_gpu_rescued_reads_correct_the_novel_sequence(data, runs):
    """The point of the feature: the long reads of B, whose sequence the -s reads do not hold, are closer to the truth with -u than without it. The reads of A may change
    where B shares k-mers with A (both graphs gain B's k-mers), so their number is printed, not asserted."""
    with_u = dict(rr.read_fastx(os.path.join(runs.with_u, "out.fastq")))
    without = dict(rr.read_fastx(os.path.join(runs.without, "out.fastq")))
    assert len(with_u) == len(without) == data.n_lr
    b_names = sorted(n for n in with_u if n.startswith("B_"))
    assert len(b_names) >= 200
    mean = lambda reads: sum(_edit_distance(reads[n], data.truth[n]) for n in b_names) / float(len(b_names))
    m_with, m_without = mean(with_u), mean(without)
    a_names = [n for n in with_u if n.startswith("A_")]
    a_changed = sum(with_u[n] != without[n] for n in a_names)
    print("mean edit distance of B's long reads to the truth: %.2f with -u, %.2f without; %d of %d reads of A differ between the two runs" % (m_with, m_without, a_changed, len(a_names)))
    assert m_with < m_without
