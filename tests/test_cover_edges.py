"""`rtk_build_index --cover-edges-from FILE` and `Ratatosk correct -s ... --k1-from-k2 --cover-edges` (DESIGN.md section 4 [A16]): the edges of the graph whose
two unitigs share fewer than min_cov_vertices colours get two fresh colour ids on both ends wherever a sequence of FILE (the unitigs of the k2 graph) walks
over them -- the last block of the reference's first-pass addCoverage (src/Graph.cpp:3085-3363). The tool is held to tests/cover_edges_restatement.py, a
literal restatement of the reference's two loops that works from the bytes of the index built WITHOUT the option; the annotations of the covered index to
oracle/oracle_annot.py on the covered colours; the device search (rtk_index_cover_*, csrc/hip/rtk_index_cover.h) to the restatement's crossings.
Non-vacuity is asserted on the restatement's own count of covered edges, never on the tool's.
The simulated sets are 30 kb diploid at 30x; one case takes another and says why: at k = 63 a 30x set has an estimated haplotype coverage of
7, below the 10 from which --subsample-colours thins anything (`subsample: hap_cov=7 off`), so the k = 63 subsampling case takes the same set at 60x."""
import gzip
import os
import random
import re
import subprocess
import sys

import pytest

from conftest import BIN, ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cover_edges_restatement as R  # noqa: E402
from oracle import oracle_annot  # noqa: E402

TOOL = os.path.join(BIN, "rtk_build_index")
EXE = os.path.join(BIN, "Ratatosk")
MODES = {"plain": [], "fast": ["--fast"]}
SET = ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-err", "0.002", "--lr-n", "6", "--lr-len", "1500"]
SMALL_JOB = {"RTK_INDEX_EVENTS": "4000000"}  # room for 4 M colour events instead of 60 % of the device memory: opening the colouring job then takes no seconds
GPU_TIMEOUT = 120
COUNTS = re.compile(r"rtk_build_index: cover: edges_recorded=(\d+) edges_covered=(\d+) ids_added=(\d+)")


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


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


def _write_fasta(path, seqs, width=None):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">%d\n" % i)
            if width:
                f.write("\n".join(s[j:j + width] for j in range(0, len(s), width)) + "\n")
            else:
                f.write(s + "\n")
    return path


def _counts(stderr):
    m = COUNTS.search(stderr)
    assert m, stderr
    return tuple(int(x) for x in m.groups())


def _check_against_restatement(base, covered, k, cover_files, stderr):
    """the covered index == the uncovered one + the restatement's ids; -> the restatement's result"""
    want = R.restate(_fasta(base, k), _rtsk(base, k), k, cover_files)
    assert open(_fasta(base, k), "rb").read() == open(_fasta(covered, k), "rb").read()
    a, b = R.parse_rtsk(_rtsk(base, k)), R.parse_rtsk(_rtsk(covered, k))
    assert len(a) == len(b)
    for u, (x, y) in enumerate(zip(a, b)):
        assert y["local"] == x["local"] + want["added"][u], "local set of unitig %d" % u
        assert y["glob"] == x["glob"] and y["kmcov"] == x["kmcov"] and y["head"] == x["head"], "unitig %d" % u
        assert (y["shared"] & 0xFF) == (x["shared"] & 0xFF), "edge bits of unitig %d" % u
    assert _counts(stderr) == (want["recorded"], want["covered"], want["ids_added"])
    return want


def _build_pair(tmp, tag, sr, k, cover_files, extra, mode, env=None, timeout=None):
    """the index without and with the option -> (base prefix, covered prefix, stderr of the covered build)"""
    base, cov = os.path.join(tmp, tag + "_base"), os.path.join(tmp, tag + "_cov")
    _ok(["-s", sr, "-k", str(k), "-o", base] + extra + mode, env, timeout)
    args = []
    for f in cover_files:
        args += ["--cover-edges-from", f]
    r = _ok(["-s", sr, "-k", str(k), "-o", cov] + extra + mode + args, env, timeout)
    assert "low-coverage edges covered" in r.stderr
    return base, cov, r.stderr


# ---------------------------------------------------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the simulated set at 30x and at 60x: short reads, the haplotype FASTA, the unitig FASTA of the k2 graph"""
    tmp = str(tmp_path_factory.mktemp("cover_sets"))
    out = {}
    for cov in (30, 60):
        pre = os.path.join(tmp, "c%d" % cov)
        subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--sr-cov", str(cov)] + SET, stderr=subprocess.DEVNULL)
        _ok(["-s", pre + ".sr.fq", "-k", "63", "-o", pre + "_g", "--graph-only"])
        out[cov] = {"sr": pre + ".sr.fq", "hap": pre + ".ref.fa", "k2": _fasta(pre + "_g", 63)}
    return out


def _bubble(tmp):
    """A SNP bubble whose second allele is seen by one read pair alone, the mates overlapping over it: every k-mer of the allele is seen twice (the default
    --min-count keeps it, at k = 31 and k = 63) and carries ONE colour, so both junction edges of the allele's unitig share 1 < 2 colours. -> reads, hapA, hapB"""
    rnd = random.Random(7)
    hap_a = "".join(rnd.choice("ACGT") for _ in range(700))
    alt = {"A": "C", "C": "G", "G": "T", "T": "A"}[hap_a[350]]
    hap_b = hap_a[:350] + alt + hap_a[351:]
    sr = os.path.join(tmp, "bubble.sr.fq")
    with open(sr, "w") as f:
        n = 0
        for rep in range(3):
            for start in range(0, len(hap_a) - 100 + 1, 4):
                f.write("@a%d\n%s\n+\n%s\n" % (n, hap_a[start:start + 100], "I" * 100)); n += 1
        f.write("@p/1\n%s\n+\n%s\n" % (hap_b[265:415], "I" * 150))
        f.write("@p/2\n%s\n+\n%s\n" % (_rc(hap_b[285:435]), "I" * 150))
    return sr, hap_a, hap_b


def _self_meeting_reads(tmp):
    """The genomes of tests/test_graph_reuse.py _self_meeting_genomes -- a circular 600 bp sequence and W + reverse complement of W (hairpin) --, with ONE name per
    genome: each unitig then carries one colour, so the edge on which it meets itself shares 1 < 2 colours and is recorded. -> reads, circle, hairpin"""
    rnd = random.Random(5)
    circ = "".join(rnd.choice("ACGT") for _ in range(600))
    w = "".join(rnd.choice("ACGT") for _ in range(300))
    hair = w + _rc(w)
    sr = os.path.join(tmp, "self.sr.fq")
    with open(sr, "w") as f:
        for rep in range(3):
            for start in range(0, 600, 7):
                f.write("@c\n%s\n+\n%s\n" % ((circ + circ)[start:start + 100], "I" * 100))
        for rep in range(3):
            for start in range(0, len(hair) - 100 + 1, 5):
                f.write("@h\n%s\n+\n%s\n" % (hair[start:start + 100], "I" * 100))
    return sr, circ, hair


# ---------------------------------------------------------------------------------------------------------------- CPU tier: the tool == the restatement
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("k", [31, 63])
def test_crafted_bubble_seen_by_one_pair(tmp_path, mode, k):
    tmp = str(tmp_path)
    sr, hap_a, hap_b = _bubble(tmp)
    g = os.path.join(tmp, "g")
    _ok(["-s", sr, "-k", "63", "-o", g, "--graph-only"])  # (default --min-count for both graphs)
    cover = [_fasta(g, 63)] if k == 31 else [_write_fasta(os.path.join(tmp, "haps.fa"), [hap_a, hap_b])]
    base, cov, err = _build_pair(tmp, "bubble", sr, k, cover, ["--snps"], MODES[mode])
    want = _check_against_restatement(base, cov, k, cover, err)
    assert want["covered"] >= 1, want  # non-vacuity, on the restatement's count


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("k,cov,extra", [(31, 30, "--subsample-colours"), (63, 60, "--subsample-colours"), (31, 30, "--merge-duplicates"), (63, 30, "--merge-duplicates")],
                         ids=["k31-subsampled", "k63-subsampled-60x", "k31-merged", "k63-merged"])
def test_simulated_set_thinned_or_merged(tmp_path, sets, mode, k, cov, extra):
    s = sets[cov]
    cover = [s["k2"]] if k == 31 else [s["hap"]]  # (k = 63: the haplotype FASTA of the simulated set)
    base, covd, err = _build_pair(str(tmp_path), "sim", s["sr"], k, cover, ["--snps", extra], MODES[mode])
    want = _check_against_restatement(base, covd, k, cover, err)
    assert want["covered"] >= 1, want
    if extra == "--subsample-colours":
        assert "subsample: hap_cov=" in err and " off" not in [l for l in err.split("\n") if "subsample: hap_cov=" in l][0], err  # the thinning ran


def test_order_and_double_cover(tmp_path):
    tmp = str(tmp_path)
    sr, hap_a, hap_b = _bubble(tmp)
    k = 31
    left, right = hap_b[300:360], hap_b[340:400]  # windows 300 .. 329 cross onto the allele's unitig (its first 31-mer starts at 320); 340 .. 369 cross off it (its last starts at 350)
    later = hap_b[305:365]                       # the first edge again, the same way
    res = {}
    for tag, seqs in (("same", [left, later]), ("opposite", [left, _rc(left)]), ("two", [left, right]), ("swapped", [right, left])):
        f = _write_fasta(os.path.join(tmp, tag + ".fa"), seqs)
        base, cov, err = _build_pair(tmp, tag, sr, k, [f], [], [])
        res[tag] = _check_against_restatement(base, cov, k, [f], err)
    assert (res["same"]["covered"], res["same"]["ids_added"]) == (1, 2)          # the second sequence finds the bit cleared
    assert [c[:2] for c in res["same"]["crossings"]] == [(0, 19), (1, 14)]      # ... though it crosses the edge as well
    assert (res["opposite"]["covered"], res["opposite"]["ids_added"]) == (2, 4)  # the other direction is another bit, on the other unitig
    assert res["two"]["covered"] == 2 and res["swapped"]["covered"] == 2
    two, swp = res["two"]["added"], res["swapped"]["added"]
    ends = [u for u in range(len(two)) if len(two[u]) == 2]
    assert len(ends) == 2 and two[ends[0]] == swp[ends[1]] and two[ends[1]] == swp[ends[0]] and two[ends[0]] != two[ends[1]]  # the ids follow the order of the file


@pytest.mark.parametrize("mode", sorted(MODES))
def test_unitigs_that_meet_themselves(tmp_path, mode):
    tmp = str(tmp_path)
    sr, circ, hair = _self_meeting_reads(tmp)
    f = _write_fasta(os.path.join(tmp, "walks.fa"), [circ + circ + circ[:50], hair])
    base, cov, err = _build_pair(tmp, "self", sr, 31, [f], [], MODES[mode])
    want = _check_against_restatement(base, cov, 31, [f], err)
    onto_itself = [c for c in want["crossings"] if c[2] == c[3]]
    assert {c[0] for c in onto_itself} == {0, 1}, want["crossings"]  # the loop closes onto itself, the hairpin turns onto its own other strand
    assert want["covered"] >= 2


@pytest.mark.parametrize("mode", sorted(MODES))
def test_foreign_file(tmp_path, sets, mode):
    tmp = str(tmp_path)
    s = sets[30]
    unitigs = R.read_fasta(s["k2"])
    rnd = random.Random(3)
    long_ones = sorted(unitigs, key=len, reverse=True)[:40]
    seqs = []
    for i, u in enumerate(long_ones + [x for x in unitigs if len(x) < 200][:200]):
        if i % 4 == 0:
            u = u[:len(u) // 2] + "N" + u[len(u) // 2 + 1:]
        elif i % 4 == 1:
            u = u.lower()
        elif i % 4 == 2:  # a k-mer that is not in the graph
            j = len(u) // 3
            u = u[:j] + {"A": "C", "C": "G", "G": "T", "T": "A"}[u[j]] + u[j + 1:]
        seqs.append(u)
    seqs += ["ACGTACGTAC", "".join(rnd.choice("ACGT") for _ in range(31)), ""]  # shorter than k + 1
    f = _write_fasta(os.path.join(tmp, "foreign.fa"), seqs, width=70)
    gz = os.path.join(tmp, "foreign.fa.gz")
    with gzip.open(gz, "wb") as out:
        out.write(open(f, "rb").read())
    base, cov, err = _build_pair(tmp, "foreign", s["sr"], 31, [f], ["--merge-duplicates"], MODES[mode])
    want = _check_against_restatement(base, cov, 31, [f], err)
    assert want["covered"] >= 1
    _ok(["-s", s["sr"], "-k", "31", "-o", os.path.join(tmp, "gz"), "--merge-duplicates", "--cover-edges-from", gz] + MODES[mode])
    assert _files(os.path.join(tmp, "gz"), 31) == _files(cov, 31)
    # a file of no use: covers nothing, says so, no error
    useless = _write_fasta(os.path.join(tmp, "useless.fa"), ["ACGTNNACGT", "acgt"])
    r = _ok(["-s", s["sr"], "-k", "31", "-o", os.path.join(tmp, "none"), "--merge-duplicates", "--cover-edges-from", useless] + MODES[mode])
    assert "no sequence of 31 characters" in r.stderr and "nothing covered" in r.stderr, r.stderr
    assert _counts(r.stderr)[1:] == (0, 0)
    assert _files(os.path.join(tmp, "none"), 31) == _files(base, 31)


def test_without_the_option_nothing_changes(tmp_path, sets):
    tmp = str(tmp_path)
    empty = os.path.join(tmp, "empty.fa")
    open(empty, "w").close()
    for extra in ([], ["--snps", "--subsample-colours"]):
        base, cov, err = _build_pair(tmp, "e%d" % len(extra), sets[30]["sr"], 31, [empty], extra, [])
        assert _files(base, 31) == _files(cov, 31)
        assert "nothing covered" in err


def test_the_annotators_see_the_ids(tmp_path, sets):
    """Covering changes shared_count along SNP bubbles and short cycles: the annotations of the covered index are those of oracle_annot on the covered colours
    (the edge bits are the index's own: they are not recomputed)."""
    tmp = str(tmp_path)
    s = sets[30]
    k = 31
    base, cov, err = _build_pair(tmp, "annot", s["sr"], k, [s["k2"]], ["--snps", "--merge-duplicates"], [])
    seqs = R.read_fasta(_fasta(cov, k))
    a, b = R.parse_rtsk(_rtsk(base, k)), R.parse_rtsk(_rtsk(cov, k))
    assert sum(x["amb"] != y["amb"] or x["cycles"] != y["cycles"] for x, y in zip(a, b)) >= 1, "covering changed no annotation: the input shows nothing"
    ag = oracle_annot.AnnotGraph(seqs, [sorted(set(r["glob"]) | set(r["local"])) for r in b], k)
    bits = [r["shared"] & 0xFF for r in b]
    n_amb = 0
    for u, r in enumerate(b):
        cycles = [c.decode() for c in r["cycles"].split(b"\0")[:-1]]
        assert ag.short_cycles(u, bits) == cycles, "short cycles of unitig %d" % u
        assert ag.snp_annotations(u, bits) == [(v >> 4, ".ACMGRSVTWYHKDBN"[v & 15]) for v in r["amb"]], "SNP annotations of unitig %d" % u  # (position << 4 | base bits, UnitigData.hpp:448-451)
        n_amb += len(r["amb"])
    assert n_amb > 0


def test_refusals(tmp_path, sets):
    tmp = str(tmp_path)
    s = sets[30]
    out = os.path.join(tmp, "o")
    r = _tool(["-s", s["sr"], "-o", out, "--colour-reads", s["sr"], "--cover-edges-from", s["k2"]])
    assert r.returncode == 2 and "--cover-edges-from next to --colour-reads" in r.stderr, r.stderr
    r = _tool(["-s", s["sr"], "-o", out, "--graph-only", "--cover-edges-from", s["k2"]])
    assert r.returncode == 2 and "--graph-only" in r.stderr and "--cover-edges-from does not go with it" in r.stderr, r.stderr
    r = _tool(["-s", s["sr"], "-o", out, "--cover-edges-from", os.path.join(tmp, "missing.fa.gz")])
    assert r.returncode == 2 and "--cover-edges-from: cannot open" in r.stderr and "missing.fa.gz" in r.stderr, r.stderr
    assert not os.listdir(tmp)
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([EXE, "correct", "-s", s["sr"], "-l", lr, "-o", out, "--cover-edges"], capture_output=True, text=True)
    assert r.returncode != 0 and "--cover-edges needs --k1-from-k2" in r.stderr, r.stderr
    r = subprocess.run([EXE, "correct", "-1", "-g", s["k2"], "-d", s["k2"], "-l", lr, "-o", out, "--k1-from-k2", "--cover-edges"], capture_output=True, text=True)
    assert r.returncode != 0 and "--cover-edges belongs to the index build" in r.stderr and "(-g, -d)" in r.stderr, r.stderr
    # the driver hands the k2 unitig file to the k1 index step (which fails here on the missing reads, after it was named)
    r = subprocess.run([EXE, "correct", "-v", "-1", "-s", os.path.join(tmp, "missing.fq"), "-l", lr, "-o", out, "--k1-from-k2", "--cover-edges"], capture_output=True, text=True)
    assert r.returncode != 0 and "step 1a" in r.stderr, r.stderr
    usage = subprocess.run([EXE, "--help"], capture_output=True, text=True).stderr + _tool([]).stderr
    assert "--cover-edges " in usage and "--cover-edges-from" in usage


def test_entries_are_declared_and_refuse_a_device_that_is_not_there():
    import ctypes as C
    from ratatosk_amd import api
    txt = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    for name in ("rtk_index_cover_begin", "rtk_index_cover_chunk", "rtk_index_cover_end"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    L = api.load_library()
    job, off, low = C.c_void_p(), (C.c_uint64 * 2)(0, 40), (C.c_ubyte * 1)(0)
    assert L.rtk_index_cover_begin(99, 31, b"A" * 40, off, 1, low, C.byref(job)) == -4 and not job.value  # RTK_ERR_NO_DEVICE
    assert b"no such HIP device" in L.rtk_last_error()
    assert L.rtk_index_cover_begin(99, 31, b"A" * 40, off, (1 << 30) + 1, low, C.byref(job)) == -6  # RTK_ERR_UNSUPPORTED: a crossing has 30 bits for a unitig
    assert L.rtk_index_cover_chunk(None, b"A", 1, off, None, off, 1) != 0 and L.rtk_index_cover_end(None, None, None) != 0  # no job: an argument error, nothing touched
    with pytest.raises(ValueError):
        api.index_cover_crossings(["A" * 40], 31, [0, 0], [])


def test_layout_of_the_chunks():
    """What api.index_cover_crossings hands to the device: a sequence below k + 1 characters is left out, the numbers of the others stay; a sequence longer than a
    chunk is cut so that every k + 1 consecutive characters lie whole inside exactly one piece."""
    from ratatosk_amd import api
    k = 31
    rnd = random.Random(1)
    seqs = ["".join(rnd.choice("ACGT") for _ in range(n)) for n in (31, 32, 0, 300, 33)]
    (chars, starts, numbers, first), = api.index_cover_layout(seqs, k)
    assert numbers.tolist() == [1, 3, 4] and first.tolist() == [0, 0, 0] and starts.tolist() == [0, 33, 334]
    assert chars == b"".join(seqs[n].encode() + b"\n" for n in (1, 3, 4))
    chunk = 100
    layout = api.index_cover_layout(seqs, k, chunks=chunk)
    seen = {}
    for chars, starts, numbers, first in layout:
        assert len(chars) <= chunk and starts[0] == 0 and len(starts) == len(numbers) == len(first)
        ends = starts.tolist()[1:] + [len(chars)]
        for s, e, n, a in zip(starts.tolist(), ends, numbers.tolist(), first.tolist()):
            assert chars[e - 1:e] == b"\n" and chars[s:e - 1].decode() == seqs[n][a:a + e - 1 - s]
            for p in range(a, a + e - 1 - s - k):  # the pairs of windows (p, p + 1) whole inside this piece
                assert (n, p) not in seen
                seen[(n, p)] = 1
    assert sorted(seen) == [(n, p) for n in (1, 3, 4) for p in range(len(seqs[n]) - k)]
    assert sum(1 for _, _, numbers, _ in layout for n in numbers.tolist() if n == 3) >= 3
    with pytest.raises(ValueError):
        api.index_cover_layout(seqs, k, chunks=k + 2)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _crossing_case(tmp, sr, k, cover_seqs, extra):
    """an index without the option and the restatement's crossings of cover_seqs on it, with the recorded bits as the restatement records them"""
    base = os.path.join(tmp, "b%d" % k)
    _ok(["-s", sr, "-k", str(k), "-o", base] + extra)
    f = _write_fasta(os.path.join(tmp, "c%d.fa" % k), cover_seqs)
    want = R.restate(_fasta(base, k), _rtsk(base, k), k, [f])
    return R.read_fasta(_fasta(base, k)), want["low"], want


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_gpu_crossings_equal_the_restatement(tmp_path, sets, k, monkeypatch):
    from ratatosk_amd import api
    tmp = str(tmp_path)
    s = sets[30]
    source = R.read_fasta(s["k2"] if k == 31 else s["hap"])
    unitigs, low, want = _crossing_case(tmp, s["sr"], k, source, ["--merge-duplicates"])
    assert len(want["crossings"]) >= 3
    assert api.index_cover_crossings(unitigs, k, low, source) == want["crossings"]
    # every crossing once on lane 63, once on lane 0 of the next wave, once on the last position of a chunk that has one: a text cut out around it and placed by hand
    texts = {n: t.upper() for n, t in enumerate(source)}
    placed, expect = [], []
    for n, p, u, v, d, b in want["crossings"][:6]:
        t = texts[n]
        lo = max(0, p - 40)
        piece = t[lo:p + k + 1]  # ends with the pair of windows (p, p + 1): the crossing is its last position
        placed.append(piece); expect.append((len(placed) - 1, p - lo, u, v, d, b))
    # one chunk; in front of piece i goes a padding sequence without a k-mer, k + 1 characters at the least (a shorter one holds no pair of windows and never reaches
    # the device), of the length that moves the crossing onto lane 63 (even i) or lane 0 (odd i): block sizes are multiples of 64 and lane = character index % 64
    seqs, exp2, at = [], [], 0
    for i, piece in enumerate(placed):
        lane = 63 if i % 2 == 0 else 0
        pad = (lane - (at + 1 + expect[i][1])) % 64 + 64  # the padding and its separator go in front
        assert pad >= k + 1
        seqs.append("N" * pad); at += pad + 1
        seqs.append(piece); exp2.append((len(seqs) - 1,) + expect[i][1:])
        at += len(piece) + 1
    # ... checked on the layout the device receives, not on the sums above
    layout = api.index_cover_layout(seqs, k)
    assert len(layout) == 1
    chars, starts, numbers, first = layout[0]
    assert len(numbers) == len(seqs) and numbers.tolist() == list(range(len(seqs))) and not first.any()
    lanes = []
    for n, p in (e[:2] for e in exp2):
        i = int(starts[n]) + p
        assert chars[i:i + k + 1].decode() == seqs[n][p:p + k + 1] and chars[i + k + 1:i + k + 2] == b"\n"  # the pair of windows of the crossing, the last of its piece
        lanes.append(i % 64)
    assert lanes == [63, 0] * (len(exp2) // 2) + [63] * (len(exp2) % 2) and len(exp2) >= 3, lanes  # lane 63, lane 0 of the next wave, ...
    assert int(starts[exp2[-1][0]]) + exp2[-1][1] + k + 2 == len(chars)  # the last crossing is the last position of the chunk that has a pair of windows
    got = api.index_cover_crossings(unitigs, k, low, seqs)
    assert [g for g in got if g in exp2] == exp2 and len(got) >= len(exp2)
    again = R.restate(os.path.join(tmp, "b%d" % k) + ".index.k%d.fasta.gz" % k, os.path.join(tmp, "b%d" % k) + ".index.k%d.rtsk" % k, k, [_write_fasta(os.path.join(tmp, "placed.fa"), seqs)])
    assert got == again["crossings"]
    # small chunks: a long sequence cut into three pieces and more with the k-character overlap; the capacity of 1 sends every chunk with a second crossing round again
    longest = max(source, key=len)
    chunk = max(k + 3, len(longest) // 3 + k)
    assert (len(longest) - k) // (chunk - 1 - k) + 1 >= 3
    monkeypatch.setenv("RTK_INDEX_COVER_CAP", "1")
    assert api.index_cover_crossings(unitigs, k, low, source, chunks=chunk) == want["crossings"]
    monkeypatch.delenv("RTK_INDEX_COVER_CAP")
    # a piece that ends right after a crossing: the crossing is the last position of its chunk
    n, p = want["crossings"][0][:2]
    cut = texts[n][:p + k + 1]
    (chars, starts, numbers, first), = api.index_cover_layout([cut], k, chunks=len(cut) + 1)
    assert len(numbers) == 1 and p + k + 2 == len(chars)
    assert api.index_cover_crossings(unitigs, k, low, [cut], chunks=len(cut) + 1) == [c for c in R.restate(_fasta(os.path.join(tmp, "b%d" % k), k), _rtsk(os.path.join(tmp, "b%d" % k), k), k, [_write_fasta(os.path.join(tmp, "cut.fa"), [cut])])["crossings"]]
    # no recorded bit: no survivor; one sequence of exactly k + 1 characters
    assert api.index_cover_crossings(unitigs, k, [0] * len(unitigs), source) == []
    one = texts[n][p:p + k + 1]
    assert api.index_cover_crossings(unitigs, k, low, [one]) == [(0, 0) + want["crossings"][0][2:]]


@pytest.mark.gpu
def test_gpu_crossing_of_a_unitig_onto_itself(tmp_path):
    from ratatosk_amd import api
    tmp = str(tmp_path)
    sr, circ, hair = _self_meeting_reads(tmp)
    for k in (31, 63):
        unitigs, low, want = _crossing_case(tmp, sr, k, [circ + circ + circ[:80], hair], [])
        assert any(c[2] == c[3] for c in want["crossings"])
        assert api.index_cover_crossings(unitigs, k, low, [circ + circ + circ[:80], hair]) == want["crossings"]
        assert api.index_cover_crossings(unitigs, k, low, [circ + circ + circ[:80], hair], chunks=200) == want["crossings"]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,env", [([], {}), (["--snps", "--subsample-colours", "--merge-duplicates"], {}), (["--snps", "--subsample-colours", "--merge-duplicates"], {"RTK_INDEX_CHUNK": "4096"})],
                         ids=["bare", "snps-subsampled-merged", "chunk4096"])
def test_gpu_tool_writes_the_plain_bytes(tmp_path, sets, extra, env):
    tmp = str(tmp_path)
    s = sets[30]
    for k, cover in ((31, s["k2"]), (63, s["hap"])):
        plain, dev = os.path.join(tmp, "plain%d" % k), os.path.join(tmp, "dev%d" % k)
        r0 = _ok(["-s", s["sr"], "-k", str(k), "-o", plain, "--cover-edges-from", cover] + extra)
        r = _ok(["--gpu", "-s", s["sr"], "-k", str(k), "-o", dev, "--cover-edges-from", cover] + extra, env=dict(SMALL_JOB, **env), timeout=GPU_TIMEOUT)
        assert "rtk_index_cover:" in r.stderr and "on the host threads" not in r.stderr, r.stderr  # the device stage ran
        assert _counts(r.stderr) == _counts(r0.stderr)
        assert _files(dev, k) == _files(plain, k), k
        if env:
            assert int(re.search(r"rtk_index_cover: \d+ characters in (\d+) chunks", r.stderr).group(1)) >= 3, r.stderr
    if extra:
        assert _counts(r0.stderr)[1] >= 1


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=GPU_TIMEOUT, env=dict(os.environ, **SMALL_JOB, **(env or {})))
    assert r.returncode == 0, (cmd, r.stderr)
    return r


@pytest.mark.gpu
def test_gpu_one_command_with_cover_edges_equals_the_steps_by_hand(tmp_path, sets):
    tmp = str(tmp_path)
    s = sets[30]
    sr, lr = s["sr"], s["sr"][:-len(".sr.fq")] + ".lr.fq"
    hand = os.path.join(tmp, "hand")
    _run([TOOL, "--gpu", "--graph-only", "-k", "63", "-s", sr, "-o", hand + "_g"])
    graph = hand + "_g.index.k63.fasta.gz"
    r1 = _run([TOOL, "--gpu", "--graph-from", graph, "--cover-edges-from", graph, "-k", "31", "-s", sr, "--snps", "--merge-duplicates", "-o", hand + "_i1"], env={"RTK_INDEX_TRACE": "1"})
    assert _counts(r1.stderr)[1] >= 1
    _run([EXE, "correct", "-1", "-c", "2", "-g", hand + "_i1.index.k31.fasta.gz", "-d", hand + "_i1.index.k31.rtsk", "-l", lr, "-o", hand])
    _run([TOOL, "--gpu", "--graph-from", graph, "-k", "63", "--colour-reads", hand + ".2.fastq", "--snps", "--merge-duplicates", "-o", hand + "_i2"])
    _run([EXE, "correct", "-2", "-c", "2", "-g", hand + "_i2.index.k63.fasta.gz", "-d", hand + "_i2.index.k63.rtsk", "-l", hand + ".2.fastq", "-L", lr, "-o", hand])
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = _run([EXE, "correct", "-v", "-c", "2", "-s", sr, "-l", lr, "-o", out, "--k1-from-k2", "--cover-edges", "--merge-duplicates"])
    step1 = [l for l in r.stderr.split("\n") if l.startswith("Ratatosk::correct: step 1 ")][0]
    step3 = [l for l in r.stderr.split("\n") if l.startswith("Ratatosk::correct: step 3")][0]
    assert "--cover-edges-from " + out + ".tmp.g2.index.k63.fasta.gz" in step1 and "--cover-edges-from" not in step3, r.stderr
    assert open(out + ".fastq", "rb").read() == open(hand + ".fastq", "rb").read()
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)
