"""Index build, lookup, seeds, both correction passes and the one-command run on low-complexity, self-similar genomes (tests/hard_genomes.py):
homopolymer runs longer than k (a k-mer that is its own successor), microsatellites of unit 2..6 (cycles of 2..6 k-mers, half-k-mers with very long
lists), inverted repeats with and without a spacer (a unitig that ends in a (k-1)-mer that is its own reverse complement), a family of seven diverged
copies, heterozygous insertions and deletions, and stretches without short-read coverage of up to 3 kb. rtk_simulate writes none of these, so no other
test puts them through the device programs. The checks are the existing ones (byte equality with the oracle, with the plain index tool, with
oracle/oracle_index.py), reused from their modules; what is new is the input, and the conditions below that keep a set from passing on nothing:
every set is checked to hold the graph features its kind is there for, every long read must be changed by the correction, and the lane kernel must
keep at least half of its class (short-cycle unitigs are handed to the wave kernel by design, so the 0.9 of tests/test_lanes_regions.py does not
fit; 0.5 is the lowest floor that module uses). Host simulator here, MI355X in the gpu tier, same cases."""
import gzip
import hashlib
import os
import re
import subprocess
import threading

import pytest

import hard_genomes as hg
import test_fixsnps as FS
import test_graph_load as GL
import test_index_build as IB
import test_index_two_word as TW
import test_lanes_regions as LR
import test_pass2 as P2
import test_sim_correct as SC
import test_sim_seeds as SS
from conftest import BIN, SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

GPU_LIB = None
LANE_FLOOR = 0.5

SPECS = {
    "homopolymer": dict(seed=101, kind="homopolymer"),
    "microsatellite": dict(seed=102, kind="microsatellite"),
    "inverted": dict(seed=103, kind="inverted"),
    "family": dict(seed=104, kind="family"),
    "all": dict(seed=105, kind="all"),
    "long": dict(seed=105, kind="all", rounds=3, lr_len=42000),    # reads of 40 kb and more: several mask segments
    "huge": dict(seed=105, kind="all", rounds=6, lr_len=110000),   # reads of 100 kb and more
    "dropout": dict(seed=105, kind="all", lr_len=8000, dropout=True),
}
CASES = [(name, k) for name in ("homopolymer", "microsatellite", "inverted", "family") for k in (31, 21)] + [("all", k) for k in (31, 21, 25, 19)]
CASE_IDS = ["%s-k%d" % c for c in CASES]

PINNED = {  # SHA-256 of PREFIX.ref.fa, PREFIX.sr.fq, PREFIX.lr.fq
    "homopolymer": ["3be950b15285462da835b9b95a5018d0c8efdd13be1c7e306760092d3f696d4d",
                   "0e2b918c9fdb0735985edbdfe87ca134e070b1d80c14807d2c57101da9ea0979",
                   "6ad40ff657738119c7114f01b4527d17545833f0c077e4162161cd357a001cfd"],
    "microsatellite": ["669b919eab0caa34477b2d1954803b12d44437e5aaf0278a432356c7db47bec3",
                      "ba1909558e7657a4d155f51260a740bbedd4caef08278844e37b0129c563d5b2",
                      "df3a1a3cc439ac816c2750b70a43a630d4c0cb481659723809c102e2f908e965"],
    "inverted": ["4ca19926990c009f559bee1942abaa3a477e598ba3c6a3cf36f495b02ce84fed",
                "49aa467eb02a5fec080fe461a8def570077873288847359f09af950c5a8e7c94",
                "1f8ba3bd181252124a9573582c5837670ee30f9b5ced192ad76e81d461d6d9c1"],
    "family": ["7cdba8d9df0ff2143bd4d04ef746dda0dd1b675556d86cc9214b6b56a49b3bf8",
              "589e063ec88ce9414ecd07348a6346057d093509e3e2e76f5955a8f3f605c4f2",
              "a6490e902af4e1420aa9d674cfc9c3975e093882bd27d77826007952af38fe06"],
    "all": ["e94a35d7442407a91484c22b700a3c064f2251eabe6216eeb7380dc63f4e8498",
           "04f74f72ec348abb06f11eaf13077f00a4f4b74b398a0295e82f8a74e2dab5c4",
           "be8f2f68cc2e4d0e6a3a6a6cd6a7fe40fa24b4e3c88e54130de9a1cdd00707fb"],
    "long": ["309bf56f5c3fad7e43b57949cdfbbb005ab53a8babef91c2e589ef93c6f7ea6a",
            "4333c9e0eeb515e34663ddcbcccef481d40b8dabcfd217515f5173c27c7c54b4",
            "9aad9d99cc12965f90480671855b04f20d83ad1d94b1d26d2b486858e67b609a"],
    "huge": ["590bf7f0786334833a025133ea0f077e09b05e4e5d2709f9ebeacc3f03479576",
            "387fb6ae5d558b46489476301777fe185e407972c44fdf3d8f8f9806073ebb95",
            "ba5ca483d742ec6396fbf15beec6114506266cd280c12c5f8aa0165f6dab43aa"],
    "dropout": ["e94a35d7442407a91484c22b700a3c064f2251eabe6216eeb7380dc63f4e8498",
               "8d70f7d3c3bda71fb9902be7311cd4dedcfac5044fb9423a41342ba269288bde",
               "f2edd17bbb0126d36934dfcab82020d68898ebfd96c5ea328b9c60705c8770f4"],
}


class _Sets:
    """the generated sets and their indexes, made once per module on first use"""

    def __init__(self, root):
        self.root, self.sets, self.traces, self.second = str(root), {}, {}, set()

    def get(self, name):
        if name not in self.sets:
            pre = os.path.join(self.root, name)
            self.sets[name] = (pre, hg.write_set(pre, **SPECS[name]))
        return self.sets[name]

    def index(self, name, k):
        """PREFIX.index.kK.* by the plain tool with --snps (what the reference's `index` writes); returns (prefix, the tool's messages)"""
        pre, _ = self.get(name)
        if (name, k) not in self.traces:
            self.traces[name, k] = IB._build(pre + ".sr.fq", pre, k, [])[2]
        return pre, self.traces[name, k]

    def pass2(self, name):
        pre, _ = self.index(name, 31)
        if name not in self.second:
            P2._second_pass_from(pre)
            self.second.add(name)
        return pre


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _Sets(tmp_path_factory.mktemp("hard_genomes"))


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_generated_files_are_pinned(sets):
    """the generator draws from splitmix64 in integer arithmetic: the same bytes on every machine and Python"""
    for name in SPECS:
        pre, _ = sets.get(name)
        assert [_sha(pre + ext) for ext in (".ref.fa", ".sr.fq", ".lr.fq")] == PINNED[name], name


# ---- conditions that keep the tests from passing on nothing ----

def _unitigs(pre, k):
    return [l for l in gzip.open(pre + ".index.k%d.fasta.gz" % k, "rt").read().split("\n") if l and l[0] != ">"]


def _meets_itself(u, k):
    """'loop': the unitig's last (k-1)-mer is its first (an edge to itself); 'hairpin': an end (k-1)-mer that is its own reverse complement"""
    out = []
    if len(u) > k - 1 and u[:k - 1] == u[-(k - 1):]:
        out.append("loop")
    if u[:k - 1] == hg.rc(u[:k - 1]) or u[-(k - 1):] == hg.rc(u[-(k - 1):]):
        out.append("hairpin")
    return out


def _features(pre, k, trace):
    us = _unitigs(pre, k)
    return dict(unitigs=len(us),
                homopolymer=sum(1 for u in us if any(c * k in u for c in "ACGT")),
                loop=sum(1 for u in us if "loop" in _meets_itself(u, k)),
                hairpin=sum(1 for u in us if "hairpin" in _meets_itself(u, k)),
                short_cycle=int(re.search(r"(\d+) unitigs in short cycles", trace).group(1)),
                snp=int(re.search(r"(\d+) SNP annotations", trace).group(1)))


@pytest.mark.parametrize("name,k", CASES + [("long", 31), ("huge", 31), ("dropout", 31), ("dropout", 21)], ids=CASE_IDS + ["long-k31", "huge-k31", "dropout-k31", "dropout-k21"])
def test_sets_hold_what_their_kind_names(sets, name, k):
    pre, trace = sets.index(name, k)
    man = sets.get(name)[1]
    kind = SPECS[name]["kind"]
    f = _features(pre, k, trace)
    print(name, k, f)
    assert f["snp"] > 0
    if kind in ("homopolymer", "all"):
        assert f["homopolymer"] > 0 and f["loop"] > 0  # the k-mer of one base is its own successor
    if kind in ("inverted", "all"):
        assert f["hairpin"] > 0
    if kind in ("homopolymer", "microsatellite", "all"):
        assert f["short_cycle"] > 0
    # by construction: the second haplotype differs where the table of hard_genomes says so, and every structure lies inside three long reads
    h1, h2 = man["haps"]
    labels = [s[0].split(".")[0] for s in man["structures"]]
    want = {"homopolymer": ["homopolymer_%d" % n for n in hg.HOMOPOLYMER_LENGTHS], "microsatellite": ["microsatellite_"] * len(hg.MICROSATELLITES),
            "inverted": ["inverted_%d_%d" % x for x in hg.INVERTED], "family": ["family_%d" % i for i in range(hg.FAMILY_COPIES)]}
    for kd, ls in want.items():
        if kind in (kd, "all"):
            for l in ls:
                assert any(x.startswith(l) for x in labels), l
    for label, c1, c2 in man["structures"]:
        if label.startswith("window"):
            continue
        n_in = sum(1 for r in man["reads"] if r["start"] <= (c1, c2)[r["hap"]][0] and (c1, c2)[r["hap"]][1] <= r["end"])
        assert n_in >= 3, (label, n_in)
        if label.startswith("inverted"):
            s = h1[c1[0]:c1[1]]
            assert s == hg.rc(s) or int(label.split(".")[0].split("_")[2]) > 0  # an empty spacer: the whole structure is its own reverse complement
        if label.startswith("homopolymer"):
            assert len(set(h1[c1[0]:c1[1]])) == 1 and (c1[1] - c1[0]) - (c2[1] - c2[0]) in (0, 1, 3)
    assert {r["hap"] for r in man["reads"]} == {0, 1} and {r["rev"] for r in man["reads"]} == {True, False}
    tiled = [r for r in man["reads"] if r["end"] - r["start"] > hg.PLAIN_LEN]  # (all but the short reads over plain flank)
    assert len(man["reads"]) - len(tiled) == hg.PLAIN_READS and any(r["burst"] for r in tiled)
    if name == "long":
        assert min(len(r["seq"]) for r in tiled) >= 40000
    if name == "huge":
        assert min(len(r["seq"]) for r in tiled) >= 100000


# ---- index ----

def _colour_args(pre):
    return ["--colour-reads", pre + ".lr.fq", "--snps"]


def _index_same_files(sets, tmp, mode, cases, device_steps=False):
    """`mode` writes the plain tool's two files, byte for byte: with --snps at k1, and at k = 63 with --colour-reads"""
    for name in sorted({c[0] for c in cases}):
        pre, _ = sets.get(name)
        trace = IB._same(tmp, name, pre + ".sr.fq", mode, ks=tuple(k for n, k in cases if n == name))
        t63 = TW._same_as_plain(tmp, name, pre + ".sr.fq", 63, mode, _colour_args(pre))
        if device_steps:
            TW._device_steps_ran(trace); TW._device_steps_ran(t63)


def test_fast_index_writes_the_plain_files(sets, tmp_path):
    _index_same_files(sets, str(tmp_path), "--fast", CASES)


ORACLE_CASES = [c for c in CASES if c[0] != "all"]


def test_index_against_the_independent_oracle(sets, tmp_path):
    """unitigs up to strand and rotation, colour sets and coverage of the plain and the --fast builder are oracle/oracle_index.py's; a k = 63 index
    coloured by long reads as well. (The Python oracle takes seconds per build on the 55 kb genome of the `all` kind: that one by the --fast builder alone,
    whose files test_fast_index_writes_the_plain_files holds to the plain builder's.)"""
    tmp = str(tmp_path)
    for name, k in ORACLE_CASES:
        sr = sets.get(name)[0] + ".sr.fq"
        n = IB._index_vs_oracle(sr, os.path.join(tmp, "%s_plain" % name), k, [])
        assert n > 10
        assert IB._index_vs_oracle(sr, os.path.join(tmp, "%s_fast" % name), k, ["--fast"]) == n
    sr = sets.get("all")[0] + ".sr.fq"
    for k in (31, 21):
        assert IB._index_vs_oracle(sr, os.path.join(tmp, "all_fast"), k, ["--fast"]) > 10
    for name in ("microsatellite", "inverted"):
        pre = sets.get(name)[0]
        assert IB._index_vs_oracle(pre + ".sr.fq", os.path.join(tmp, name + "_c63"), 63, ["--fast"], colour=pre + ".lr.fq") > 10


# ---- lookup and seeds ----

def _check_lookup(pre, k, lib, pg=None):
    """exact hits of every long read are the oracle's; every k-mer of every unitig that meets itself (loop, hairpin) or holds a homopolymer k-mer is
    found where it lies, on the forward strand"""
    fa, rt = pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k
    og = op.Graph(fa, rt, k)
    pg = pg or api.Graph(fa, rt, k, device=0, lib_path=lib)
    for name, s, q in op.read_fastq(pre + ".lr.fq"):
        assert pg.lookup_exact(s) == og.exact(s), name
    n = 0
    for u in range(og.n_unitigs):
        s = og.unitig(u)["seq"]
        if _meets_itself(s, k) or any(c * k in s for c in "ACGT"):
            hits = pg.lookup_exact(s)
            assert hits == [(u << 33) | (i << 1) | 1 for i in range(len(s) - k + 1)] == og.exact(s), (u, s[:60])
            assert pg.lookup_exact(hg.rc(s)) == og.exact(hg.rc(s))
            n += 1
    return n


def _check_seeds(sets, name, k, lib, monkeypatch):
    """anchors of every long read, by the half-k-mer index and by spelling every variant. Weak anchors must exist in every set at every k (at k <= 21 the exact
    hits of a read at 7 % errors are too dense to leave a gap to the 1-edit search: the bursts of errors that hard_genomes puts into every fourth read do)"""
    pre, _ = sets.index(name, k)
    n_weak = SS._check(pre, None, lib, k)
    print(name, k, "weak anchors:", n_weak)
    assert n_weak > 0
    monkeypatch.setenv("RTK_INEXACT_ENUM", "1")
    assert SS._check(pre, None, lib, k) == n_weak
    monkeypatch.delenv("RTK_INEXACT_ENUM")


@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_sim_lookup_and_seeds(sets, name, k, monkeypatch):
    pre, _ = sets.index(name, k)
    n = _check_lookup(pre, k, SIM_LIB)
    assert n > 0 or SPECS[name]["kind"] in ("family", "microsatellite")
    _check_seeds(sets, name, k, SIM_LIB, monkeypatch)


def _check_long_reads(sets, lib, monkeypatch):
    """reads of 40 kb and more: the mask in several segments (8192 windows by default, 4096 as well); reads of 100 kb and more"""
    pre, _ = sets.index("long", 31)
    assert SS._check(pre, None, lib) > 0
    monkeypatch.setenv("RTK_MASK_SEG", "4096")
    assert SS._check(pre, None, lib) > 0
    monkeypatch.delenv("RTK_MASK_SEG")
    _check_pass1(sets, "long", 31, lib, monkeypatch)
    _check_pass1(sets, "huge", 31, lib, monkeypatch)


def test_sim_long_reads(sets, monkeypatch):
    _check_long_reads(sets, SIM_LIB, monkeypatch)


# ---- pass 1 ----

def _check_pass1(sets, name, k, lib, monkeypatch, max_gap="256"):
    """wave kernel alone and with the lane kernel on: sequence and quality bytes of every read are the oracle's; every read is changed; the region
    stage and the lane kernel had work of their own"""
    pre, _ = sets.index(name, k)
    st = LR._check(pre, None, lib, monkeypatch, k=k, max_gap=max_gap, min_lane_share=LANE_FLOOR)
    print(name, k, "lane class %d, handed on %d: %.3f kept" % (st["n_lane_regions"], st["n_lane_handed"], 1 - st["n_lane_handed"] / st["n_lane_regions"]))
    assert st["n_regions"] > 0 and st["n_expand"] > 0
    reads = op.read_fastq(pre + ".lr.fq")
    seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
    og = op.Graph(pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k, k)
    want, cnt = og.correct_batch(seqs, quals, threads=4)
    print(name, k, "n_expand: device %d, reference walk %d" % (st["n_expand"], cnt["n_expand"]))
    same = [r[0] for r, w in zip(reads, want) if r[1] == w[0]]
    assert not same, ("reads the oracle leaves as they are", same)
    monkeypatch.delenv("RTK_LANE_MAX_GAP")
    return seqs, want


@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_sim_pass1(sets, name, k, monkeypatch):
    _check_pass1(sets, name, k, SIM_LIB, monkeypatch)


COUNTERS_HOLD = ("homopolymer", "inverted", "family")
OTHER_OPTIONS = dict(insert_sz=300, max_len_weak_region1=300, max_qual=30, min_confidence_snp_corr=0.5)  # -i / -w / -Q / -m


def _check_pass1_settings(sets, name, k, lib, monkeypatch):
    """a narrower lane class, other options, work areas that overflow (with and without the lane kernel)"""
    pre, _ = sets.index(name, k)
    LR._check(pre, None, lib, monkeypatch, k=k, max_gap="64", min_lane_share=LANE_FLOOR)
    monkeypatch.delenv("RTK_LANE_MAX_GAP")
    # (the counter check of test_sim_correct, device events <= the reference walk's, only where there are no microsatellites: rtk_explore_subgraph walks a
    # second time where its first, pruned walk met a live candidate, often enough on microsatellites for n_expand to exceed the reference's; _check_pass1 prints both)
    SC._check(pre, None, lib, counters_must_match=SPECS[name]["kind"] in COUNTERS_HOLD, k=k, opts=OTHER_OPTIONS)
    monkeypatch.setenv("RTK_TEST_TINY_SCRATCH", "1")
    st, _, _ = SC._check(pre, None, lib, counters_must_match=False, k=k)
    assert st["n_arena_overflow"] > 0
    monkeypatch.setenv("RTK_LANE_MAX_GAP", "256")
    got, st, seqs, quals = LR._run(pre, None, lib, k)
    assert got == LR._oracle(pre, seqs, quals, k)
    assert st["n_arena_overflow"] > 0 and st["n_lane_regions"] > 0
    monkeypatch.delenv("RTK_LANE_MAX_GAP"); monkeypatch.delenv("RTK_TEST_TINY_SCRATCH")


@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_sim_pass1_settings(sets, name, k, monkeypatch):
    _check_pass1_settings(sets, name, k, SIM_LIB, monkeypatch)


def _check_dropout(sets, k, lib, monkeypatch):
    """windows of 200 .. 3000 bp without a single short read: long weak regions, regions above -w left alone. At least one read comes back with
    1000+ bp of its input, untouched, across the 1500 or the 3000 bp window."""
    seqs, want = _check_pass1(sets, "dropout", k, lib, monkeypatch)
    man = sets.get("dropout")[1]
    kept = set()
    for label, i, x, y in man["over_windows"]:
        if label in ("window_1500", "window_3000") and any(seqs[i][p:p + 1000] in want[i][0] for p in range(x, y - 1000 + 1, 20)):
            kept.add(i)
    print("dropout", k, "reads with 1000+ bp untouched across a window:", len(kept))
    assert kept
    pre = sets.get("dropout")[0]
    SC._check(pre, None, lib, counters_must_match=False, k=k, opts=OTHER_OPTIONS)


def test_sim_dropout(sets, monkeypatch):
    for k in (31, 21):
        _check_dropout(sets, k, SIM_LIB, monkeypatch)


# ---- pass 2 ----

KINDS = hg.KINDS


def _check_second_pass(sets, name, lib, monkeypatch):
    """built from the oracle's pass-1 output: bytes of the oracle at k = 31 and k = 63, the phasing skip, -f"""
    pre = sets.pass2(name)
    P2._check_pass2(pre, lib, k=31)
    P2._check_pass2(pre, lib, k=63)
    skipped, n = P2._skip_check(pre, lib, monkeypatch, k=63)  # (0 < skipped < n: the short reads over plain flank have nothing to remove)
    print(name, "pass 2, k = 63: alignment skipped for %d of %d reads" % (skipped, n))
    monkeypatch.delenv("RTK_PHASE_ALIGN_ALL")
    FS._check_end_to_end(pre, lib, 63, None)


@pytest.mark.parametrize("name", KINDS)
def test_sim_pass2(sets, name, monkeypatch):
    _check_second_pass(sets, name, SIM_LIB, monkeypatch)


# ---- MI355X ----

@pytest.mark.gpu
def test_gpu_index_writes_the_plain_files(sets, tmp_path):
    """counting, unitigs and colours on the device (the trace says so): the plain tool's files, byte for byte"""
    _index_same_files(sets, str(tmp_path), "--gpu", CASES, device_steps=True)


@pytest.mark.gpu
def test_gpu_index_against_the_independent_oracle(sets, tmp_path):
    """(k = 31 of every kind and both k of the microsatellites; the other k are held to the plain builder's files above, and those to the oracle in the CPU tier)"""
    tmp = str(tmp_path)
    for name, k in [(n, 31) for n in KINDS] + [("microsatellite", 21)]:
        assert IB._index_vs_oracle(sets.get(name)[0] + ".sr.fq", os.path.join(tmp, "%s_gpu" % name), k, ["--gpu"]) > 10
    for name in ("microsatellite", "inverted"):
        pre = sets.get(name)[0]
        assert IB._index_vs_oracle(pre + ".sr.fq", os.path.join(tmp, name + "_c63"), 63, ["--gpu"], colour=pre + ".lr.fq") > 10


def _raw_events(pre, k):
    """(unitig, read) events that k_col_map (csrc/hip/rtk_index.hip) writes for PREFIX.sr.fq handed over as ONE chunk in file order (what a plain file below
    32 MB is): the reads one after the other, a separator behind each; an event wherever a k-mer lies on another unitig than the one before it, or on one
    at all after a miss, and at every 64th character of a run (a wavefront does not look into the one before it)."""
    where = {}
    for u, s in enumerate(_unitigs(pre, k)):
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            where[min(w, hg.rc(w))] = u
    n = at = 0
    for _, s, _q in op.read_fastq(pre + ".sr.fq"):
        prev = -1
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            u = where.get(min(w, hg.rc(w)), -1)
            n += u >= 0 and (u != prev or (at + i) % 64 == 0)
            prev = u
        at += len(s) + 1
    return n


@pytest.mark.gpu
def test_gpu_index_colours_with_a_small_event_buffer(sets, tmp_path, monkeypatch):
    """The (unitig, read) events of the --gpu colouring, sorted and thinned out while the reads still come (RTK_INDEX_EVENTS, as
    test_index_build.test_gpu_index_colours_with_a_small_event_buffer sets it). A read inside a microsatellite goes round a cycle of 2..6 unitigs and
    writes an event at every step for a handful of distinct ones.
    (1) The short reads of the `huge` set (36 microsatellites, 66 homopolymers, 12 Mb of bases) as gzip: the reader hands 1 Mb pieces to 16 feeder threads and
    every thread sends a chunk of its own, so the device looks at its buffer between chunks. Room for 1.75 times the distinct events: half of it is less
    than the distinct events, so it thins out mid-stream (more than the one time at the end), and the files are the plain tool's.
    (2) The microsatellite set is one chunk, and its events before thinning (counted here from the plain index) exceed 1.5 times the distinct ones: the
    tool says that they do not fit between two looks and writes nothing -- an error, never a loss."""
    import gzip as gz
    tmp = str(tmp_path)
    monkeypatch.setenv("RTK_INDEX_THREADS", "16")
    pre, _ = sets.get("huge")
    srz = os.path.join(tmp, "huge.sr.fq.gz")
    with open(pre + ".sr.fq", "rb") as f, gz.open(srz, "wb", compresslevel=1) as g:
        g.write(f.read())
    a = IB._build(pre + ".sr.fq", os.path.join(tmp, "huge_plain"), 31, [])
    b = IB._build(srz, os.path.join(tmp, "huge_gpu0"), 31, ["--gpu"])
    assert a[0] == b[0] and a[1] == b[1]
    n_distinct, n_chunks = int(re.search(r"-> (\d+) distinct", b[2]).group(1)), int(re.search(r"in (\d+) chunks", b[2]).group(1))
    assert n_chunks >= 4, b[2]
    monkeypatch.setenv("RTK_INDEX_EVENTS", str(n_distinct * 7 // 4))
    b = IB._build(srz, os.path.join(tmp, "huge_gpu"), 31, ["--gpu"])
    assert a[0] == b[0] and a[1] == b[1]
    n_thinned = int(re.search(r"thinned out (\d+) times", b[2]).group(1))
    print("huge: %d distinct events in %d chunks, thinned out %d times" % (n_distinct, n_chunks, n_thinned))
    assert n_thinned >= 2, b[2]
    assert int(re.search(r"-> (\d+) distinct", b[2]).group(1)) == n_distinct
    monkeypatch.delenv("RTK_INDEX_EVENTS")
    pre, _ = sets.index("microsatellite", 31)
    b = IB._build(pre + ".sr.fq", os.path.join(tmp, "ms_gpu0"), 31, ["--gpu"])
    n_distinct, raw = int(re.search(r"-> (\d+) distinct", b[2]).group(1)), _raw_events(pre, 31)
    print("microsatellite: %d distinct events, %d before thinning" % (n_distinct, raw))
    assert int(re.search(r"in (\d+) chunks", b[2]).group(1)) == 1 and raw > n_distinct * 3 // 2
    monkeypatch.setenv("RTK_INDEX_EVENTS", str(n_distinct * 3 // 2))
    out = os.path.join(tmp, "ms_small")
    r = subprocess.run([os.path.join(BIN, "rtk_build_index"), "-s", pre + ".sr.fq", "-o", out, "--gpu", "--snps"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "events" in r.stderr and not os.path.exists(out + ".index.k31.rtsk"), r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_gpu_tables_lookup_and_seeds(sets, name, k, monkeypatch):
    """the tables built in HBM are the host's; lookups through them; anchors"""
    pre, _ = sets.index(name, k)
    dev = GL._check_device_tables(pre, k)
    n = _check_lookup(pre, k, GPU_LIB, pg=dev)
    assert n > 0 or SPECS[name]["kind"] in ("family", "microsatellite")
    _check_lookup(pre, k, GPU_LIB)
    _check_seeds(sets, name, k, GPU_LIB, monkeypatch)
    if name == "microsatellite":  # half-k-mers with very long lists, the index sorted in several ranges of leading bits
        monkeypatch.setenv("RTK_HX_PART_KEYS", "2000")
        GL._check_device_tables(pre, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", KINDS)
def test_gpu_tables_two_word_kmers(sets, name):
    pre = sets.pass2(name)
    GL._check_device_tables(pre + ".p2", 63)


@pytest.mark.gpu
def test_gpu_long_reads(sets, monkeypatch):
    _check_long_reads(sets, GPU_LIB, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_gpu_pass1(sets, name, k, monkeypatch):
    _check_pass1(sets, name, k, GPU_LIB, monkeypatch)
    _check_pass1_settings(sets, name, k, GPU_LIB, monkeypatch)


@pytest.mark.gpu
def test_gpu_pass1_stolen_regions_that_overflow(sets, monkeypatch):
    """the setting of test_lanes_regions.test_gpu_stolen_regions_that_overflow_are_redone: one slow lane wave, the wave kernel steals the class, tiny work areas"""
    monkeypatch.setenv("RTK_LANE_MAX_GAP", "256")
    monkeypatch.setenv("RTK_LANE_WAVES", "1"); monkeypatch.setenv("RTK_LANE_ROUND", "4")
    monkeypatch.setenv("RTK_TEST_TINY_SCRATCH", "1")
    for name, k in CASES:
        pre, _ = sets.index(name, k)
        got, st, seqs, quals = LR._run(pre, None, GPU_LIB, k)
        want = LR._oracle(pre, seqs, quals, k)
        assert got == want, "%s k=%d: %d reads differ from the oracle" % (name, k, sum(1 for a, b in zip(got, want) if a != b))
        assert st["n_arena_overflow"] > 0


@pytest.mark.gpu
def test_gpu_dropout(sets, monkeypatch):
    for k in (31, 21):
        _check_dropout(sets, k, GPU_LIB, monkeypatch)


@pytest.mark.gpu
def test_gpu_pipelined_batches_and_small_tickets(sets):
    """the `all` set as three batches through api.run_pipelined (every batch twice), then as many small tickets from eight callers at once"""
    pre, _ = sets.index("all", 31)
    fa, rt = pre + ".index.k31.fasta.gz", pre + ".index.k31.rtsk"
    og, pg = op.Graph(fa, rt, 31), api.Graph(fa, rt, 31, device=0)
    reads = op.read_fastq(pre + ".lr.fq")
    want, _ = og.correct_batch([r[1] for r in reads], [r[2] for r in reads], threads=8)
    cut = [0, len(reads) // 3, 2 * len(reads) // 3, len(reads)]
    batches = [api.Batch(pg, [r[1] for r in reads[a:b]], [r[2] for r in reads[a:b]]) for a, b in zip(cut, cut[1:])]
    api.run_pipelined(batches + batches)
    for (a, b), bt in zip(zip(cut, cut[1:]), batches):
        assert bt.fetch() == want[a:b]
    parts = [(i, min(i + 4, len(reads))) for i in range(0, len(reads), 4)] * 2
    out, err, nxt, lock = [None] * len(parts), [], [0], threading.Lock()

    def caller():
        while True:
            with lock:
                i = nxt[0]; nxt[0] += 1
            if i >= len(parts):
                return
            try:
                a, b = parts[i]
                bt = api.Batch(pg, [r[1] for r in reads[a:b]], [r[2] for r in reads[a:b]]); bt.run(pg.opts()); out[i] = bt.fetch(); bt.close()
            except Exception as e:  # noqa: BLE001
                err.append(repr(e))

    th = [threading.Thread(target=caller) for _ in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not err, err[:2]
    for i, (a, b) in enumerate(parts):
        assert out[i] == want[a:b], "ticket %d differs" % i


@pytest.mark.gpu
@pytest.mark.parametrize("name", KINDS)
def test_gpu_pass2(sets, name, monkeypatch):
    _check_second_pass(sets, name, GPU_LIB, monkeypatch)
    # the multi-wave phasing kernel forced onto every read longer than 2 kb (test_pass2.test_gpu_pass2_multiwave_kernel)
    monkeypatch.setenv("RTK_PHASE_LONG", "2000")
    P2._check_pass2(sets.pass2(name), GPU_LIB, k=63)


@pytest.mark.gpu
def test_gpu_pass2_long_reads_on_the_multiwave_kernel(sets):
    """reads of 40 kb and more through the whole-read alignment of phasing() with its default threshold"""
    sets.index("long", 31)
    pre = sets.pass2("long")
    og, pg, seqs, quals, raws = P2._load(pre, GPU_LIB, 63)
    want = og.correct_batch2(seqs, quals, raws, og.opts(long_read_correct=1), threads=12)
    assert pg.correct_batch(seqs, quals, pg.opts(long_read_correct=1), raw=raws) == want


@pytest.mark.gpu
def test_gpu_one_command_on_the_all_set(sets, tmp_path):
    """`correct -s .. -l .. -o ..` equals the four steps by hand, and both equal the oracle run on the indexes of the hand-made steps"""
    exe, tool = os.path.join(BIN, "Ratatosk"), os.path.join(BIN, "rtk_build_index")
    pre, _ = sets.get("all")
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    hand = str(tmp_path / "hand")
    def run(args):
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (args, r.stderr[-2000:])
    run([tool, "--gpu", "-k", "31", "-s", sr, "--snps", "-o", hand + "_i1"])
    run([exe, "correct", "-1", "-c", "2", "-g", hand + "_i1.index.k31.fasta.gz", "-d", hand + "_i1.index.k31.rtsk", "-l", lr, "-o", hand])
    run([tool, "--gpu", "-k", "63", "-s", sr, "--colour-reads", hand + ".2.fastq", "--snps", "-o", hand + "_i2"])
    run([exe, "correct", "-2", "-c", "2", "-g", hand + "_i2.index.k63.fasta.gz", "-d", hand + "_i2.index.k63.rtsk", "-l", hand + ".2.fastq", "-L", lr, "-o", hand])
    sub = tmp_path / "one"; sub.mkdir()
    run([exe, "correct", "-c", "2", "-s", sr, "-l", lr, "-o", str(sub / "out")])
    assert open(str(sub / "out.fastq"), "rb").read() == open(hand + ".fastq", "rb").read()
    assert sorted(os.listdir(str(sub))) == ["out.fastq"]
    raw = op.read_fastq(lr)
    o1 = op.Graph(hand + "_i1.index.k31.fasta.gz", hand + "_i1.index.k31.rtsk", 31)
    p1, _ = o1.correct_batch([r[1] for r in raw], [r[2] for r in raw], threads=8)
    assert [(r[1], r[2]) for r in op.read_fastq(hand + ".2.fastq")] == p1
    o2 = op.Graph(hand + "_i2.index.k63.fasta.gz", hand + "_i2.index.k63.rtsk", 63)
    want = o2.correct_batch2([s for s, _ in p1], [q for _, q in p1], [r[1] for r in raw], o2.opts(long_read_correct=1), threads=8)
    got = op.read_fastq(str(sub / "out.fastq"))
    assert [(g[1], g[2]) for g in got] == want and [g[0] for g in got] == [r[0] for r in raw]
