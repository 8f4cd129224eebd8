"""The candidate search of the SNP annotations on the device (rtk_index_snp_candidates; `rtk_build_index --gpu --snps` with RTK_INDEX_SNPS=device).

The stage is held to a brute force kept in this file: a dictionary from canonical k-mer to unitig, and for every window, every offset and every other base a
look-up of the variant (the rule of oracle/oracle_annot.py, snp_annotations: a variant on the window's own unitig is no candidate). Hand-made unitigs at
k = 11 (2k < 24: the prefix tables are the whole key), 21 and 31 (one-word keys), 33 (the first two-word k) and 63 (the largest), then the unitigs of two
simulated indexes. The tool is held to the plain tool and to its own host route: the same two files, byte for byte.

CPU tier: the simulator build has the symbol and refuses it, the interface revision stays 10, the replay that all routes share still gives `--fast` and the
plain tool the same bytes, and RTK_INDEX_SNPS without --gpu changes nothing."""
import gzip
import os
import random
import re
import subprocess

import pytest

import hard_genomes as hg
import test_index_build as IB
from conftest import BIN, ROOT, SIM_LIB
from ratatosk_amd import api

LIB = os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so")
GPU_STEP_TIMEOUT = 300  # seconds, every child process that opens the GPU
SMALL_JOB = {"RTK_INDEX_EVENTS": "4000000"}  # room for 4 M colour events instead of 60 % of the device memory: opening the colouring job then takes no seconds
KS = (11, 21, 31, 33, 63)
RTK_ERR_FORMAT, RTK_ERR_DEVICE, RTK_ERR_UNSUPPORTED = -2, -5, -6


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def canonical(x):
    return min(x, rc(x))


def table_of(unitigs, k):
    """canonical k-mer -> unitig; a k-mer on two unitigs (or twice on one) is an error of the case"""
    t = {}
    for u, s in enumerate(unitigs):
        for p in range(len(s) - k + 1):
            c = canonical(s[p:p + k])
            assert c not in t, "the case holds a canonical k-mer twice: unitigs %d and %d" % (t[c], u)
            t[c] = u
    return t


def brute(unitigs, k, searched=None, own=False):
    """every (u, p, j, alt, w): window p of unitig u with base alt at offset j is a k-mer of unitig w != u (own: w == u as well), by (u, p, j, alt)"""
    t, out = table_of(unitigs, k), []
    t.update([(rc(c), u) for c, u in t.items()])  # a k-mer is in the graph when its canonical form is: both strands, one look-up per variant
    for u, s in enumerate(unitigs):
        if searched is not None and not searched[u]:
            continue
        for p in range(len(s) - k + 1):
            x = s[p:p + k]
            for j in range(k):
                head, cur, tail = x[:j], x[j], x[j + 1:]
                for alt, b in enumerate("ACGT"):
                    if b != cur:
                        w = t.get(head + b + tail)
                        if w is not None and (own or w != u):
                            out.append((u, p, j, alt, w))
    return out


def first_per_site(cands):
    """of the candidates with equal (u, p + j, alt) the one with the smallest p; again by (u, p, j, alt)"""
    best = {}
    for c in cands:
        key = (c[0], c[1] + c[2], c[3])
        if key not in best or c[1] < best[key][1]:
            best[key] = c
    return sorted(best.values())


def random_seq(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def star(k, seed=1):
    """X and its 3k one-substitution variants, one window each"""
    x = random_seq(random.Random(1000 * seed + k), k)
    return [x] + [x[:j] + b + x[j + 1:] for j in range(k) for b in "ACGT" if b != x[j]]


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_simulator_build_refuses_the_stage():
    with pytest.raises(api.RtkError) as e:
        api.index_snp_candidates(star(11), 11, lib_path=SIM_LIB)
    assert "rtk error %d:" % RTK_ERR_UNSUPPORTED in str(e.value) and "rtk_index_snp_candidates" in str(e.value), str(e.value)


def test_interface_revision_stays_10():
    for path in (LIB, SIM_LIB):
        assert api.load_library(path).rtk_api_revision() == 10, path


@pytest.fixture(scope="module")
def many_neighbours(tmp_path_factory):
    """the reads of the `many_neighbours` recipe and the index the plain tool writes for them at k = 21"""
    tmp = str(tmp_path_factory.mktemp("many_neighbours"))
    name, args = IB.SETS[3]
    assert name == "many_neighbours"
    sr = IB._simulated(tmp, name, args)
    return tmp, sr, IB._build(sr, os.path.join(tmp, "plain"), 21, [])


def test_fast_and_plain_share_the_replay(many_neighbours):
    tmp, sr, plain = many_neighbours
    fast = IB._build(sr, os.path.join(tmp, "fast"), 21, ["--fast"])
    assert plain[0] == fast[0] and plain[1] == fast[1]
    assert "SNP search on the host threads: candidate search" in fast[2] and "SNP search on the host threads: candidate search" in plain[2]  # the split of the lap, traced


def test_the_knob_is_ignored_without_gpu(many_neighbours, monkeypatch):
    tmp, sr, plain = many_neighbours
    monkeypatch.setenv("RTK_INDEX_SNPS", "device")
    for mode in ([], ["--fast"]):
        got = IB._build(sr, os.path.join(tmp, "knob" + "".join(mode)), 21, mode)
        assert plain[0] == got[0] and plain[1] == got[1], mode
        assert "rtk_index_snps:" not in got[2] and "SNP candidates on the host threads" not in got[2], got[2]


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the stage

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_star(k):
    """X has a neighbour at every offset and with every other base; every satellite has X and its two same-offset siblings"""
    U = star(k)
    table_of(U, k)  # all canonical k-mers distinct (the seed is chosen so)
    want = brute(U, k)
    of_x = [c for c in want if c[0] == 0]
    assert len(of_x) == 3 * k and {c[2] for c in of_x} == set(range(k)) and {0, k // 2 - 1, k // 2, k - 1} <= {c[2] for c in of_x}
    assert all(len([c for c in want if c[0] == u]) == 3 for u in range(1, len(U)))
    flipped = [canonical(U[c[4]]) != U[c[4]] for c in of_x]  # the canonical form is the reverse complement of the oriented neighbour
    assert any(flipped) and not all(flipped)
    assert api.index_snp_candidates(U, k) == want
    assert api.index_snp_candidates(U, k, first_per_site=True) == first_per_site(want) == want  # one window each: nothing to drop


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_bubbles(k):
    """Two sequences of 3k bases that differ at the middle base, as the compacted graph holds them: the windows that do not cover the site are the same k-mers in both
    (as two unitigs of 3k bases they would be k-mers on two unitigs, which the stage refuses: asserted below), so they form the two flanks, and the windows over the
    site are the two arms of 2k - 1 bases: one stored as written, one as its reverse complement. Every window of an arm covers the site and has one candidate."""
    a = random_seq(random.Random(77 + k), 3 * k)
    mid = 3 * k // 2
    b = a[:mid] + "ACGT"[("ACGT".index(a[mid]) + 1) % 4] + a[mid + 1:]
    with pytest.raises(api.RtkError) as e:
        api.index_snp_candidates([a, rc(b)], k)
    assert "rtk error %d:" % RTK_ERR_FORMAT in str(e.value), str(e.value)
    U = [a[mid - k + 1:mid + k], rc(b[mid - k + 1:mid + k]), a[:mid], a[mid + 1:]]
    want = brute(U, k)
    assert len(want) == 2 * k and len({(c[0], c[1]) for c in want}) == 2 * k and {c[0] for c in want} == {0, 1}  # every window over the site: one candidate
    assert {c[1] + c[2] for c in want} == {k - 1}  # the site, on either arm
    assert api.index_snp_candidates(U, k) == want
    kept = first_per_site(want)
    assert len(kept) == 2 and all(c[1] == min(d[1] for d in want if d[0] == c[0]) for c in kept)  # one per (u, site, alt): the smallest p
    assert api.index_snp_candidates(U, k, first_per_site=True) == kept


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_own_strand(k):
    """W m rc(W): the window is one substitution (its centre) away from its own reverse complement, which is no candidate: w == u"""
    rnd = random.Random(5 + k)
    w = random_seq(rnd, (k - 1) // 2)
    x = w + "A" + rc(w)
    other = "C" + x[1:] if x[0] != "C" else "G" + x[1:]  # one substitution away at offset 0, on another unitig
    U = [x, other, random_seq(rnd, 2 * k)]
    with_own = brute(U, k, own=True)
    assert (0, 0, k // 2, 3, 0) in with_own  # centre A -> T gives rc(x), on unitig 0 itself
    want = brute(U, k)
    assert [c for c in want if c[0] == 0] == [(0, 0, 0, "ACGT".index(other[0]), 1)]
    assert api.index_snp_candidates(U, k) == want
    with pytest.raises(api.RtkError) as e:  # the same unitig on two ids: its k-mer twice
        api.index_snp_candidates([x, other, x], k)
    assert "rtk error %d:" % RTK_ERR_FORMAT in str(e.value), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_searched_flags(k):
    U = star(k, seed=2)
    flags = [u % 2 for u in range(len(U))]  # X itself is not searched
    want = brute(U, k, flags)
    assert want and all(flags[c[0]] for c in want) and any(not flags[c[4]] for c in want)  # unflagged unitigs ask nothing and are still found
    assert api.index_snp_candidates(U, k, searched=flags) == want
    assert api.index_snp_candidates(U, k, searched=[1] * len(U)) == api.index_snp_candidates(U, k) == brute(U, k)
    assert api.index_snp_candidates(U, k, searched=[0] * len(U)) == []


@pytest.mark.gpu
def test_edge_sizes():
    assert api.index_snp_candidates([], 31) == []
    for k in KS:
        one = random_seq(random.Random(k), k)  # a unitig of exactly k bases, alone
        assert api.index_snp_candidates([one], k) == [] == brute([one], k)
        two = [one, one[:-1] + ("A" if one[-1] != "A" else "C")]  # ... and with its neighbour at the last offset
        assert api.index_snp_candidates(two, k) == brute(two, k) and len(brute(two, k)) == 2


@pytest.mark.gpu
def test_memory_refusal(monkeypatch):
    monkeypatch.setenv("RTK_INDEX_SNP_MEM", "4096")
    with pytest.raises(api.RtkError) as e:
        api.index_snp_candidates(star(31), 31)
    m = re.search(r"need (\d+) bytes of device memory, (\d+) are to be had", str(e.value))
    assert "rtk error %d:" % RTK_ERR_DEVICE in str(e.value) and m and int(m.group(1)) > 4096 and int(m.group(2)) == 4096, str(e.value)


def _unitigs_of(fasta_gz):
    return [line.strip() for line in gzip.open(fasta_gz, "rt") if not line.startswith(">")]


def _stage_against_brute(unitigs, k):
    want = brute(unitigs, k)
    assert api.index_snp_candidates(unitigs, k) == want
    assert api.index_snp_candidates(unitigs, k, first_per_site=True) == first_per_site(want)
    return want


@pytest.mark.gpu
def test_simulated_many_neighbours(many_neighbours):
    tmp, _, _ = many_neighbours
    want = _stage_against_brute(_unitigs_of(os.path.join(tmp, "plain.index.k21.fasta.gz")), 21)
    per_window = {}
    for c in want:
        per_window[c[0], c[1]] = per_window.get((c[0], c[1]), 0) + 1
    assert max(per_window.values()) > 16  # what the recipe was added for


@pytest.mark.gpu
def test_simulated_microsatellites(tmp_path):
    pre = os.path.join(str(tmp_path), "microsatellite")
    hg.write_set(pre, seed=102, kind="microsatellite")
    IB._build(pre + ".sr.fq", pre, 31, [])
    assert _stage_against_brute(_unitigs_of(pre + ".index.k31.fasta.gz"), 31)


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the tool

def _tool(sr, out, k, extra, env):
    r = subprocess.run([os.path.join(BIN, "rtk_build_index"), "-s", sr, "-o", out, "-k", str(k), "--snps"] + extra, capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT,
                       env=dict(os.environ, RTK_INDEX_TRACE="1", **dict(SMALL_JOB, **env)))
    assert r.returncode == 0, r.stderr
    return open(out + ".index.k%d.fasta.gz" % k, "rb").read(), open(out + ".index.k%d.rtsk" % k, "rb").read(), r.stderr


@pytest.fixture(scope="module")
def tool_sets(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("snp_tool"))
    out = {}
    for name, args in IB.SETS[:2]:
        pre = os.path.join(tmp, name)
        subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + args + ["--lr-n", "30", "--lr-len", "3000", "--lr-err", "0.02"], stderr=subprocess.DEVNULL)
        out[name] = pre
    return tmp, out


def _routes(tmp, tag, sr, k, extra):
    plain = _tool(sr, os.path.join(tmp, tag + "_plain"), k, extra, {})
    dev = _tool(sr, os.path.join(tmp, tag + "_dev"), k, extra + ["--gpu"], {"RTK_INDEX_SNPS": "device"})
    assert plain[:2] == dev[:2], (tag, "device route")
    assert "rtk_index_snps:" in dev[2] and "SNP candidates on the host threads" not in dev[2] and "1-substitution neighbour index built" not in dev[2], dev[2]
    return plain, dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("het_repeats", 31), ("het_repeats", 21), ("tandem", 31), ("tandem", 21), ("het_repeats", 63)])
def test_tool_writes_the_same_files(tool_sets, name, k):
    tmp, sets = tool_sets
    tag, sr = "%s_k%d" % (name, k), sets[name] + ".sr.fq"
    plain, dev = _routes(tmp, tag, sr, k, [])
    host = _tool(sr, os.path.join(tmp, tag + "_host"), k, ["--gpu"], {"RTK_INDEX_SNPS": "host"})
    assert plain[:2] == host[:2], (tag, "host route")
    assert "rtk_index_snps:" not in host[2] and "1-substitution neighbour index built" in host[2], host[2]
    back = _tool(sr, os.path.join(tmp, tag + "_back"), k, ["--gpu"], {"RTK_INDEX_SNPS": "device", "RTK_INDEX_SNP_MEM": "4096"})
    assert plain[:2] == back[:2], (tag, "fallback")
    assert "rtk_build_index: --gpu: SNP candidates on the host threads (" in back[2] and "rtk_index_snps:" not in back[2], back[2]
    assert re.search(r"\d+ SNP annotations on \d+ unitigs", dev[2]).group(0) == re.search(r"\d+ SNP annotations on \d+ unitigs", plain[2]).group(0)


@pytest.mark.gpu
def test_tool_second_pass_index(tool_sets):
    tmp, sets = tool_sets
    pre = sets["het_repeats"]
    _routes(tmp, "second_k63", pre + ".sr.fq", 63, ["--colour-reads", pre + ".lr.fq"])
