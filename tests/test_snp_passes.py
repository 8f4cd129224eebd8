"""The candidate search of the SNP annotations in passes over partitions of the key space (rtk_index_snp_candidates with RTK_INDEX_SNP_PASSES, or when the views
of all windows do not fit RTK_INDEX_SNP_MEM; rtk_index_snp_plan says beforehand what the stage will do).

The stage is held to the brute force of tests/test_snp_candidates.py and to its own single pass: the same list for every number of passes, with and without
first_per_site. The cases cross both kinds of boundary (a star's variants at the first offsets leave X's partition of view one, those at the last offsets its
partition of view two), straddle boundaries with one query range (k = 11: a range spans 2^12 prefixes of the 2^22), leave partitions empty (more passes than
keys), and share sites across partitions (the simulated sets). The tool is held to the plain tool: the same two files, byte for byte.

CPU tier: the simulator build has rtk_index_snp_plan and refuses it, the interface revision stays 10, and RTK_INDEX_SNP_PASSES without --gpu changes nothing."""
import os
import random
import re

import pytest

import test_index_build as IB
import test_snp_candidates as SC
from conftest import SIM_LIB
from ratatosk_amd import api
from test_snp_candidates import many_neighbours, tool_sets  # noqa: F401  (fixtures)

PASSES = (1, 2, 3, 7)


def _stage(monkeypatch, passes, unitigs, k, **kw):
    monkeypatch.setenv("RTK_INDEX_SNP_PASSES", str(passes))  # read at the call (rtk_knobs.h)
    return api.index_snp_candidates(unitigs, k, **kw)


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_simulator_build_refuses_the_plan():
    with pytest.raises(api.RtkError) as e:
        api.index_snp_plan(SC.star(11), 11, lib_path=SIM_LIB)
    assert "rtk error %d:" % SC.RTK_ERR_UNSUPPORTED in str(e.value) and "rtk_index_snp_plan" in str(e.value), str(e.value)


def test_interface_revision_stays_10():
    for path in (SC.LIB, SIM_LIB):
        L = api.load_library(path)
        assert L.rtk_api_revision() == 10 and hasattr(L, "rtk_index_snp_plan"), path


def test_the_knob_is_ignored_without_gpu(many_neighbours, monkeypatch):  # noqa: F811
    tmp, sr, plain = many_neighbours
    monkeypatch.setenv("RTK_INDEX_SNP_PASSES", "3")
    for mode in ([], ["--fast"]):
        got = IB._build(sr, os.path.join(tmp, "passes" + "".join(mode)), 21, mode)
        assert plain[0] == got[0] and plain[1] == got[1], mode
        assert "rtk_index_snps:" not in got[2], got[2]


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the stage

@pytest.mark.gpu
@pytest.mark.parametrize("k", SC.KS)
def test_star_in_passes(k, monkeypatch):
    U = SC.star(k)
    want = SC.brute(U, k)
    kept = SC.first_per_site(want)
    one = _stage(monkeypatch, 1, U, k)
    for p in PASSES:
        assert _stage(monkeypatch, p, U, k) == want == one, p
        assert _stage(monkeypatch, p, U, k, first_per_site=True) == kept, p


@pytest.mark.gpu
@pytest.mark.parametrize("passes", (2, 5, 64))
def test_ranges_that_straddle_boundaries(passes, monkeypatch):
    """k = 11: the tables are the whole 22-bit key, the shared half is 10 bits, so one query range spans 2^12 prefix values and the partitions of a few hundred to a thousand keys cut it"""
    k, rnd, U = 11, random.Random(4711), []
    seen = set()
    while len(U) < 600:  # unitigs of k .. k + 7 bases whose canonical k-mers are new
        s = SC.random_seq(rnd, k + rnd.randrange(8))
        kms = [SC.canonical(s[p:p + k]) for p in range(len(s) - k + 1)]
        if len(set(kms)) == len(kms) and not seen & set(kms):
            seen |= set(kms)
            U.append(s)
    SC.table_of(U, k)
    want = SC.brute(U, k)
    assert len(want) > 50 and len(SC.first_per_site(want)) < len(want)  # some 2700 of the 2^21 canonical keys taken: neighbours are rare but there
    assert _stage(monkeypatch, passes, U, k) == want
    assert _stage(monkeypatch, passes, U, k, first_per_site=True) == SC.first_per_site(want)


@pytest.mark.gpu
def test_more_passes_than_keys(monkeypatch):
    for k in (11, 31, 63):  # the whole key as prefix, one-word and two-word keys
        one = SC.random_seq(random.Random(k), k)
        assert _stage(monkeypatch, 4, [one], k) == []
        two = [one, one[:-1] + ("A" if one[-1] != "A" else "C")]
        got = _stage(monkeypatch, 256, two, k)
        assert got == SC.brute(two, k) and len(got) == 2, k
    assert _stage(monkeypatch, 3, [], 31) == []


@pytest.mark.gpu
@pytest.mark.parametrize("k", SC.KS)
def test_searched_flags_in_passes(k, monkeypatch):
    U = SC.star(k, seed=2)
    flags = [u % 2 for u in range(len(U))]
    want = SC.brute(U, k, flags)
    assert want
    assert _stage(monkeypatch, 3, U, k, searched=flags) == want


@pytest.mark.gpu
@pytest.mark.parametrize("k", SC.KS)
def test_errors_survive_partitioning(k, monkeypatch):
    rnd = random.Random(9 + k)
    x = SC.random_seq(rnd, 2 * k)
    others = [SC.random_seq(rnd, 2 * k) for _ in range(6)]
    with pytest.raises(api.RtkError) as e:  # the first window of x again, on another unitig and the other strand
        _stage(monkeypatch, 3, [x] + others + [SC.rc(x[:k])], k)
    assert "rtk error %d:" % SC.RTK_ERR_FORMAT in str(e.value) and "occurs twice" in str(e.value), str(e.value)
    y = SC.random_seq(rnd, 2 * k)
    with pytest.raises(api.RtkError) as e:
        _stage(monkeypatch, 3, [x] + others + [y[:k] + "N" + y[k + 1:]], k)
    assert "rtk error %d:" % SC.RTK_ERR_FORMAT in str(e.value) and "no base" in str(e.value), str(e.value)


@pytest.mark.gpu
def test_simulated_sets_in_passes(many_neighbours, tmp_path, monkeypatch):  # noqa: F811
    """many candidates share a site, and their windows' neighbours lie in different partitions: first_per_site picks across passes"""
    monkeypatch.setenv("RTK_INDEX_SNP_PASSES", "4")
    tmp, _, _ = many_neighbours
    assert SC._stage_against_brute(SC._unitigs_of(os.path.join(tmp, "plain.index.k21.fasta.gz")), 21)
    pre = os.path.join(str(tmp_path), "microsatellite")
    SC.hg.write_set(pre, seed=102, kind="microsatellite")
    IB._build(pre + ".sr.fq", pre, 31, [])
    assert SC._stage_against_brute(SC._unitigs_of(pre + ".index.k31.fasta.gz"), 31)


@pytest.mark.gpu
def test_memory_driven_passes(tool_sets, monkeypatch, capfd):  # noqa: F811
    """The room decides: with less than the single pass needs the stage partitions, with less than the smallest plan it refuses; rtk_index_snp_plan says which beforehand."""
    tmp, sets = tool_sets
    SC._tool(sets["het_repeats"] + ".sr.fq", os.path.join(tmp, "plan_k63"), 63, [], {})
    U = SC._unitigs_of(os.path.join(tmp, "plan_k63.index.k63.fasta.gz"))
    monkeypatch.delenv("RTK_INDEX_SNP_PASSES", raising=False)
    monkeypatch.delenv("RTK_INDEX_SNP_MEM", raising=False)
    p, one, mn = api.index_snp_plan(U, 63)
    print("windows %d, plan: passes %d, one pass %d bytes, smallest %d bytes" % (sum(len(u) - 62 for u in U), p, one, mn))
    assert p == 1 and mn < one
    before = api.index_snp_candidates(U, 63)
    assert before
    assert api.index_snp_plan(U, 63, room=(one + mn) // 2)[0] >= 2 and api.index_snp_plan(U, 63, room=one)[0] == 1 and api.index_snp_plan(U, 63, room=mn)[0] >= 2

    monkeypatch.setenv("RTK_INDEX_SNP_MEM", str((one + mn) // 2))
    assert api.index_snp_plan(U, 63) == (api.index_snp_plan(U, 63, room=(one + mn) // 2)[0], one, mn)
    monkeypatch.setenv("RTK_INDEX_TRACE", "1")
    capfd.readouterr()
    assert api.index_snp_candidates(U, 63) == before
    trace = capfd.readouterr().err
    m = re.search(r"rtk_index_snps: (\d+) passes over the key space, the largest partition holds (\d+) of (\d+) k-mers", trace)
    assert m and int(m.group(1)) >= 2 and int(m.group(2)) < int(m.group(3)), trace
    assert re.search(r"rtk_index_snps: \d+ windows .* views [0-9.]+ s, scan [0-9.]+ s", trace), trace
    monkeypatch.delenv("RTK_INDEX_TRACE")

    monkeypatch.setenv("RTK_INDEX_SNP_MEM", str(mn - 1))
    assert api.index_snp_plan(U, 63)[0] == 0
    with pytest.raises(api.RtkError) as e:
        api.index_snp_candidates(U, 63)
    m = re.search(r"need (\d+) bytes of device memory, (\d+) are to be had", str(e.value))
    assert "rtk error %d:" % SC.RTK_ERR_DEVICE in str(e.value) and m and int(m.group(1)) == mn and int(m.group(2)) == mn - 1, str(e.value)


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the tool

@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("het_repeats", 31), ("tandem", 21), ("het_repeats", 63)])
def test_tool_in_passes(tool_sets, name, k):  # noqa: F811
    tmp, sets = tool_sets
    tag, sr = "%s_k%d_passes" % (name, k), sets[name] + ".sr.fq"
    plain = SC._tool(sr, os.path.join(tmp, tag + "_plain"), k, [], {})
    dev = SC._tool(sr, os.path.join(tmp, tag + "_dev"), k, ["--gpu"], {"RTK_INDEX_SNPS": "device", "RTK_INDEX_SNP_PASSES": "3"})
    assert plain[:2] == dev[:2], tag
    assert "rtk_index_snps: 3 passes over the key space" in dev[2] and "SNP candidates on the host threads" not in dev[2], dev[2]
