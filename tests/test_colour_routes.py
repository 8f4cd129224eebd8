"""The routes of the colour selection (chooseColors, src/Correction.cpp:215-429): counted, forced and audited.

rtk_choose_colors (csrc/hip/rtk_colours.h) asks up to three programs for the sorted id list a region's graph walk may follow: the register program of
rtk_colours.h (device only; 8-word bit vectors up to 512 ids, "small", and 64-word vectors up to 1664 ids, "wide"), rtk_choose_colors_bits (bit vectors in
scratch memory; its device branch sorts in LDS and scatters with atomicOr, its simulator branch calls std::sort) and the general program on sorted arrays, which
is the definition. Corrected bytes equal to the oracle's do not show a list that is off by one id at a quota edge, and the default order leaves the device
branch of `bits` almost without work. So the calls are counted by the program that answered (rtk_stats n_colours_small / _wide / _bits / _general), and three
knobs of rtk_knobs.h are read on every call:
  RTK_COLOURS_ROUTE=bits     the register program is skipped: `bits` answers what it can on the device too;
  RTK_COLOURS_ROUTE=general  the general program answers every call;
  RTK_COLOURS_AUDIT=1        where another program answered, the general program selects again and the two lists are compared id by id
                             (n_colours_audit_mismatch); the region goes on with the general program's list;
  RTK_TEST_COLOURS_FAULT=1   test hook under the audit: the first answer loses its largest id before the comparison, so the audit must report it.

Per set, on the 1-lane simulator and on the MI355X: the corrected reads equal the oracle's under every setting (the oracle runs once); the four route counters
sum to the same number under the default and the two forced routes; `general` leaves the other three at 0; `bits` leaves small and wide at 0 and bits above 0;
the audit finds no mismatch; the audit with the fault finds one wherever a bit-vector program answered with at least one id, and the bytes stay the oracle's.
n_colour_elem counts the ids of both runs under the audit, so counters are only compared between runs of one setting or through the sums above.

Sets: the hard genomes `all` and `family` at k = 21 (the only sets of the suite that reach the general program at volume), a ds_clean-like and a ds_small-like
set (conftest.py), a small second-pass set (the read's own qualities, k2 = 31), and `family20`: the repeat family with 20 copies that differ in 13 of 1024 bases
(instead of 7 copies and 27) at k = 21. Both bit-vector programs decline a call with more than 24 side unitigs; the other sets make one or two such calls,
`family20` makes 45 of its 1597 (counted in a throw-away simulator build; the figure moves a lot with the two settings: 21 / 22 copies at that divergence give 17 / 1).

Counted with the default setting on `all` k = 21 (seed 105), calls answered by small / wide / bits / general:
  simulator   0 / 0 / 2039 / 188
  MI355X      809 / 1230 / 0 / 188"""
import os

import pytest

import hard_genomes as hg
import test_index_build as IB
import test_pass2 as P2
from conftest import SIM_LIB, make_dataset
from oracle import oracle_py as op
from ratatosk_amd import api

ROUTE, AUDIT, FAULT = "RTK_COLOURS_ROUTE", "RTK_COLOURS_AUDIT", "RTK_TEST_COLOURS_FAULT"
SETTINGS = (("default", {}), ("bits", {ROUTE: "bits"}), ("general", {ROUTE: "general"}), ("audit", {AUDIT: "1"}), ("audit+fault", {AUDIT: "1", FAULT: "1"}))
COUNTERS = ("n_colours_small", "n_colours_wide", "n_colours_bits", "n_colours_general", "n_colours_audit_mismatch")
SEEDS = {"family": 104, "all": 105}  # the seeds of tests/test_fix_ambiguity_linked.py
SETS = ("all-k21", "family-k21", "family20-k21", "clean", "small", "pass2")


def _make(tmp, name, monkeypatch):
    """(prefix of the set's files, k, second pass?)"""
    if name in ("all-k21", "family-k21", "family20-k21"):
        kind = "family" if name.startswith("family") else "all"
        if name == "family20-k21":  # more and closer copies: more than 24 side unitigs around a region
            monkeypatch.setattr(hg, "FAMILY_COPIES", 20); monkeypatch.setattr(hg, "FAMILY_DIV_PER_1024", 13)
        pre = os.path.join(str(tmp), kind)
        hg.write_set(pre, seed=SEEDS[kind], kind=kind)
        IB._build(pre + ".sr.fq", pre, 21, [])  # the plain tool with --snps
        return pre, 21, False
    if name == "clean":  # the arguments of conftest.ds_clean
        return make_dataset(tmp, "clean", ["--seed", 1, "--ref-len", 50000, "--sr-cov", 30, "--sr-err", 0.002, "--lr-n", 10, "--lr-len", 5000, "--lr-err", 0.10]), 31, False
    if name == "small":  # the arguments of conftest.ds_small
        return make_dataset(tmp, "small", ["--seed", 11, "--ref-len", 30000, "--het", 0.004, "--repeat-frac", 0.1, "--sr-cov", 40, "--sr-err", 0.01,
                                           "--lr-n", 12, "--lr-len", 3000, "--lr-profile", "ont", "--lr-err", 0.08], ["--global-cov-factor", 1.2]), 31, False
    assert name == "pass2"  # the set of tests/test_second_strand.py's pass-2 case
    return P2._second_pass_set(tmp, "p2", ["--seed", 31, "--ref-len", 40000, "--het", 0.004, "--repeat-frac", 0.05, "--sr-cov", 40, "--sr-err", 0.005,
                                           "--lr-n", 60, "--lr-len", 3000, "--lr-profile", "ont", "--lr-err", 0.08]), 31, True


def _set_knobs(monkeypatch, env):
    for knob in (ROUTE, AUDIT, FAULT):
        monkeypatch.delenv(knob, raising=False)
    for knob, value in env.items():
        monkeypatch.setenv(knob, value)  # read on every call (rtk_knobs.h)


def _check(tmp, name, lib, monkeypatch):
    device = lib is None
    pre, k, second_pass = _make(tmp, name, monkeypatch)
    _set_knobs(monkeypatch, {})
    if second_pass:
        og, pg, seqs, quals, raws = P2._load(pre, lib)
        want = [(w[0], w[1]) for w in og.correct_batch2(seqs, quals, raws, og.opts(long_read_correct=1), threads=8)]
        opts = dict(long_read_correct=1)
    else:
        fa, rt = pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k
        reads = op.read_fastq(pre + ".lr.fq")
        seqs, quals, raws = [r[1] for r in reads], [r[2] for r in reads], None
        want = [(w[0], w[1]) for w in op.Graph(fa, rt, k).correct_batch(seqs, quals, threads=8)[0]]  # once per set
        pg, opts = api.Graph(fa, rt, k, device=0, lib_path=lib), {}
    seen = {}
    for setting, env in SETTINGS:
        _set_knobs(monkeypatch, env)
        b = api.Batch(pg, seqs, quals, raw=raws)
        b.run(pg.opts(**opts))
        got, st = b.fetch(), b.stats()
        b.close()
        seen[setting] = c = dict((n, st[n]) for n in COUNTERS)
        print("%s %s %s: %d reads, %d regions; colour selections answered by small %d wide %d bits %d general %d, audit mismatches %d" % (
            "MI355X" if device else "simulator", name, setting, len(seqs), st["n_regions"], c[COUNTERS[0]], c[COUNTERS[1]], c[COUNTERS[2]], c[COUNTERS[3]], c[COUNTERS[4]]))
        assert [(g[0], g[1]) for g in got] == want, "%s: %d reads differ from the oracle" % (setting, sum(1 for g, w in zip(got, want) if (g[0], g[1]) != w))
    _set_knobs(monkeypatch, {})
    total = lambda c: sum(c[n] for n in COUNTERS[:4])
    d, bits, gen, audit, fault = (seen[s] for s, _ in SETTINGS)
    assert total(d) == total(bits) == total(gen) and total(d) > 0
    assert (gen["n_colours_small"], gen["n_colours_wide"], gen["n_colours_bits"]) == (0, 0, 0)
    assert (bits["n_colours_small"], bits["n_colours_wide"]) == (0, 0) and bits["n_colours_bits"] > 0
    assert all(seen[s]["n_colours_audit_mismatch"] == 0 for s in ("default", "bits", "general", "audit"))
    if not device:
        assert all(seen[s]["n_colours_small"] == 0 and seen[s]["n_colours_wide"] == 0 for s, _ in SETTINGS)  # the simulator has neither
    if device or d["n_colours_bits"] > 0:
        assert fault["n_colours_audit_mismatch"] > 0, "the audit did not notice a first answer without its largest id"
    if name == "all-k21":
        if device:
            assert d["n_colours_small"] >= 100 and d["n_colours_wide"] >= 100 and d["n_colours_general"] >= 100, d
        else:
            assert d["n_colours_bits"] >= 100 and d["n_colours_general"] >= 100, d  # (so the fault assertion above is never vacuous)
    return seen


@pytest.mark.parametrize("name", SETS)
def test_sim_routes(tmp_path, monkeypatch, name):
    _check(tmp_path, name, SIM_LIB, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gpu_routes(tmp_path, monkeypatch, name):
    _check(tmp_path, name, None, monkeypatch)
