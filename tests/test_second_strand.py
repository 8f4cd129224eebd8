"""A gap region skips its second strand where the forward result decides the bytes alone (csrc/hip/rtk_region.h, rtk_strand2_skippable).

A gap region that its forward strand does not settle alone is corrected again on the reverse complement and the two results are merged (generateConsensus,
src/Correction.cpp:859-915). When the forward strand corrected every old position the merge hands the forward strings back, unless the second strand comes back
`is_corrected` or one of the conditions R2 .. R4 of the rule fails; the region program checks R1 .. R5 from the forward result, the read and the graph and then runs
neither the second strand nor the consensus. RTK_STRAND2_ALWAYS=1 runs every second strand, as the reference does; RTK_STRAND2_AUDIT=1 runs the full route where
the rule says skip, emits its result and counts the regions whose bytes differ from the forward strings.

Checked per set, on the 1-lane simulator and on the MI355X, under the three settings: the corrected reads equal the oracle's (which runs both strands); second
strands run + skipped is the same number; ALWAYS skips none; the audit finds no mismatch; some second strands still run, so the exceptions of the rule stay
exercised (every set holds second strands that come back `is_corrected`; `all` at k = 21 holds a region with a full forward bitmap that emits the reverse
strand's string). On the 1 Mb set (the generator arguments of tests/test_fix_ambiguity_linked.py) at least 90 % are skipped: the condition below which the rule
is not worth its code. Counted on that set on the simulator: 10 480 second strands, 10 419 skipped (0.994), 61 run. Pass 2 runs the same program with the read's
own qualities (`lrc`): one small set built like those of tests/test_pass2.py, oracle bytes under the default and under the audit."""
import os
import subprocess

import pytest

import hard_genomes as hg
import test_index_build as IB
import test_pass2 as P2
from conftest import BIN, SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

ALWAYS, AUDIT = "RTK_STRAND2_ALWAYS", "RTK_STRAND2_AUDIT"
SETTINGS = ((), (ALWAYS,), (AUDIT,))
SEEDS = {"homopolymer": 101, "microsatellite": 102, "family": 104, "all": 105}  # the seeds of tests/test_fix_ambiguity_linked.py
HARD = [(kind, k) for kind in ("all", "microsatellite", "homopolymer", "family") for k in (31, 21)]


def _one_mb_set(tmp):
    pre = os.path.join(str(tmp), "P")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "1000000", "--het", "0.001", "--sr-cov", "0", "--lr-cov", "4",
                           "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.07"], stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(BIN, "rtk_build_index"), "-s", "sample:%s.ref.fa?cov=30&len=150&insert=500&err=0.005&seed=2" % pre, "-o", pre, "--snps"],
                          stderr=subprocess.DEVNULL)
    return pre


def _hard_set(tmp, kind, k):
    pre = os.path.join(str(tmp), kind)
    hg.write_set(pre, seed=SEEDS[kind], kind=kind)
    IB._build(pre + ".sr.fq", pre, k, [])  # the plain tool with --snps
    return pre


def _set_knobs(monkeypatch, setting):
    for knob in (ALWAYS, AUDIT):
        monkeypatch.delenv(knob, raising=False)
    for knob in setting:
        monkeypatch.setenv(knob, "1")  # read on every call (rtk_knobs.h)


def _counts(st):
    return st["n_strand2_run"], st["n_strand2_skipped"], st["n_strand2_audit_mismatch"]


def _check(pre, k, lib, monkeypatch):
    """the three settings against the oracle and against each other; returns (run, skipped) of the default setting"""
    fa, rt = pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k
    reads = op.read_fastq(pre + ".lr.fq")
    seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
    want, _ = op.Graph(fa, rt, k).correct_batch(seqs, quals, threads=8)  # once per set: the oracle runs both strands of every region
    pg = api.Graph(fa, rt, k, device=0, lib_path=lib)
    seen = {}
    for setting in SETTINGS:
        _set_knobs(monkeypatch, setting)
        b = api.Batch(pg, seqs, quals)
        b.run(pg.opts())
        got, st = b.fetch(), b.stats()
        run, skipped, mismatch = seen[setting] = _counts(st)
        print("%s k=%d %s: %d reads; second strands run %d skipped %d (%.4f) audit mismatches %d; n_expand %d n_align_cells %d" % (
            os.path.basename(pre), k, "+".join(setting) or "default", len(reads), run, skipped, skipped / max(1, run + skipped), mismatch, st["n_expand"], st["n_align_cells"]))
        assert got == want, "%d reads differ from the oracle (%s)" % (sum(1 for a, b_ in zip(got, want) if a != b_), "+".join(setting) or "default")
    _set_knobs(monkeypatch, ())
    (run, skipped, mismatch), (run_all, skipped_all, mismatch_all), (run_au, skipped_au, mismatch_au) = (seen[s] for s in SETTINGS)
    assert run + skipped == run_all + skipped_all == run_au + skipped_au
    assert skipped_all == 0
    assert (run_au, skipped_au) == (run, skipped)  # the audit counts the rule's verdicts (and runs both kinds)
    assert mismatch == 0 and mismatch_all == 0 and mismatch_au == 0
    assert run > 0, "no second strand runs any more: the exceptions of the rule are not exercised"
    return run, skipped


def _check_one_mb(tmp, lib, monkeypatch):
    run, skipped = _check(_one_mb_set(tmp), 31, lib, monkeypatch)
    assert skipped >= 0.9 * (run + skipped), (run, skipped)


def _check_pass2(tmp, lib, monkeypatch):
    """pass 2 (`lrc`, the read's own qualities): the set of tests/test_pass2.py's ds_pass2, oracle bytes under the default and under the audit"""
    pre = P2._second_pass_set(tmp, "p2", ["--seed", 31, "--ref-len", 40000, "--het", 0.004, "--repeat-frac", 0.05, "--sr-cov", 40, "--sr-err", 0.005,
                                          "--lr-n", 60, "--lr-len", 3000, "--lr-profile", "ont", "--lr-err", 0.08])
    og, pg, seqs, quals, raws = P2._load(pre, lib)
    want = og.correct_batch2(seqs, quals, raws, og.opts(long_read_correct=1), threads=8)
    assert sum(1 for (s, _), s0 in zip(want, seqs) if s != s0) > 0  # the pass has something to do
    seen = {}
    for setting in ((), (AUDIT,)):
        _set_knobs(monkeypatch, setting)
        b = api.Batch(pg, seqs, quals, raw=raws)
        b.run(pg.opts(long_read_correct=1))
        got, st = b.fetch(), b.stats()
        seen[setting] = _counts(st)
        print("pass 2 %s: %d reads; second strands run %d skipped %d audit mismatches %d" % (("+".join(setting) or "default", len(seqs)) + seen[setting]))
        assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want], "+".join(setting) or "default"
    _set_knobs(monkeypatch, ())
    assert seen[()] == seen[(AUDIT,)] and seen[()][2] == 0
    assert seen[()][1] > 0, "pass 2 skipped no second strand: the rule is not exercised there"


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
def test_sim_one_mb_set(tmp_path, monkeypatch):
    _check_one_mb(tmp_path, SIM_LIB, monkeypatch)


@pytest.mark.parametrize("kind,k", HARD, ids=["%s-k%d" % h for h in HARD])
def test_sim_hard_genomes(tmp_path, monkeypatch, kind, k):
    _check(_hard_set(tmp_path, kind, k), k, SIM_LIB, monkeypatch)


def test_sim_pass2(tmp_path, monkeypatch):
    _check_pass2(tmp_path, SIM_LIB, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_one_mb_set(tmp_path, monkeypatch):
    _check_one_mb(tmp_path, None, monkeypatch)


@pytest.mark.gpu
def test_gpu_all_k21(tmp_path, monkeypatch):
    _check(_hard_set(tmp_path, "all", 21), 21, None, monkeypatch)


@pytest.mark.gpu
def test_gpu_pass2(tmp_path, monkeypatch):
    _check_pass2(tmp_path, None, monkeypatch)
