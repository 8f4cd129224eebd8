"""fixAmbiguity's linked-allele searches are skipped when they cannot count (csrc/hip/rtk_ambiguity.h, rtk_fix_ambiguity).

For every entry of the safe set that the alignment has decided, the reference looks the up to k k-mers around it up in the graph and collects the alleles of the
other annotated positions of the unitigs it meets (src/Alignment.cpp:711-770) -- but only for positions whose own entry is still undecided (:755-759). When no
entry is undecided no search of the call can append anything, so the region program leaves them out. RTK_FA_LINKED_ALWAYS=1 runs them all, as the reference does.

Checked per set, on the 1-lane simulator and on the MI355X: the corrected reads equal the oracle's with the knob and without; searches run + skipped is the same
number under both settings and with the knob nothing is skipped; the searches produce the same number of entries under both settings (the skipped ones produce
none). On the 1 Mb set (1 Mb diploid reference at 0.1 % het, 4x ONT-profile reads of 8 kb, index of 30x simulated short reads with SNP annotations: the recipe of
profiles/trim_consensus_sweep.txt) at least 90 % of the searches are skipped, and some still run and produce entries, so the kept route is exercised.
Counted on that set, all 415 reads, on the simulator: 10 689 searches, 10 269 skipped (0.961), 420 run, 52 entries. The 0.9 is the condition: the rule is
only worth having while nearly every call has a single low-confidence position."""
import os
import subprocess

import pytest

import hard_genomes as hg
import test_index_build as IB
from conftest import BIN, SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

KNOB = "RTK_FA_LINKED_ALWAYS"
HARD = (("homopolymer", 101), ("microsatellite", 102), ("inverted", 103), ("family", 104), ("all", 105))  # every kind plants het substitutions in its flanks


def _one_mb_set(tmp):
    pre = os.path.join(str(tmp), "P")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "1000000", "--het", "0.001", "--sr-cov", "0", "--lr-cov", "4",
                           "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.07"], stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(BIN, "rtk_build_index"), "-s", "sample:%s.ref.fa?cov=30&len=150&insert=500&err=0.005&seed=2" % pre, "-o", pre, "--snps"],
                          stderr=subprocess.DEVNULL)
    return pre


def _hard_set(tmp, kind, seed):
    pre = os.path.join(str(tmp), kind)
    hg.write_set(pre, seed=seed, kind=kind)
    IB._build(pre + ".sr.fq", pre, 31, [])  # the plain tool with --snps
    return pre


def _run(pg, seqs, quals):
    b = api.Batch(pg, seqs, quals)
    b.run(pg.opts())
    return b.fetch(), b.stats()


def _check(pre, lib, monkeypatch):
    """both settings against the oracle and against each other; returns (run, skipped, entries) of the default setting"""
    fa, rt = pre + ".index.k31.fasta.gz", pre + ".index.k31.rtsk"
    reads = op.read_fastq(pre + ".lr.fq")
    seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
    want, _ = op.Graph(fa, rt, 31).correct_batch(seqs, quals, threads=4)
    pg = api.Graph(fa, rt, 31, device=0, lib_path=lib)
    monkeypatch.delenv(KNOB, raising=False)
    got, st = _run(pg, seqs, quals)
    monkeypatch.setenv(KNOB, "1")  # read on every call (rtk_knobs.h)
    got_all, st_all = _run(pg, seqs, quals)
    monkeypatch.delenv(KNOB)
    run, skipped, entries = st["n_fa_linked_run"], st["n_fa_linked_skipped"], st["n_fa_linked_entries"]
    run_all, skipped_all, entries_all = st_all["n_fa_linked_run"], st_all["n_fa_linked_skipped"], st_all["n_fa_linked_entries"]
    print("%s: %d reads; searches run %d skipped %d (%.4f) entries %d; with %s=1: run %d skipped %d entries %d" % (
        os.path.basename(pre), len(reads), run, skipped, skipped / max(1, run + skipped), entries, KNOB, run_all, skipped_all, entries_all))
    assert got == want, "%d reads differ from the oracle" % sum(1 for a, b in zip(got, want) if a != b)
    assert got_all == want, "%d reads differ from the oracle with %s=1" % (sum(1 for a, b in zip(got_all, want) if a != b), KNOB)
    assert run + skipped == run_all + skipped_all
    assert skipped_all == 0
    assert entries == entries_all
    return run, skipped, entries


def _check_one_mb(tmp, lib, monkeypatch):
    run, skipped, entries = _check(_one_mb_set(tmp), lib, monkeypatch)
    assert skipped >= 0.9 * (run + skipped), (run, skipped)
    assert run > 0 and entries > 0, (run, entries)


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
def test_sim_one_mb_set(tmp_path, monkeypatch):
    _check_one_mb(tmp_path, SIM_LIB, monkeypatch)


@pytest.mark.parametrize("kind,seed", HARD, ids=[h[0] for h in HARD])
def test_sim_hard_genomes(tmp_path, monkeypatch, kind, seed):
    _check(_hard_set(tmp_path, kind, seed), SIM_LIB, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_one_mb_set(tmp_path, monkeypatch):
    _check_one_mb(tmp_path, None, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", HARD, ids=[h[0] for h in HARD])
def test_gpu_hard_genomes(tmp_path, monkeypatch, kind, seed):
    _check(_hard_set(tmp_path, kind, seed), None, monkeypatch)
