"""The trim and the consensus of a gap region share one sweep (csrc/hip/rtk_myers_distance.h, rtk_myers_shw_by_column; csrc/hip/rtk_region_align.h, rtk_trim_by_column).

The trim's SHW alignment of (raw, corrected) is read off the LAST COLUMN of one NW sweep of (corrected, raw): equality is symmetric, so the SHW matrix is the
transpose of that NW matrix. Row i of a stored sweep only depends on rows <= i, so the same table walked from row keep gives the consensus's NW path of
(corrected[0, keep), raw). The stage entry rtk_myers_batch holds both routes to the reference's golden vectors and to the oracle through two test-only modes:
3 (SHW by column: distance, number of end locations, the first and the last one) and 4 (NW path of query[0, k) walked from row k of the sweep of the whole
query). Each test also counts the problems the route took and the ones it left to the calls it replaces (rtk_myers_column_last_routes): a route that took
nothing would otherwise pass on the fallback's results. The region-level tests check the corrected reads against the oracle and the route counters of
rtk_stats. The 1-lane simulator runs the same restatement through the generic pass and the column read-out; the gpu tests run the wave sweeps."""
import os
import random
import subprocess

import pytest

from conftest import BIN, SIM_LIB, golden_rows
from oracle import oracle_py as op
from ratatosk_amd import api

TB_CAP_WORDS = 4 * 52429 + 64  # traceback table of a wave of the stage entry (rtk_device.hip, rtk_myers_batch_waves)


def _acgt(s):
    return len(s) > 0 and set(s) <= set("ACGT")


def _words(n):
    return (n + 63) // 64


def _in_memory(m, n):
    """the in-memory traceback branch of obtainAlignment (edlib.cpp:1191-1193) for an m x n NW problem"""
    return (2 * 8 + 4) * _words(m) * n + 8 * n < 1024 * 1024


def _shw_takes_column(q, t):
    """mode 3 sweeps NW(t, q): t is the swept query (at most 4096 characters), q the swept target (A/C/G/T only)"""
    return len(t) > 0 and len(t) <= 4096 and _acgt(q)


def _prefix_takes_column(q, k, t):
    """mode 4 stores the sweep of the whole query q against t and walks it from row k"""
    return (k > 0 and len(q) <= 4096 and _acgt(t) and 4 * _words(len(q)) * len(t) <= TB_CAP_WORDS and _in_memory(k, len(t)))


def _expect_locs(locs):
    """what mode 3 reports of a list of end locations: as many entries, the first and the last one (the others are not listed)"""
    return len(locs), (locs[0] if locs else None), (locs[-1] if locs else None)


def _check_shw(lib, qs, ts, want):
    """want: [(distance, end locations)] of edlibAlign(q, t, SHW), k = -1"""
    res = api.myers_batch(qs, ts, [-1] * len(qs), [api.MODE_SHW_BY_COLUMN] * len(qs), want_path=False, lib_path=lib)
    for q, t, (d, locs), (gd, glocs, _) in zip(qs, ts, want, res):
        assert gd == d, (q, t, gd, d)
        got = (len(glocs), glocs[0] if glocs else None, glocs[-1] if glocs else None)
        assert got == _expect_locs(locs), (q, t, got, locs)
    col, fb = api.myers_column_last_routes(lib)
    must = sum(1 for q, t in zip(qs, ts) if _shw_takes_column(q, t))
    assert (col, fb) == (must, len(qs) - must)
    return col, fb


def _check_prefix(lib, qs, ks, ts, want):
    """want: [(distance, cigar)] of edlibAlign(q[0, k), t, NW, path)"""
    res = api.myers_batch(qs, ts, ks, [api.MODE_NW_PREFIX] * len(qs), want_path=True, lib_path=lib)
    for q, k, t, (d, cig), (gd, glocs, gcig) in zip(qs, ks, ts, want, res):
        assert (gd, gcig) == (d, cig), (q[:k], t, gd, d)
        assert glocs == [len(t) - 1]
    col, fb = api.myers_column_last_routes(lib)
    must = sum(1 for q, k, t in zip(qs, ks, ts) if _prefix_takes_column(q, k, t))
    assert (col, fb) == (must, len(qs) - must)
    return col, fb


def _golden_shw(lib):
    """every SHW row of the golden vectors (with or without a path; a bounded row's distance is -1 above its k)"""
    rows = [r for r in golden_rows() if r["mode"] == 1]
    res = api.myers_batch([r["q"] for r in rows], [r["t"] for r in rows], [-1] * len(rows), [api.MODE_SHW_BY_COLUMN] * len(rows), want_path=False, lib_path=lib)
    for r, (d, locs, _) in zip(rows, res):
        if r["d"] < 0:
            assert d > r["k"], (r["q"], r["t"], r["k"], d)
        else:
            assert d == r["d"], (r["q"], r["t"], r["d"], d)
            assert (len(locs), locs[0] if locs else None, locs[-1] if locs else None) == _expect_locs(r["locs"]), (r["q"], r["t"], locs, r["locs"])
    col, fb = api.myers_column_last_routes(lib)
    must = sum(1 for r in rows if _shw_takes_column(r["q"], r["t"]))
    assert (col, fb) == (must, len(rows) - must)
    assert col > 0
    return col, fb


def _golden_prefix(lib):
    """every NW path row of the golden vectors, its query followed by a seeded random suffix and the path walked from row |q|"""
    rnd = random.Random(5)
    rows = [r for r in golden_rows() if r["mode"] == 0 and r["path"] and r["d"] >= 0]
    qs = [r["q"] + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 200))) for r in rows]
    ks = [len(r["q"]) for r in rows]
    col, fb = _check_prefix(lib, qs, ks, [r["t"] for r in rows], [(r["d"], r["cigar"]) for r in rows])
    in_memory = sum(1 for r in rows if len(r["q"]) > 0 and len(r["t"]) > 0 and _in_memory(len(r["q"]), len(r["t"])))
    assert col > 0 and in_memory > 0
    return col, fb


def _random_pairs(seed, n, big=False):
    """(raw, corrected) pairs as the trim sees them: corrected = raw with edits, IUPAC codes and N now and then, lengths 1-600 (multiples of 64 included);
    big: corrected strings above 2048 (the 64-bit sweep) and above 4096 (the fallback)"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        if big:
            m = rnd.choice((2049, 2100, 3000, 4095, 4096, 4097, 5000))
        else:
            m = rnd.choice((1, 2, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 256, 300, 320, 448, 511, 512, 513, 599, 600))
        raw = "".join(rnd.choice("ACGT") for _ in range(m))
        if i % 9 == 0:
            raw = raw[:m // 2] + "N" + raw[m // 2 + 1:]  # a raw byte the sweep's target cannot hold: the fallback
        corr = []
        for c in raw:
            x = rnd.random()
            if x < 0.03:
                continue
            if x < 0.06:
                corr.append(rnd.choice("ACGT"))
            elif x < 0.08 and i % 3 == 0:
                corr.append(rnd.choice("MRSVWYHKDBN"))
                continue
            corr.append(c)
        corr = "".join(corr)
        if i % 4 == 1:  # the corrected string runs on past the raw region, as before a trim that shortens it
            corr += "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 80)))
        if not corr:
            corr = "A"
        out.append((raw, corr))
    return out


def _random_shw(lib, seed, n, big=False):
    pairs = _random_pairs(seed, n, big)
    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    want = [op.myers(q, t, -1, 1)[:2] for q, t in zip(qs, ts)]
    return _check_shw(lib, qs, ts, want)


def _random_prefix(lib, seed, n, big=False):
    """NW(corr[0, k), raw) walked from row k of the sweep of all of corr: corr carries IUPAC codes and N, raw now and then N. big: the raw region is cut to
    at most 600 characters, so that the table of a corrected string above 2048 characters fits the stage entry's traceback table"""
    pairs = _random_pairs(seed, n, big)
    rnd = random.Random(seed + 1)
    qs, ts = [p[1] for p in pairs], [p[0] for p in pairs]
    if big:
        ts = [t[:rnd.randrange(1, 601)] for t in ts]
    ks = [rnd.randrange(0, len(q) + 1) if i % 5 else len(q) for i, q in enumerate(qs)]
    want = []
    for q, k, t in zip(qs, ks, ts):
        d, _, cig = op.myers(q[:k], t, -1, 0, True)
        want.append((d, cig))
    return _check_prefix(lib, qs, ks, ts, want)


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
def test_sim_shw_by_column_golden():
    _golden_shw(SIM_LIB)


def test_sim_nw_prefix_walk_golden():
    _golden_prefix(SIM_LIB)


def test_sim_column_routes_random_vs_oracle():
    col, fb = _random_shw(SIM_LIB, 1, 300)
    assert col > 0 and fb > 0
    col, fb = _random_prefix(SIM_LIB, 2, 300)
    assert col > 0 and fb > 0
    col, fb = _random_shw(SIM_LIB, 3, 14, big=True)
    assert col > 0 and fb > 0
    col, fb = _random_prefix(SIM_LIB, 4, 14, big=True)
    assert col > 0 and fb > 0


def _correct(prefix, n, lib, k=31):
    fa, rt = prefix + ".index.k%d.fasta.gz" % k, prefix + ".index.k%d.rtsk" % k
    pg = api.Graph(fa, rt, k, device=0, lib_path=lib)
    reads = op.read_fastq(prefix + ".lr.fq")
    reads = reads[:n] if n else reads
    seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
    b = api.Batch(pg, seqs, quals)
    b.run(pg.opts())
    return b.fetch(), b.stats(), seqs, quals


def _check_region_routes(st):
    assert st["n_trim_stored"] > 0 and st["n_trim_column"] > 0
    assert st["n_consensus_resumed"] > 0
    assert st["n_consensus_resumed"] <= st["n_trim_stored"]  # a resumed alignment comes from a stored trim of the same region


def test_sim_region_routes_and_bytes(ds_snps, ds_small):
    """The corrected reads equal the oracle's while the trims go by column and the consensus calls resume the forward alignment."""
    for pre, n in ((ds_snps, 24), (ds_small, 12)):
        got, st, seqs, quals = _correct(pre, n, SIM_LIB)
        og = op.Graph(pre + ".index.k31.fasta.gz", pre + ".index.k31.rtsk", 31)
        want, _ = og.correct_batch(seqs, quals, threads=4)
        assert got == want, "%d reads differ from the oracle" % sum(1 for a, b in zip(got, want) if a != b)
        _check_region_routes(st)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_shw_by_column_golden():
    _golden_shw(None)


@pytest.mark.gpu
def test_gpu_nw_prefix_walk_golden():
    _golden_prefix(None)


@pytest.mark.gpu
def test_gpu_column_routes_random_vs_oracle():
    col, fb = _random_shw(None, 11, 1500)
    assert col > 0 and fb > 0
    col, fb = _random_prefix(None, 12, 1500)
    assert col > 0 and fb > 0
    col, fb = _random_shw(None, 13, 60, big=True)
    assert col > 0 and fb > 0
    col, fb = _random_prefix(None, 14, 60, big=True)
    assert col > 0 and fb > 0


@pytest.mark.gpu
def test_gpu_consensus_resumed_share(tmp_path):
    """The issue's set (1 Mb diploid reference, 4x ONT-profile reads of 8 kb, index of 30x simulated short reads with SNP annotations): at least 95 % of the
    consensus calls take the forward strand's alignment from the stored sweep of its trim. On the parent's simulator build, 5 088 of its 5 153 consensus calls
    (98.7 %) had a raw region and a forward string of A/C/G/T only."""
    pre = str(tmp_path / "P")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "1000000", "--het", "0.001", "--sr-cov", "0", "--lr-cov", "4",
                           "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.07"], stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(BIN, "rtk_build_index"), "-s", "sample:%s.ref.fa?cov=30&len=150&insert=500&err=0.005&seed=2" % pre, "-o", pre, "--snps"],
                          stderr=subprocess.DEVNULL)
    _, st, _, _ = _correct(pre, 0, None)
    _check_region_routes(st)
    res, swept = st["n_consensus_resumed"], st["n_consensus_swept"]
    print("consensus calls: resumed %d swept %d (%.4f); trims stored %d by column %d by the distance call %d" % (
        res, swept, res / max(1, res + swept), st["n_trim_stored"], st["n_trim_column"], st["n_trim_fallback"]))
    assert res >= 0.95 * (res + swept), (res, swept)
