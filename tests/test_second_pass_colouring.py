"""Colouring the index of the second pass by base confidence and read length ([A14], DESIGN.md section 4: rtk_build_index --colour-reads with --colour-min-conf /
--colour-max-qual / --colour-min-len, `Ratatosk correct -s ... -M -C`, rtk_index_colour_chunk_q). The oracle needs no tolerance: the filtered index equals, byte for
byte, the index that the code path WITHOUT the options builds from a pre-masked copy of the colouring file written here in Python (masked bases spelled N, a read
below the minimum length replaced by the one-base record N / !, so that every read keeps its id). The four variants -- no filter, quality only, length only, both --
must give four different .rtsk files on the test's own input, or a filter that does nothing would pass."""
import gzip
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BIN, ROOT, SIM_LIB
import second_pass_colouring_restatement as rule

TOOL = os.path.join(BIN, "rtk_build_index")
EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
LIB = os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so")
SIM_ARGS = ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--tandem", "5", "--sr-cov", "40", "--sr-err", "0.01",
            "--lr-n", "12", "--lr-len", "3000", "--lr-profile", "ont", "--lr-err", "0.01"]
MIN_CONF, MIN_LEN = 0.5, 1000
Q_MIN = rule.c_min(MIN_CONF)  # 53, '5'
FILTER = ["--colour-min-conf", str(MIN_CONF), "--colour-min-len", str(MIN_LEN)]
GPU_STEP_TIMEOUT = 300  # seconds, every child process that opens the GPU
SMALL_JOB = {"RTK_INDEX_EVENTS": "4000000"}  # room for 4 M events instead of 60 % of the device memory: opening a colouring job then takes no seconds


def test_c_min_restated():
    """the formula of the issue, worked out here: (unsigned char)(min(M, 1.0) * (Q - 1) + 34.0)"""
    assert (rule.c_min(0), rule.c_min(0.5), rule.c_min(1)) == (34, 53, 73) == (ord('"'), ord("5"), ord("I"))
    for m, q in itertools.product((0, 0.5, 0.9, 1, 1.5), (40, 60)):
        want = int(min(m, 1.0) * (q - 1) + 34.0) % 256
        assert rule.c_min(m, q) == want, (m, q)
    assert rule.c_min(0.9, 40) == 69 and rule.c_min(1.5, 60) == rule.c_min(1, 60) == 93 and rule.c_min(0.9, 60) == 87


class Data:
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """raw.fq: the long reads of the 30 kb set at 1 % error, some cut to MIN_LEN - 1, MIN_LEN, k - 1 and k bases (k = 63 and 31), the qualities rewritten in runs around
    the threshold; the pre-masked copies of it for every variant of the filter, as FASTQ, gzipped and as FASTA."""
    d = Data()
    d.tmp = str(tmp_path_factory.mktemp("second_pass_colouring"))
    pre = os.path.join(d.tmp, "s")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + SIM_ARGS, stderr=subprocess.DEVNULL)
    d.sr = pre + ".sr.fq"
    recs = rule.read_fastq(pre + ".lr.fq")
    assert len(recs) == 12 and min(len(r[1]) for r in recs) > MIN_LEN
    rng = rule.seeded(5)
    cuts = {1: MIN_LEN - 1, 3: MIN_LEN, 5: 62, 6: 63, 8: 30, 9: 31}
    d.raw = []
    for i, (name, seq, _) in enumerate(recs):
        seq = seq[:cuts.get(i, len(seq))]
        d.raw.append((name, seq, rule.qualities_in_runs(len(seq), Q_MIN, rng)))
    d.variants = {"none": (0, 0), "quality": (Q_MIN, 0), "length": (0, MIN_LEN), "both": (Q_MIN, MIN_LEN)}
    d.options = {"none": [], "quality": FILTER[:2], "length": FILTER[2:], "both": FILTER}
    d.fq, d.gz, d.fa = {}, {}, {}
    for v, (q_min, min_len) in d.variants.items():
        r = d.raw if v == "none" else rule.premask(d.raw, q_min, min_len)
        d.fq[v], d.gz[v], d.fa[v] = (os.path.join(d.tmp, "%s.%s" % (v, ext)) for ext in ("fq", "fq.gz", "fa"))
        for path, opener, text in ((d.fq[v], open, rule.fastq_text(r)), (d.gz[v], gzip.open, rule.fastq_text(r)), (d.fa[v], open, rule.fasta_text(r))):
            with opener(path, "wt") as f:
                f.write(text)
    masked = sum(ord(q) < Q_MIN for _, _, qual in d.raw for q in qual)
    assert masked > 1000 and sum(len(r[1]) < MIN_LEN for r in d.raw) == 5
    d.n = itertools.count()
    return d


def _tool(args, env=None, timeout=None):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})), timeout=timeout)


def _build(d, k, colour, extra, timeout=None, env=None):
    """(.rtsk bytes, inflated unitig FASTA, trace)"""
    out = os.path.join(d.tmp, "i%d" % next(d.n))
    r = _tool(["-s", d.sr, "-o", out, "-k", str(k), "--colour-reads", colour] + extra, timeout=timeout, env=env)
    assert r.returncode == 0, (extra, r.stderr)
    return open(out + ".index.k%d.rtsk" % k, "rb").read(), gzip.open(out + ".index.k%d.fasta.gz" % k, "rb").read(), r.stderr


@pytest.mark.parametrize("k", [63, 31])
def test_filtered_index_is_the_unfiltered_index_of_the_premasked_file(data, k):
    """plain (the reader route) and --fast (the range route on a plain file), on FASTQ: every variant equals its pre-masked twin built without the options; the four
    variants differ; the trace counts the reads the length rule left out"""
    rtsk = {}
    for v in ("none", "quality", "length", "both"):
        for mode in ([], ["--fast"]):
            got = _build(data, k, data.fq["none"], data.options[v] + mode)
            want = _build(data, k, data.fq[v], mode)
            assert got[:2] == want[:2], (v, mode)
            assert rtsk.setdefault(v, got[0]) == got[0], (v, "plain and --fast differ")
            if data.variants[v][1]:
                assert "5 colouring reads shorter than %d left out" % MIN_LEN in got[2], got[2]
            elif v == "quality":
                assert "quality byte below %d masked" % Q_MIN in got[2] and "left out" not in got[2], got[2]
            else:
                assert "colour filter" not in got[2]
    assert len(set(rtsk.values())) == 4, "the four variants of the filter do not give four different .rtsk files"


@pytest.mark.parametrize("k", [63, 31])
def test_gzip_input_and_snps(data, k):
    """gzip input takes the reader route also with --fast; --snps on top"""
    want = _build(data, k, data.gz["both"], ["--snps"])
    assert want[:2] == _build(data, k, data.fq["both"], ["--snps", "--fast"])[:2]
    for mode in ([], ["--fast"]):
        assert _build(data, k, data.gz["none"], FILTER + ["--snps"] + mode)[:2] == want[:2], mode
    assert _build(data, k, data.fq["none"], FILTER + ["--snps", "--fast"])[:2] == want[:2]
    assert _build(data, k, data.gz["none"], ["--snps"])[0] != want[0]


def test_max_qual_moves_the_threshold(data):
    """--colour-max-qual 60 with M = 19 / 59 is the threshold 53 of M = 0.5 at Q = 40 ... and M = 0.5 at Q = 60 is another one"""
    assert rule.c_min(0.33, 60) == Q_MIN and rule.c_min(0.5, 60) == 63
    want = _build(data, 63, data.fq["quality"], [])[:2]
    assert _build(data, 63, data.fq["none"], ["--colour-min-conf", "0.33", "--colour-max-qual", "60"])[:2] == want
    other = _build(data, 63, data.fq["none"], ["--colour-min-conf", "0.5", "--colour-max-qual", "60", "--fast"])
    assert other[0] != want[0] and "quality byte below 63 masked" in other[2]


def test_options_need_colour_reads_and_a_valid_confidence(data, tmp_path):
    out = str(tmp_path / "o")
    for opt in (["--colour-min-conf", "0.5"], ["--colour-max-qual", "40"], ["--colour-min-len", "100"]):
        r = _tool(["-s", data.sr, "-o", out] + opt)
        assert r.returncode == 2 and opt[0] + " without --colour-reads" in r.stderr, r.stderr
    for m in ("1.5", "-0.1", "x", "nan"):
        r = _tool(["-s", data.sr, "-o", out, "--colour-reads", data.fq["none"], "--colour-min-conf", m])
        assert r.returncode == 2 and "--colour-min-conf" in r.stderr, (m, r.stderr)
    assert os.listdir(str(tmp_path)) == []
    usage = _tool([]).stderr
    for opt in ("--colour-min-conf", "--colour-max-qual", "--colour-min-len"):
        assert opt in usage


def test_fasta_colour_file(data, tmp_path):
    """no qualities: refused under a confidence threshold, the file named, the same message on both routes; the length rule alone takes it"""
    msgs = set()
    for mode in ([], ["--fast"]):
        r = _tool(["-s", data.sr, "-o", str(tmp_path / "o"), "-k", "63", "--colour-reads", data.fa["none"]] + FILTER + mode)
        assert r.returncode not in (0, 2) and r.returncode > 0, r.stderr
        line = [l for l in r.stderr.split("\n") if "--colour-min-conf" in l]
        assert len(line) == 1 and data.fa["none"] in line[0] and "quality" in line[0], r.stderr
        msgs.add(line[0])
        want = _build(data, 63, data.fa["length"], mode)
        assert _build(data, 63, data.fa["none"], FILTER[2:] + mode)[:2] == want[:2]
        assert want[:2] == _build(data, 63, data.fq["length"], mode)[:2]
    assert len(msgs) == 1


def test_subsampled_colours_with_the_filter(data):
    a = _build(data, 63, data.fq["none"], FILTER + ["--subsample-colours"])
    b = _build(data, 63, data.fq["none"], FILTER + ["--subsample-colours", "--fast"])
    assert a[:2] == b[:2]
    assert a[:2] == _build(data, 63, data.fq["both"], ["--subsample-colours", "--fast"])[:2]


def test_header_and_libraries_have_the_entry():
    import ctypes
    txt = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    assert re.search(r"\bint\s+rtk_index_colour_chunk_q\s*\(", txt) and re.search(r"#define\s+RTK_API_REVISION\s+10\b", txt)
    for path in (LIB, SIM_LIB):
        assert hasattr(ctypes.CDLL(path), "rtk_index_colour_chunk_q"), path
    from ratatosk_amd import api
    assert callable(api.index_colour_reads)
    with pytest.raises(ValueError):
        api.index_colour_reads(["ACGTA"], 3, ["ACGTA", "ACGTA"], quals=["IIIII", None], q_min=40)


@pytest.mark.parametrize("exe", [EXE, SIM_EXE], ids=["Ratatosk", "Ratatosk_sim"])
def test_cli_hands_the_options_to_the_k2_index_step(tmp_path, exe):
    tmp = str(tmp_path)
    out, p1, raw = (os.path.join(tmp, n) for n in ("out", "p1.fq", "raw.fq"))
    for p in (p1, raw):
        open(p, "w").write("@r\nACGT\n+\nIIII\n")
    base = [exe, "correct", "-2", "-v", "-s", os.path.join(tmp, "missing.fq"), "-l", p1, "-L", raw]
    r = subprocess.run(base + ["-M", "0.5", "-C", "2000", "-Q", "41", "-o", out], capture_output=True, text=True)
    step3 = [l for l in r.stderr.split("\n") if l.startswith("Ratatosk::correct: step 3") and "rtk_build_index --gpu" in l]
    assert r.returncode != 0 and len(step3) == 1, r.stderr
    assert "--colour-reads %s --colour-min-conf 0.5 --colour-min-len 2000 --colour-max-qual 41" % p1 in step3[0], step3[0]
    assert "step 4" not in r.stderr, r.stderr  # ... and the run ended there
    assert sorted(os.listdir(tmp)) == ["p1.fq", "raw.fq"]
    r = subprocess.run(base + ["-Q", "41", "-o", out], capture_output=True, text=True)
    assert r.returncode != 0 and "step 3" in r.stderr and "--colour-m" not in r.stderr, r.stderr
    # the first index step never gets them
    r = subprocess.run([exe, "correct", "-v", "-s", os.path.join(tmp, "missing.fq"), "-l", raw, "-M", "0.5", "-C", "2000", "-o", out], capture_output=True, text=True)
    assert r.returncode != 0 and "step 1" in r.stderr and "--colour-m" not in r.stderr, r.stderr
    for m, word in (("1.5", "lower or equal to 1.0"), ("-0.1", "greater or equal to 0.0")):
        r = subprocess.run(base + ["-M", m, "-o", out], capture_output=True, text=True)
        assert r.returncode == 1 and "used for coloring in 2nd pass must be " + word in r.stderr and "step" not in r.stderr, (m, r.stderr)
    r = subprocess.run(base + ["-C", "-5", "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot be less than 0" in r.stderr and "step" not in r.stderr, r.stderr
    assert sorted(os.listdir(tmp)) == ["p1.fq", "raw.fq"]
    assert "-M, --min-conf-color2" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr


# ------------------------------------------------------------------------------------------------------------------------------------------------------ GPU tier

def _stage_cases(k, rng):
    """unitigs, and (read, quality) cases at q_min = 53 in chunks: [[(read, qual), ...], ...]"""
    unitigs = [rule.random_dna(n, rng) for n in (k, 200, 1000)]
    table = rule.kmer_table(unitigs, k)  # (asserts that the canonical k-mers are distinct)
    keep, low = chr(Q_MIN), chr(Q_MIN - 1)

    def sub(n, i):
        u = unitigs[2] if n > 150 else unitigs[1 + i % 2]
        at = (37 * i) % (len(u) - n + 1)
        s = u[at:at + n]
        return rule.revcomp(s) if i % 3 == 0 else s

    def one_low(n, at):
        return keep * at + low + keep * (n - at - 1)

    lens = (k, k + 1, 64 + k - 1, 300)
    chunks, i = [], 0
    first = []
    for n in lens:
        pats = [keep * n, "I" * n, low * n, "!" * n, (keep + low) * (n // 2) + keep * (n % 2), (low + "I") * (n // 2) + low * (n % 2)]
        pats += [one_low(n, at) for at in (0, k - 1, k, n - 1) if at < n]
        for q in pats:
            first.append((sub(n, i), q)); i += 1
    first.append((unitigs[0], keep * k)); first.append((rule.revcomp(unitigs[0]), one_low(k, k // 2)))
    chunks.append(first)
    # one masked base at a chunk offset: the first read of a chunk of its own covers offsets 0 .. 299
    for at in (15, 16, 63, 64, 255, 256):
        chunks.append([(sub(300, i), one_low(300, at)), (sub(300, i + 1), keep * 300)]); i += 2
    # the base before and the base after a separator
    chunks.append([(sub(300, i), one_low(300, 299)), (sub(300, i + 1), one_low(300, 0)), (sub(k, i + 2), keep * k)]); i += 3
    # tails of 1 .. 15 bytes behind the 16-byte body: chunks of 301 + n + 1 characters
    for n in (k, k + 1, k + 6, k + 13):
        chunks.append([(sub(300, i), one_low(300, 298)), (sub(n, i + 1), one_low(n, n - 1))]); i += 2
    return unitigs, table, chunks


def _flatten(chunks):
    reads = [r for c in chunks for r, _ in c]
    quals = [q for c in chunks for _, q in c]
    cuts = list(itertools.accumulate(len(c) for c in chunks))[:-1]
    return reads, quals, cuts


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_gpu_stage_masks_exactly(k, monkeypatch):
    """rtk_index_colour_chunk_q through api.index_colour_reads against (1) the same job fed the pre-masked characters without qualities and (2) the dictionary walk"""
    from ratatosk_amd import api
    monkeypatch.setenv(*list(SMALL_JOB.items())[0])
    rng = rule.seeded(100 + k)
    unitigs, table, chunks = _stage_cases(k, rng)
    reads, quals, cuts = _flatten(chunks)
    masked = [rule.mask(r, q, Q_MIN) for r, q in zip(reads, quals)]
    ids = list(range(len(reads)))
    w_ev, w_cov = rule.colour_walk(table, len(unitigs), k, masked, ids)
    assert len(w_ev) > 20 and all(w_cov)
    got = api.index_colour_reads(unitigs, k, reads, quals=quals, q_min=Q_MIN, chunks=cuts)
    pre = api.index_colour_reads(unitigs, k, masked, chunks=cuts)
    for ev, cov in (got, pre):
        assert ev.dtype == np.uint64 and ev.tolist() == w_ev and cov.tolist() == w_cov
    # q_min = 0, and a threshold below every byte: nothing is masked
    u_ev, u_cov = rule.colour_walk(table, len(unitigs), k, reads, ids)
    assert u_ev != w_ev
    for q_min in (0, 33):
        ev, cov = api.index_colour_reads(unitigs, k, reads, quals=quals, q_min=q_min, chunks=cuts)
        assert ev.tolist() == u_ev and cov.tolist() == u_cov, q_min
    # bytes compare unsigned: a quality byte of 200 is above the threshold
    ev, cov = api.index_colour_reads(unitigs, k, reads[:4], quals=[bytes([200]) * len(r) for r in reads[:4]], q_min=Q_MIN)
    assert (ev.tolist(), cov.tolist()) == rule.colour_walk(table, len(unitigs), k, reads[:4], ids[:4])


@pytest.mark.gpu
def test_gpu_stage_chunk_without_qualities_after_one_with(monkeypatch):
    """one job, two chunks, so both slots run: the first with qualities that mask everything, the second -- the same reads, other ids -- without: it is not masked by
    what the first left behind; and the other way round"""
    from ratatosk_amd import api
    monkeypatch.setenv(*list(SMALL_JOB.items())[0])
    k = 31
    unitigs, table, chunks = _stage_cases(k, rule.seeded(7))
    reads = [r for r, _ in chunks[0]]
    n = len(reads)
    low = ["!" * len(r) for r in reads]
    want = rule.colour_walk(table, len(unitigs), k, reads, range(n, 2 * n))
    ev, cov = api.index_colour_reads(unitigs, k, reads + reads, quals=low + [None] * n, q_min=Q_MIN, chunks=[n])
    assert (ev.tolist(), cov.tolist()) == want and len(want[0]) >= n
    want = rule.colour_walk(table, len(unitigs), k, reads, range(n))
    ev, cov = api.index_colour_reads(unitigs, k, reads + reads, quals=[None] * n + low, q_min=Q_MIN, chunks=[n])
    assert (ev.tolist(), cov.tolist()) == want
    # three chunks: the first slot is used again, with other qualities
    qs = [q for _, q in chunks[0]]
    masked = [rule.mask(r, q, Q_MIN) for r, q in zip(reads, qs)]
    want = rule.colour_walk(table, len(unitigs), k, masked + reads + masked, range(3 * n))
    ev, cov = api.index_colour_reads(unitigs, k, reads * 3, quals=qs + ["I" * len(r) for r in reads] + qs, q_min=Q_MIN, chunks=[n, 2 * n])
    assert (ev.tolist(), cov.tolist()) == want


@pytest.mark.gpu
def test_gpu_stage_chunk_beyond_one_round_of_the_launch(monkeypatch):
    """a chunk of more than 4096 x 256 characters: the mask kernel's lanes come round a second time (its launch covers 256 x 256 x 16 bytes a round)"""
    from ratatosk_amd import api
    monkeypatch.setenv(*list(SMALL_JOB.items())[0])
    k = 31
    rng = rule.seeded(9)
    unitigs, table, _ = _stage_cases(k, rng)
    keep, low = chr(Q_MIN), chr(Q_MIN - 1)
    pool = [unitigs[2][at:at + 300] for at in range(0, 700, 20)]
    pats = [keep * 300] + [keep * at + low + keep * (299 - at) for at in (0, 1, 30, 31, 150, 268, 269, 298, 299)] + [((keep * 40 + low) * 8)[:300]]
    reads, quals = [], []
    for i in range(3700):
        reads.append(pool[i % len(pool)]); quals.append(pats[(i // 7) % len(pats)])
    assert sum(len(r) + 1 for r in reads) > 4096 * 256
    masked = [rule.mask(r, q, Q_MIN) for r, q in zip(reads, quals)]
    ids = [i // 2 for i in range(len(reads))]
    want = rule.colour_walk(table, len(unitigs), k, masked, ids)
    got = api.index_colour_reads(unitigs, k, reads, ids=ids, quals=quals, q_min=Q_MIN)
    pre = api.index_colour_reads(unitigs, k, masked, ids=ids)
    assert (got[0].tolist(), got[1].tolist()) == want == (pre[0].tolist(), pre[1].tolist())
    assert want != rule.colour_walk(table, len(unitigs), k, reads, ids)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 31])
def test_gpu_tool_writes_the_filtered_bytes(data, k):
    """--gpu with the options on raw.fq == the plain filtered index == --gpu without the options on the pre-masked file; the colours ran on the device"""
    want = _build(data, k, data.fq["none"], FILTER)
    got = _build(data, k, data.fq["none"], FILTER + ["--gpu"], timeout=GPU_STEP_TIMEOUT, env=SMALL_JOB)
    assert got[:2] == want[:2]
    assert "rtk_index_colour:" in got[2] and "on the host threads" not in got[2], got[2]
    assert "5 colouring reads shorter than %d left out" % MIN_LEN in got[2], got[2]
    twin = _build(data, k, data.fq["both"], ["--gpu"], timeout=GPU_STEP_TIMEOUT, env=SMALL_JOB)
    assert twin[:2] == want[:2] and "on the host threads" not in twin[2]
    if k == 63:
        sub = _build(data, k, data.gz["none"], FILTER + ["--subsample-colours", "--gpu"], timeout=GPU_STEP_TIMEOUT, env=SMALL_JOB)
        assert sub[:2] == _build(data, k, data.fq["none"], FILTER + ["--subsample-colours", "--fast"])[:2] and "on the host threads" not in sub[2]
    else:
        r = _tool(["-s", data.sr, "-o", os.path.join(data.tmp, "refused"), "-k", str(k), "--colour-reads", data.fa["none"], "--gpu"] + FILTER, timeout=GPU_STEP_TIMEOUT, env=SMALL_JOB)
        assert r.returncode not in (0, 2) and data.fa["none"] in r.stderr and "--colour-min-conf" in r.stderr, r.stderr


ONE_SIM_ARGS = ["--seed", "17", "--ref-len", "60000", "--het", "0.003", "--repeat-frac", "0.05", "--sr-cov", "30", "--sr-err", "0.005",
                "--lr-n", "40", "--lr-len", "3000", "--lr-err", "0.08"]  # the 60 kb set of test_cli_one_command.py


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT, env=dict(os.environ, **SMALL_JOB))  # (the index steps of `correct -s` inherit it)
    assert r.returncode == 0, (args, r.stderr)
    return r


@pytest.mark.gpu
def test_gpu_one_command_with_the_reference_defaults(tmp_path):
    """`correct -s SR -l LR -M 0 -C 3000` == the four commands by hand with the options on the hand-built k2 index; the options act on this input"""
    tmp = str(tmp_path)
    pre = os.path.join(tmp, "s")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + ONE_SIM_ARGS, stderr=subprocess.DEVNULL)
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    hand = os.path.join(tmp, "hand")
    _run([TOOL, "--gpu", "-k", "31", "-s", sr, "--snps", "-o", hand + "_i1"])
    _run([EXE, "correct", "-1", "-c", "2", "-g", hand + "_i1.index.k31.fasta.gz", "-d", hand + "_i1.index.k31.rtsk", "-l", lr, "-o", hand])
    p1 = rule.read_fastq(hand + ".2.fastq")
    assert any("!" in q for _, _, q in p1), "no '!' in the first-pass reads: -M 0 would not act"
    assert any(len(s) < 3000 for _, s, _ in p1), "no first-pass read below 3000 bases: -C 3000 would not act"
    _run([TOOL, "--gpu", "-k", "63", "-s", sr, "--colour-reads", hand + ".2.fastq", "--snps", "-o", hand + "_i0"])
    _run([TOOL, "--gpu", "-k", "63", "-s", sr, "--colour-reads", hand + ".2.fastq", "--colour-min-conf", "0", "--colour-min-len", "3000", "--snps", "-o", hand + "_i2"])
    assert open(hand + "_i2.index.k63.rtsk", "rb").read() != open(hand + "_i0.index.k63.rtsk", "rb").read(), "the options change nothing on this input"
    _run([EXE, "correct", "-2", "-c", "2", "-g", hand + "_i2.index.k63.fasta.gz", "-d", hand + "_i2.index.k63.rtsk", "-l", hand + ".2.fastq", "-L", lr, "-o", hand])
    want = open(hand + ".fastq", "rb").read()
    assert want.count(b"\n") >= 4 * 40
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = _run([EXE, "correct", "-v", "-c", "2", "-s", sr, "-l", lr, "-M", "0", "-C", "3000", "-o", out])
    assert "--colour-min-conf 0 --colour-min-len 3000" in r.stderr and "--colour-max-qual" not in r.stderr
    assert open(out + ".fastq", "rb").read() == want
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)  # temporary indexes and OUT.2.fastq removed
