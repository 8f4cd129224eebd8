"""k-mer QV of reads against the short reads' k-mers (DESIGN.md section 4 [A17]): tool rtk_qv (plain and --gpu), library entries rtk_qv_begin / _chunk / _end /
_span, api.qv_reads / qv_span, `Ratatosk correct -s ... --qv`. Parity is to tests/qv_restatement.py: integers exactly; error_rate / qv parsed and compared at a
relative 1e-9 with the restatement's figures (rounded as the table prints them), "inf" / "nan" / "0" as strings.

Without a GPU: the plain route on a ds_small-sized set (two -l files, gzip / BGZF, FASTA, an empty file, K = 15 / 21 / 31, --min-count 1 / 3, -g with the unitigs
of the fixture's index, reads cut into pieces), the point of the feature on tests/golden/toy, the command-line errors. On the GPU: k_qv on the shapes at which it
can go wrong (lengths around 64, the span and k; a piece boundary on every lane; several boundaries in one step; non-bases; the table's edges; more pieces than
waves; one read of 2 Mb next to 2 000 short ones; pieces; two threads), the --gpu route's bytes, the one-command run."""
import ctypes
import gzip
import os
import re
import subprocess
import time

import numpy as np
import pytest

import qv_restatement as qr
from conftest import BIN, ROOT, SIM_LIB
from rescue_restatement import read_fastx

EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
TOOL = os.path.join(BIN, "rtk_qv")
LIB = os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so")
GPU_STEP_TIMEOUT = 600  # seconds, every child process that opens the GPU
if not os.path.exists(TOOL):  # (a tree built before the tool existed)
    import __graft_entry__
    __graft_entry__.build()

HEADER = "file\treads\tbases\twindows\tfound\tmissing\terror_rate\tqv"


def _tool(args, env=None, timeout=None):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_THREADS="4", **(env or {})), timeout=timeout)


def _write_fastq(path, records):
    with open(path, "w") as f:
        for n, s in records:
            f.write("@%s extra words\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _same_figure(got, want):
    if isinstance(want, str):
        return got == want
    return got not in ("nan", "inf") and abs(float(got) - want) <= 1e-9 * abs(want)


def _check_outputs(out, files, k, kmers, per_read=True):
    """OUT.qv.tsv (and OUT.qv.reads.tsv) against the restatement. files = [(path as given to -l, [(name, seq)])]; returns the table's rows."""
    arr = qr.sorted_array(kmers)
    lines = open(out + ".qv.tsv").read().split("\n")
    assert lines[0] == HEADER and lines[-1] == "" and len(lines) == len(files) + 2, lines
    rows, want_reads = [], ["file_index\tname\tlength\twindows\tfound"]
    for f, (path, records) in enumerate(files):
        counts = [qr.windows_found(s, k, arr) for _, s in records]
        w, fd = sum(c[0] for c in counts), sum(c[1] for c in counts)
        missing, e, q = qr.row(w, fd, k)
        col = lines[1 + f].split("\t")
        assert col[:6] == [path, str(len(records)), str(sum(len(s) for _, s in records)), str(w), str(fd), str(w - fd)], (col, w, fd)
        assert missing == w - fd or w == 0
        assert _same_figure(col[6], e) and _same_figure(col[7], q), (col, e, q)
        rows.append(col)
        want_reads += ["%d\t%s\t%d\t%d\t%d" % (f, n, len(s), c[0], c[1]) for (n, s), c in zip(records, counts)]
    if per_read:
        assert open(out + ".qv.reads.tsv").read() == "\n".join(want_reads) + "\n"
    else:
        assert not os.path.exists(out + ".qv.reads.tsv")
    return rows


class Data:
    pass


@pytest.fixture(scope="module")
def data(ds_small, tmp_path_factory):
    """The short and long reads of the ds_small set; the long reads as two -l files; the short reads' k-mer sets come from the restatement, once per (K, count)."""
    d = Data(); d.tmp = str(tmp_path_factory.mktemp("qv"))
    d.sr = ds_small + ".sr.fq"
    d.unitigs = ds_small + ".index.k31.fasta.gz"
    d.sr_seqs = [s for _, s in read_fastx(d.sr)]
    lr = read_fastx(ds_small + ".lr.fq")
    assert len(lr) == 12
    lr[3] = (lr[3][0], lr[3][1][:500].lower() + "N" + lr[3][1][501:])  # lower case counts as bases, an N does not
    d.l1, d.l2 = os.path.join(d.tmp, "l1.fq"), os.path.join(d.tmp, "l2.fq")
    d.rec1, d.rec2 = lr[:7], lr[7:]
    _write_fastq(d.l1, d.rec1); _write_fastq(d.l2, d.rec2)
    d.sets = {}
    return d


def _set(d, k, min_count=2):
    if (k, min_count) not in d.sets:
        d.sets[(k, min_count)] = qr.kmer_set(d.sr_seqs, k, min_count)
    return d.sets[(k, min_count)]


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("chunk", [None, "1024"], ids=["whole-reads", "pieces-of-1023"])
def test_plain_two_files_rows_in_the_order_given(data, tmp_path, chunk):
    out = str(tmp_path / "o")
    r = _tool(["-s", data.sr, "-l", data.l2, "-l", data.l1, "-k", "31", "-o", out, "--per-read", "-v"], env={"RTK_INDEX_CHUNK": chunk} if chunk else None)
    assert r.returncode == 0, r.stderr
    rows = _check_outputs(out, [(data.l2, data.rec2), (data.l1, data.rec1)], 31, _set(data, 31))
    assert all(0 < int(c[4]) < int(c[3]) for c in rows)  # raw 8 %-error reads: some windows found, most not
    for lap in ("count", "table", "filter"):
        assert re.search(r"rtk_qv: \[ *[0-9.]+ s\] %s" % lap, r.stderr), r.stderr
    assert r.stderr.endswith(open(out + ".qv.tsv").read())  # the table is shown as well
    assert sorted(os.listdir(str(tmp_path))) == ["o.qv.reads.tsv", "o.qv.tsv"]


def test_plain_gzip_bgzf_fasta_list_and_an_empty_file(data, tmp_path):
    tmp = str(tmp_path)
    l1z, l2b, srb = os.path.join(tmp, "l1.fq.gz"), os.path.join(tmp, "l2.bgz"), os.path.join(tmp, "sr.bgz")
    with open(data.l1, "rb") as fi, gzip.open(l1z, "wb") as fo:
        fo.write(fi.read())
    subprocess.check_call([os.path.join(BIN, "rtk_bgzip"), data.l2, l2b])
    subprocess.check_call([os.path.join(BIN, "rtk_bgzip"), data.sr, srb])
    fa = os.path.join(tmp, "l2.fa")
    with open(fa, "w") as f:  # FASTA on several lines, a description after the name
        for n, s in data.rec2:
            f.write(">%s some description\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))))
    empty = os.path.join(tmp, "empty.fq")
    open(empty, "w").close()
    out = os.path.join(tmp, "o")
    r = _tool(["-s", srb, "-l", l1z, "-l", l2b, "-l", fa, "-l", empty, "-k", "31", "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    rows = _check_outputs(out, [(l1z, data.rec1), (l2b, data.rec2), (fa, data.rec2), (empty, [])], 31, _set(data, 31))
    assert rows[3][1:] == ["0", "0", "0", "0", "0", "nan", "nan"]
    lst = os.path.join(tmp, "reads.txt")  # a text file of paths: one row per path
    open(lst, "w").write(data.l1 + "\n" + fa + "\n")
    r = _tool(["-s", data.sr, "-l", lst, "-k", "31", "-o", out])
    assert r.returncode == 0, r.stderr
    _check_outputs(out, [(data.l1, data.rec1), (fa, data.rec2)], 31, _set(data, 31), per_read=False)  # (and the file of the run before is gone)


@pytest.mark.parametrize("k", [15, 21, 31])
def test_plain_other_k(data, tmp_path, k):
    out = str(tmp_path / "o")
    r = _tool(["-s", data.sr, "-l", data.l1, "-l", data.l2, "-k", str(k), "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    _check_outputs(out, [(data.l1, data.rec1), (data.l2, data.rec2)], k, _set(data, k))


@pytest.mark.parametrize("min_count", [1, 3])
def test_plain_min_count(data, tmp_path, min_count):
    out = str(tmp_path / "o")
    r = _tool(["-s", data.sr, "--min-count", str(min_count), "-l", data.l1, "-k", "31", "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    _check_outputs(out, [(data.l1, data.rec1)], 31, _set(data, 31, min_count))
    assert len(_set(data, 31, 1)) > len(_set(data, 31, 2)) > len(_set(data, 31, 3)) > 0  # the three sets differ, so the option shows


def test_plain_set_from_the_unitigs_of_an_index(data, tmp_path):
    out = str(tmp_path / "o")
    r = _tool(["-g", data.unitigs, "-l", data.l1, "-l", data.l2, "-k", "31", "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    kmers = qr.kmer_set([s for _, s in read_fastx(data.unitigs)], 31, 1)
    assert len(kmers) > 20000
    _check_outputs(out, [(data.l1, data.rec1), (data.l2, data.rec2)], 31, kmers)


def test_corrected_toy_reads_score_higher_than_the_raw_ones(tmp_path):
    """The point of the feature, on the hand-checked fixture: against the k-mers seen twice in sr.fq, the corrected reads hold a larger share of supported
    31-mers than the raw ones, and a larger QV."""
    toy = os.path.join(ROOT, "tests", "golden", "toy")
    sr, raw, fixed = os.path.join(toy, "sr.fq"), os.path.join(toy, "lr.fq"), os.path.join(toy, "expected.fastq")
    out = str(tmp_path / "o")
    r = _tool(["-s", sr, "-l", raw, "-l", fixed, "-k", "31", "-o", out, "--per-read"])
    assert r.returncode == 0, r.stderr
    kmers = qr.kmer_set([s for _, s in read_fastx(sr)], 31, 2)
    before, after = _check_outputs(out, [(raw, read_fastx(raw)), (fixed, read_fastx(fixed))], 31, kmers)
    assert int(before[3]) > 0 and int(after[3]) > 0
    assert int(after[4]) * int(before[3]) > int(before[4]) * int(after[3])  # found / windows, in integers
    if after[5] == "0":
        assert after[7] == "inf" and before[7] != "inf"
    else:
        assert float(after[7]) > float(before[7])


def test_command_line_errors_are_status_2_and_bad_inputs_status_1(data, tmp_path):
    out = str(tmp_path / "o")
    base = ["-l", data.l1, "-o", out]
    for args in (["-s", data.sr, "-k", "30"] + base, ["-s", data.sr, "-k", "33"] + base, ["-s", data.sr, "-k", "31", "-o", out], ["-k", "31"] + base,
                 ["-s", data.sr, "-g", data.unitigs, "-k", "31"] + base, ["-s", data.sr, "-k", "31", "--frobnicate"] + base,
                 ["-g", data.unitigs, "--min-count", "2", "-k", "31"] + base, ["-s", data.sr, "--min-count", "0", "-k", "31"] + base, ["-s", data.sr, "-k", "31", "-l", data.l1, "-o"]):
        r = _tool(args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    r = _tool(["-s", data.sr, "-k", "31", "-l", str(tmp_path / "missing.fq"), "-o", out])
    assert r.returncode == 1 and "missing.fq" in r.stderr
    bad = str(tmp_path / "cut.fq.gz")
    with gzip.open(bad, "wb") as fo:
        fo.write(open(data.sr, "rb").read()[:400000])
    blob = open(bad, "rb").read()
    open(bad, "wb").write(blob[:len(blob) // 2])  # a gzip stream cut short is not the end of the reads
    for args in (["-s", data.sr, "-l", bad], ["-s", bad, "-l", data.l1]):
        r = _tool(args + ["-k", "31", "-o", out, "--per-read"])
        assert r.returncode == 1, (args, r.stderr)
    assert os.listdir(str(tmp_path)) == ["cut.fq.gz"]  # no run above left a file


@pytest.mark.parametrize("exe", [EXE, SIM_EXE], ids=["Ratatosk", "Ratatosk_sim"])
def test_cli_qv_next_to_a_prebuilt_index_is_refused_before_anything_runs(tmp_path, exe):
    out = str(tmp_path / "out")
    for args in (["-1", "--qv", "-g", "a", "-d", "b"], ["-2", "-g", "a", "-d", "b", "-L", "r", "--qv"], ["-1", "-s", "x", "-g", "a", "-d", "b", "--qv"]):
        r = subprocess.run([exe, "correct"] + args + ["-l", "c", "-o", out], capture_output=True, text=True)
        assert r.returncode == 1 and "rtk_qv -g" in r.stderr, (args, r.stderr)
    assert os.listdir(str(tmp_path)) == []
    assert "--qv" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr


def test_header_and_libraries_hold_the_qv_entries():
    txt = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    for name in ("rtk_qv_begin", "rtk_qv_chunk", "rtk_qv_end", "rtk_qv_span"):
        assert re.search(r"\b(int|uint32_t)\s+%s\s*\(" % name, txt), name
        for path in (LIB, SIM_LIB):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    sim = ctypes.CDLL(SIM_LIB)
    job = ctypes.c_void_p()
    assert sim.rtk_qv_begin(0, 31, None, ctypes.c_uint64(0), ctypes.byref(job)) != 0  # as the rescue entries there: not part of the simulator build


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _random_text(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _half(text, k):
    """About half of the canonical k-mers of a text, chosen by a hash of the k-mer: sorted array."""
    can, valid = qr.canonical_kmers(text, k)
    u = np.unique(can[valid])
    return u[((u * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63)) == 1]


class Gpu:
    pass


@pytest.fixture(scope="module")
def gpu():
    """One random text of 80 kb and, for K = 31 and 15, half of its k-mers; api and the span. Shared by the GPU tests and left unchanged."""
    from ratatosk_amd import api
    g = Gpu(); g.api = api; g.S = api.qv_span()
    rng = np.random.default_rng(20261020)
    g.text = _random_text(rng, 80000)
    g.other = _random_text(rng, 4000)  # (none of its 31-mers is in the text)
    g.sets = {k: _half(g.text, k) for k in (31, 15)}
    g.rng = rng
    return g


def _lengths(S, k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129, S - 1, S, S + 1, S + k - 2, S + k - 1, S + k, 3 * S + 17, 70001]


def _cut_reads(text, lengths):
    """One read of each length, each from another place of the text."""
    return [text[(37 * i * i + 11 * i) % (len(text) - n + 1):][:n] for i, n in enumerate(lengths)]


def _expect(seqs, k, arr):
    """([windows], [found]) per read from the restatement: the reads laid end to end with a separator (no base: no window crosses it), summed per read."""
    can, valid = qr.canonical_kmers("\n".join(seqs) + "\n" + "N" * (k - 1), k)  # one entry per character of the joined reads
    hit = valid & np.isin(can, arr)
    cw, cf = np.concatenate(([0], np.cumsum(valid))), np.concatenate(([0], np.cumsum(hit)))
    ends = np.cumsum([len(s) + 1 for s in seqs])
    begs = ends - np.array([len(s) + 1 for s in seqs])
    return [int(x) for x in cw[ends] - cw[begs]], [int(x) for x in cf[ends] - cf[begs]]


def _check(g, seqs, k, arr, **kw):
    st = {}
    got = g.api.qv_reads(arr, seqs, k=k, stats=st, **kw)
    want = _expect(seqs, k, arr)
    assert got == want, [(i, len(s), got[0][i], want[0][i], got[1][i], want[1][i]) for i, s in enumerate(seqs) if (got[0][i], got[1][i]) != (want[0][i], want[1][i])][:10]
    assert (st["n_windows"], st["n_found"]) == (sum(want[0]), sum(want[1]))
    return want, st


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 15])
def test_gpu_lengths_around_64_the_span_and_k(gpu, k):
    seqs = _cut_reads(gpu.text, _lengths(gpu.S, k))
    (w, f), st = _check(gpu, seqs, k, gpu.sets[k])
    assert st["n_chunks"] == 1
    assert w == [max(0, len(s) - k + 1) for s in seqs] and 0.3 * sum(w) < sum(f) < 0.7 * sum(w)  # half of the windows are found
    _check(gpu, seqs[::-1], k, gpu.sets[k])  # the same reads at other places of the chunk


@pytest.mark.gpu
def test_gpu_a_piece_boundary_on_every_lane(gpu):
    seqs = _cut_reads(gpu.text, list(range(40, 170)))
    bounds = np.cumsum([len(s) + 1 for s in seqs])
    assert len(set(int(b) % 64 for b in bounds)) == 64  # every residue of a boundary occurs
    _check(gpu, seqs, 31, gpu.sets[31])
    with_empty = []
    for i, s in enumerate(seqs):  # empty reads between them, up to five in a row: several boundaries in one 64-position step
        with_empty += [s] + [""] * (i % 6)
    (w, _), _ = _check(gpu, with_empty + [""] * 70, 31, gpu.sets[31])  # (and a step that is boundaries only)
    assert sum(1 for x in w if x == 0) >= 300
    short = _cut_reads(gpu.text, [5, 31, 7, 32, 1, 33, 2, 31, 31, 9] * 40)  # reads shorter than a step: up to a dozen boundaries in one
    _check(gpu, short, 31, gpu.sets[31])


@pytest.mark.gpu
def test_gpu_non_bases(gpu):
    k, t = 31, gpu.text
    base = t[1000:1200]
    put = lambda s, i, c: s[:i] + c + s[i + 1:]
    seqs = [put(base, 0, "N"), put(base, k - 1, "N"), put(base, 100, "N"), put(base, 199, "N"), base.lower(), base[:90].lower() + base[90:], put(base.lower(), 100, "n"),
            "R" * 100, "RYN" * 50, "N" * 31, put(base, 64, "\r"), put(base, 63, "\r"), base + "\r", put(put(base, 10, "-"), 150, "*"), put(base, 100, "\x00"), put(base, 100, "@"), put(base, 100, "!")]
    (w, f), _ = _check(gpu, seqs, k, gpu.sets[k])
    assert w[:4] == [169, 170 - k, 170 - k, 169] and w[4] == 170 and f[4] == f[5] > 0 and w[7:10] == [0, 0, 0] and w[10] == 170 - k and w[12] == 170


@pytest.mark.gpu
def test_gpu_the_sets_edges(gpu):
    k = 31
    seqs = _cut_reads(gpu.text, [200, 31, 5000]) + ["A" * 100, "T" * 100, "a" * 40]
    (w, f), _ = _check(gpu, seqs, k, np.zeros(0, dtype=np.uint64))  # an empty set: nothing is found
    assert sum(f) == 0 and sum(w) > 0
    one = qr.sorted_array(qr.kmer_set([seqs[1]], k))
    assert len(one) == 1
    (_, f), _ = _check(gpu, seqs + [gpu.text[:3000]], k, one)
    assert f[1] == 1
    top = "T" * 15 + "C" + "A" * 15  # the largest canonical 31-mer: any larger code has a smaller reverse complement
    can, _ = qr.canonical_kmers(top, k)
    code = sum("ACGT".index(c) << (2 * (k - 1 - i)) for i, c in enumerate(top))
    assert int(can[0]) == code and int(qr.canonical_kmers("T" * 15 + "G" + "A" * 15, k)[0][0]) == code and code >> 61 == 1  # (its reverse complement)
    assert int(qr.canonical_kmers("T" * 16 + "A" * 15, k)[0][0]) < code  # a T in the middle: the reverse complement, with an A there, is the smaller one
    edges = np.array([0, code], dtype=np.uint64)  # the all-A k-mer (code 0) and the largest one
    reads = ["A" * 100, "T" * 100, "A" * 31, "T" * 30, "GG" + top + "GG", "C" + "T" * 15 + "G" + "A" * 15 + "C", "A" * 50 + "C" + "A" * 50] + seqs[:3]
    (w, f), _ = _check(gpu, reads, k, edges)
    assert f[:7] == [70, 70, 1, 0, 1, 1, 40] and sum(f[7:]) == 0
    rng = np.random.default_rng(5)
    big_text = _random_text(rng, (1 << 20) + k - 1)  # 2^20 random k-mers: probe chains in the table
    can, valid = qr.canonical_kmers(big_text, k)
    big = np.unique(can)
    assert valid.all() and len(big) > (1 << 20) - 16
    reads = [big_text[o:o + 3000] for o in range(0, len(big_text) - 3000, 50021)] + [gpu.other, gpu.text[:3000]]
    (w, f), _ = _check(gpu, reads, k, big)
    assert f[:-2] == w[:-2] and f[-2:] == [0, 0]


@pytest.mark.gpu
def test_gpu_more_pieces_than_waves(gpu):
    seqs = [gpu.text[(31 * i) % 79000:][:33] for i in range(20000)]
    (w, _), st = _check(gpu, seqs, 31, gpu.sets[31])
    assert w == [3] * 20000 and st["n_chunks"] == 1


@pytest.mark.gpu
def test_gpu_one_read_of_two_megabases_next_to_two_thousand_short_ones(gpu):
    rng = np.random.default_rng(6)
    tiles = [gpu.text[o:o + 20000] for o in (0, 20000, 40000, 60000)]
    long_read = "".join(tiles[i] for i in rng.integers(0, 4, 100))  # 2 000 000 bases, half of its windows found
    assert len(long_read) == 2000000
    seqs = [gpu.text[(41 * i) % 79000:][:150] for i in range(1000)] + [long_read] + [gpu.text[(43 * i) % 79000:][:150] for i in range(1000)]
    arr = gpu.sets[31]
    want = _expect(seqs, 31, arr)
    gpu.api.qv_reads(arr, seqs[:10], k=31)  # (the library and the device are up)
    t0 = time.perf_counter()
    got = gpu.api.qv_reads(arr, seqs, k=31)
    print("qv_reads, 1 read of 2 000 000 + 2 000 reads of 150: %.3f s wall (table, layout, copies and k_qv)" % (time.perf_counter() - t0))
    assert got == want and want[0][1000] == 2000000 - 30 and 0.3 * 2000000 < want[1][1000] < 0.7 * 2000000


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 15])
def test_gpu_reads_cut_into_pieces_add_up(gpu, k):
    seqs = _cut_reads(gpu.text, _lengths(gpu.S, k))
    for max_piece in (1000, gpu.S + 7):
        pieces = sum(len(qr.cut(len(s), k, max_piece)) for s in seqs)
        assert pieces > len(seqs) + 30
        _, st = _check(gpu, seqs, k, gpu.sets[k], max_piece=max_piece)
        assert st["n_chunks"] > 30
    assert qr.cut(70001, 31, 1000)[:2] == [(0, 1000), (970, 1970)] and qr.cut(1000, 31, 1000) == [(0, 1000)] and qr.cut(0, 31, 1000) == [(0, 0)]


@pytest.mark.gpu
def test_gpu_two_threads_feed_the_chunks(gpu):
    seqs = [gpu.text[(53 * i) % 79000:][:100 + i % 200] for i in range(600)]
    st1, st2 = {}, {}
    one = gpu.api.qv_reads(gpu.sets[31], seqs, k=31, max_piece=15000, threads=1, stats=st1)
    two = gpu.api.qv_reads(gpu.sets[31], seqs, k=31, max_piece=15000, threads=2, stats=st2)
    assert st1["n_chunks"] == st2["n_chunks"] >= 8
    assert one == two == _expect(seqs, 31, gpu.sets[31]) and st1 == st2


@pytest.mark.gpu
def test_gpu_tool_writes_the_plain_routes_bytes(data, tmp_path):
    for name, set_args in (("s", ["-s", data.sr]), ("g", ["-g", data.unitigs])):
        plain, dev = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_dev"))
        args = set_args + ["-l", data.l2, "-l", data.l1, "-k", "31", "--per-read"]
        assert _tool(args + ["-o", plain]).returncode == 0
        r = _tool(["--gpu"] + args + ["-o", dev], env={"RTK_INDEX_TRACE": "1", "RTK_INDEX_CHUNK": "8192"}, timeout=GPU_STEP_TIMEOUT)
        assert r.returncode == 0, r.stderr
        assert int(re.search(r"characters in (\d+) chunks", r.stderr).group(1)) >= 4, r.stderr
        for ext in (".qv.tsv", ".qv.reads.tsv"):
            assert open(dev + ext, "rb").read() == open(plain + ext, "rb").read(), (name, ext)
    _check_outputs(str(tmp_path / "s_dev"), [(data.l2, data.rec2), (data.l1, data.rec1)], 31, _set(data, 31))


@pytest.mark.gpu
def test_gpu_one_command_run_with_qv(ds_small, tmp_path):
    sr, lr = ds_small + ".sr.fq", ds_small + ".lr.fq"
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.mkdir(a); os.mkdir(b)
    r = subprocess.run([EXE, "correct", "-c", "2", "-s", sr, "-l", lr, "-o", os.path.join(a, "out")], capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT)
    assert r.returncode == 0, r.stderr
    out = os.path.join(b, "out")
    r = subprocess.run([EXE, "correct", "-c", "2", "-s", sr, "-l", lr, "-o", out, "--qv"], capture_output=True, text=True, timeout=GPU_STEP_TIMEOUT)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(b)) == ["out.fastq", "out.qv.tsv"]
    assert open(out + ".fastq", "rb").read() == open(os.path.join(a, "out.fastq"), "rb").read()
    table = open(out + ".qv.tsv").read()
    lines = table.split("\n")
    assert lines[0] == HEADER and len(lines) == 4 and table in r.stderr
    before, after = lines[1].split("\t"), lines[2].split("\t")
    assert before[0] == lr and after[0] == out + ".fastq" and before[1] == after[1] == "12"
    assert int(after[4]) * int(before[3]) > int(before[4]) * int(after[3])  # found / windows went up
    kmers = qr.kmer_set([s for _, s in read_fastx(sr)], 31, 2)
    _check_outputs(out, [(lr, read_fastx(lr)), (out + ".fastq", read_fastx(out + ".fastq"))], 31, kmers, per_read=False)
