"""Anchor stage (k_lookup_exact, k_mask, k_inexact / k_inexact_enum, k_finalize) at the places the read-shaped tests do not reach, against the oracle
(`op.Graph(...).seeds` / `.exact`); every comparison is exact equality. One body per topic, run by the host simulator (test_sim_*) and on the device
(test_gpu_*):
  B1  the anchors of every read of a batch of MANY reads (Batch.seeds, stage entry rtk_batch_fetch_seeds): reads that share 64-base tiles, read starts on
      every residue modulo 64, reads of the lengths around k and around one and two tiles, empty / all-N / lower-case reads, three orders of the batch
  B2  k = 25 and k = 21 and the tandem set, under the half-k-mer search, the enumerating search by its knob, and the enumerating search because the
      half-k-mer index was not built; palindromic half-k-mers planted next to one-edit windows (the `palin` branch of rtk_seeded_window)
  B3  the k-mer table asked about itself: every k-mer of the graph on both strands, the one-substitution neighbours of every 7th, strings around k
      characters, N and lower case, one-edit windows at unitig ends (the flank words and the following-bases bit of a half-k-mer place)
  B4  the mask's gap, head and tail rules at odd insert sizes (a gap, a head and a tail of exactly half the insert size and of the whole of it, one window
      either way, the gap filled with windows one edit away from the graph), and at insert sizes below 2 k, where two hits that bound a gap lie fewer than k windows apart"""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import BIN, SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api
from test_sim_seeds import _check, _check_gap_reads

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def _rc(s):
    return s[::-1].translate(_COMP)


def _graphs(prefix, k, lib_path):
    fa, rt = prefix + ".index.k%d.fasta.gz" % k, prefix + ".index.k%d.rtsk" % k
    return op.Graph(fa, rt, k), api.Graph(fa, rt, k, device=0, lib_path=lib_path)


def _batch_seeds(pg, reads, opts=None):
    """the anchors of every read of ONE batch"""
    b = api.Batch(pg, reads)
    try:
        b.run_seeds(opts)
        return [b.seeds(i) for i in range(len(reads))]
    finally:
        b.close()


def _ref_text(prefix):
    return "".join(l.strip() for l in open(prefix + ".ref.fa") if not l.startswith(">"))


def _near_miss(s, rnd, k=31):
    """s with a substitution at the characters k / 2, k / 2 + (k - 1), k / 2 + 2 (k - 1), ...: every window of k characters holds one of them (no exact hit),
    and all but every (k - 1)th window holds exactly one: where s is a stretch of the reference, those windows are one edit away from the graph"""
    for at in range(k // 2, len(s), k - 1):
        s = _edit(s, at, 0, rnd)
    return s


def _opened_head(ref, c, n, a, m, rnd):
    """n >= 250 near-miss characters of the reference at c in front of m characters of the reference at a: the first hit lies at n, so the head rule of the
    mask (default insert size) opens everything in front of it, and the read's FIRST window, the one at the read's own offset 0, is a candidate of the
    1-edit search: the window whose owner the stage finds by stepping forward to the read that starts exactly at it."""
    return _near_miss(ref[c:c + n], rnd) + ref[a:a + m]


# ------------------------------------------------------------------------------------------------ B1: batched anchors
def _edge_batch(seqs, k, ref):
    """The reads of B1, in order: cuts of the set's reads to the lengths at which a read stops having windows (1, k - 1, k, k + 1), fills a tile with its
    last window (k + 62, k + 63, k + 64), ends two tiles (2 * 64 + k - 1) and is masked in more than one round of a wave (4096 + k); an all-N read, N at
    the first / the last position, a lower-case read, three whole reads, an empty read (rtk_batch_create accepts one); between them runs of 1-, 2-, 3-,
    5- and 7-base reads; four reads with an opened head (_opened_head), which start in the tile the fillers in front of them end in. Returns (reads,
    indices of the reads that are not fillers, indices of the opened-head reads)."""
    long_src = max(seqs, key=len)
    if len(long_src) < 4096 + k:  # (no read of the set is that long: two of them end to end)
        long_src = (seqs[0] + seqs[1] + seqs[2])[:4096 + k]
    main = [seqs[i % len(seqs)][50 * i:50 * i + n] for i, n in enumerate((1, k - 1, k, k + 1, k + 62, k + 63, k + 64, 2 * 64 + k - 1))]
    main.append(long_src[:4096 + k])
    main += ["N" * 100, "N" + seqs[3][1:700], seqs[4][:700] + "N", seqs[5][:900].lower(), ""]
    main += [seqs[0], seqs[1], seqs[2]]
    heads = [_opened_head(ref, 9000 + 4000 * i, 250 + 7 * i, 2000 + 3000 * i, 120 + 13 * i, random.Random(40 + i)) for i in range(4)]
    main += heads
    reads, keep, rnd, n_fill = [], [], random.Random(3), 0
    for m in main:
        for j in range(5 + len(reads) % 4):  # a run of fillers in front of every read
            n = (1, 2, 3, 5, 7)[n_fill % 5]; n_fill += 1
            p = rnd.randrange(0, len(seqs[0]) - 8)
            reads.append(seqs[0][p:p + n])
        keep.append(len(reads)); reads.append(m)
    # ... and behind the last one, each of a length that puts the next read start on a residue modulo 64 no start has had yet (else 1)
    seen, at = set(s % 64 for s in _starts(reads)), sum(len(r) for r in reads)
    for j in range(200):
        n = next((n for n in (7, 5, 3, 2, 1) if (at + n) % 64 not in seen), 1)
        reads.append(seqs[1][j:j + n]); at += n; seen.add(at % 64)
        if len(seen) == 64:
            break
    reads.append(seqs[1][300:305])
    return reads, keep, [i for i in keep if reads[i] in heads]


def _starts(reads):
    out, at = [], 0
    for r in reads:
        out.append(at); at += len(r)
    return out


def _shares_a_tile(reads):
    """indices of the non-empty reads whose first or last base lies in a 64-base tile of the batch that also holds a base of another read"""
    st, out = _starts(reads), []
    tiles = {}
    for i, r in enumerate(reads):
        for t in set((st[i] // 64, (st[i] + len(r) - 1) // 64) if r else ()):
            tiles.setdefault(t, set()).add(i)
    for i, r in enumerate(reads):
        if r and any(len(tiles[t]) > 1 for t in (st[i] // 64, (st[i] + len(r) - 1) // 64)):
            out.append(i)
    return out


def _check_batched(prefix, lib_path, min_solid=200, min_weak=20):
    k = 31
    og, pg = _graphs(prefix, k, lib_path)
    seqs = [r[1] for r in op.read_fastq(prefix + ".lr.fq")]
    reads, keep, heads = _edge_batch(seqs, k, _ref_text(prefix))
    assert "" in reads and set(s % 64 for s in _starts(reads)) == set(range(64))  # read starts on every residue modulo 64
    memo = {}
    for r in reads:
        if r not in memo:
            memo[r] = og.seeds(r.upper())  # (the entries upper-case a read as the worker does before getSeeds, src/Ratatosk.cpp:814; the oracle's stage calls do not)
    want = [memo[r] for r in reads]
    # non-vacuity, from the oracle alone
    n_solid, n_weak = sum(len(w[0]) for w in want), sum(len(w[1]) for w in want)
    shared = [i for i in _shares_a_tile(reads) if want[i][0] or want[i][1]]
    print("B1 %s: %d reads, %d solid and %d weak anchors, %d reads with anchors share a tile with a neighbour" % (os.path.basename(prefix), len(reads), n_solid, n_weak, len(shared)))
    assert n_solid >= min_solid and n_weak >= min_weak and len(shared) >= 5
    # the opened-head reads share their first tile with the read in front, and the oracle keeps a weak anchor at their offset 0
    n_at_0 = sum(1 for i in heads if i in shared and any(a[0] == 0 for a in want[i][1]))
    print("B1 %s: weak anchor at offset 0 of %d of %d opened-head reads" % (os.path.basename(prefix), n_at_0, len(heads)))
    assert len(heads) == 4 and n_at_0 >= 3
    got = _batch_seeds(pg, reads)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, ("read %d of the batch (%d bases, starts at %d)" % (i, len(reads[i]), _starts(reads)[i]))
    # (a) the order of the reads in the batch does not change a read's anchors
    perm = list(range(len(reads))); random.Random(17).shuffle(perm)
    for order in (list(range(len(reads)))[::-1], perm):
        got = _batch_seeds(pg, [reads[i] for i in order])
        for at, i in enumerate(order):
            assert got[at] == want[i], ("read %d at place %d" % (i, at))
    # (b) a read alone (rtk_seeds: a batch of one) and the same read inside the batch
    for r in sorted(set(reads), key=len):
        assert pg.seeds(r) == memo[r], len(r)
    # the refusals of the entry: a read the batch does not have, a batch that has not been seeded (or whose regions have run since), a small cap
    b = api.Batch(pg, reads)
    try:
        with pytest.raises(api.RtkError):
            b.seeds(0)
        b.run_seeds()
        with pytest.raises(api.RtkError):
            b.seeds(len(reads))
        i = max(keep, key=lambda j: len(want[j][0]))
        with pytest.raises(api.RtkError) as e:
            b.seeds(i, cap=len(want[i][0]) - 1)
        assert "capacity" in str(e.value)
        assert b.seeds(i, cap=max(len(want[i][0]), len(want[i][1]))) == want[i]
        b.run_regions()
        with pytest.raises(api.RtkError):
            b.seeds(0)
    finally:
        b.close()
    return og, pg, seqs


def _check_every_offset(prefix, lib_path):
    """(c) ONE batch of 128 reads, pad and probe in turn: pad r has 64 + r characters and the probe 2944 = 46 * 64, so that probe r starts at
    64 r + r (r + 1) / 2, and the triangular numbers of 0 .. 63 are all different modulo 64: the probe -- and the read in front of it, whose last tile it
    shares -- at every offset of a tile."""
    k = 31
    og, pg = _graphs(prefix, k, lib_path)
    seqs = [r[1] for r in op.read_fastq(prefix + ".lr.fq")]
    ref = _ref_text(prefix)
    # the read of the set, and a read of the same length with an opened head (_opened_head): its window at offset 0 is searched, at every offset of a tile
    for name, probe in (("read of the set", seqs[0][:2944]), ("opened head", _opened_head(ref, 12000, 280, 4000, 2944 - 280, random.Random(6)))):
        assert len(probe) == 2944
        reads = []
        for r in range(64):
            reads += [seqs[1][7 * r:7 * r + 64 + r], probe]
        st = _starts(reads)
        assert set(st[2 * r + 1] % 64 for r in range(64)) == set(range(64))
        want_probe = og.seeds(probe)
        assert len(want_probe[0]) >= 20 and len(want_probe[1]) >= 1
        if name == "opened head":
            assert any(a[0] == 0 for a in want_probe[1]), "the oracle keeps no weak anchor at the probe's offset 0"
        got = _batch_seeds(pg, reads)
        for r in range(64):
            assert got[2 * r + 1] == want_probe, ("%s at offset %d of its tile" % (name, st[2 * r + 1] % 64))
            assert got[2 * r] == og.seeds(reads[2 * r]), ("pad of %d characters" % (64 + r))


def test_sim_batched_anchors_branching(ds_small):
    _check_batched(ds_small, SIM_LIB)


def test_sim_batched_anchors_clean(ds_clean):
    _check_batched(ds_clean, SIM_LIB)


def test_sim_batched_anchors_every_offset(ds_small):
    _check_every_offset(ds_small, SIM_LIB)


@pytest.mark.gpu
def test_gpu_batched_anchors_branching(ds_small):
    _check_batched(ds_small, None)


@pytest.mark.gpu
def test_gpu_batched_anchors_clean(ds_clean):
    _check_batched(ds_clean, None)


@pytest.mark.gpu
def test_gpu_batched_anchors_every_offset(ds_small):
    _check_every_offset(ds_small, None)


# ------------------------------------------------------------------------------------------------ B2: other k, both searches
_HX = 16  # flat buffer of the half-k-mer index (order of rtk_graph_buffer)


def _hx_words(pg):
    p, b = C.c_void_p(), C.c_uint64()
    pg._check(pg.L.rtk_graph_buffer(pg.h, _HX, C.byref(p), C.byref(b)))
    return b.value // 8


def _check_set(prefix, k, n, lib_path):
    """the set's reads and the edge reads of test_sim_seeds._check at the default insert size; the set's reads once more, as ONE batch, at an insert size of
    4 k (at k = 21 every sixth window of these reads has an exact hit: no stretch of 250 windows is without one, and the default opens nothing). Returns
    the weak anchors of the two."""
    tot = _check(prefix, n, lib_path, k=k)
    og, pg = _graphs(prefix, k, lib_path)
    seqs = [r[1] for r in op.read_fastq(prefix + ".lr.fq")[:n]]
    want = [og.seeds(s, og.opts(insert_sz=4 * k)) for s in seqs]
    got = _batch_seeds(pg, seqs, pg.opts(insert_sz=4 * k))
    for i, (g_, w) in enumerate(zip(got, want)):
        assert g_ == w, (k, i)
    return tot, sum(len(w[1]) for w in want)


def _check_three_ways(prefix, k, n, lib_path, monkeypatch):
    """(i) the half-k-mer search, (ii) RTK_INEXACT_ENUM=1, (iii) RTK_HX_MAX_GB=0: the index is estimated above the cap and not built (one empty slot:
    hx_mask == 0), which selects k_inexact_enum without its knob"""
    fa, rt = prefix + ".index.k%d.fasta.gz" % k, prefix + ".index.k%d.rtsk" % k
    assert _hx_words(api.Graph(fa, rt, k, device=0, lib_path=lib_path)) > 1
    tot = _check_set(prefix, k, n, lib_path)
    print("B2 %s k=%d: %d weak anchors at the default insert size, %d at %d" % (os.path.basename(prefix), k, tot[0], tot[1], 4 * k))
    assert tot[1] >= 50
    monkeypatch.setenv("RTK_INEXACT_ENUM", "1")
    assert _check_set(prefix, k, n, lib_path) == tot
    monkeypatch.delenv("RTK_INEXACT_ENUM")
    monkeypatch.setenv("RTK_HX_MAX_GB", "0")
    assert _hx_words(api.Graph(fa, rt, k, device=0, lib_path=lib_path)) == 1
    assert _check_set(prefix, k, n, lib_path) == tot
    monkeypatch.delenv("RTK_HX_MAX_GB")
    # [A2] in the order insertion -> deletion -> substitution: the kinds of edit the enumerating search attaches to its variants decide which hits stay
    monkeypatch.setenv("RTK_A2_XOR", "exclusive-ids")
    t2 = _check_set(prefix, k, n, lib_path)
    monkeypatch.setenv("RTK_INEXACT_ENUM", "1")
    assert _check_set(prefix, k, n, lib_path) == t2
    monkeypatch.delenv("RTK_INEXACT_ENUM"); monkeypatch.delenv("RTK_A2_XOR")


def test_sim_other_k_three_ways_k25(ds_k25, monkeypatch):
    _check_three_ways(ds_k25, 25, 6, SIM_LIB, monkeypatch)


def test_sim_other_k_three_ways_k21(ds_k21, monkeypatch):
    _check_three_ways(ds_k21, 21, 16, SIM_LIB, monkeypatch)


def test_sim_other_k_three_ways_tandem(ds_tandem, monkeypatch):
    _check_three_ways(ds_tandem, 31, 6, SIM_LIB, monkeypatch)


@pytest.mark.gpu
def test_gpu_other_k_three_ways_k25(ds_k25, monkeypatch):
    _check_three_ways(ds_k25, 25, 6, None, monkeypatch)


@pytest.mark.gpu
def test_gpu_other_k_three_ways_k21(ds_k21, monkeypatch):
    _check_three_ways(ds_k21, 21, 16, None, monkeypatch)


@pytest.mark.gpu
def test_gpu_other_k_three_ways_tandem(ds_tandem, monkeypatch):
    _check_three_ways(ds_tandem, 31, 16, None, monkeypatch)


def _index_of(tmp, name, seqs, k, step=6, reps=1):
    """error-free 100-base reads tiling `seqs` at `step`-base steps, indexed at k; returns the prefix"""
    pre = os.path.join(str(tmp), name)
    with open(pre + ".sr.fq", "w") as f:
        n = 0
        for rep in range(reps):
            for s in seqs:
                for start in list(range(0, len(s) - 100, step)) + [len(s) - 100]:
                    f.write("@r%d\n%s\n+\n%s\n" % (n, s[start:start + 100], "I" * 100)); n += 1
    subprocess.check_call([os.path.join(BIN, "rtk_build_index"), "-s", pre + ".sr.fq", "-o", pre, "-k", str(k)], stderr=subprocess.DEVNULL)
    return pre


def _edit(s, at, kind, rnd):
    """one edit of the read s at `at`: 0 substitution, 1 inserted base, 2 deleted base"""
    if kind == 0:
        return s[:at] + rnd.choice([c for c in "ACGT" if c != s[at]]) + s[at + 1:]
    if kind == 1:
        return s[:at] + rnd.choice("ACGT") + s[at:]
    return s[:at] + s[at + 1:]


def _lone_edit(s, w0, k, at, kind, rnd):
    """The read s with ONE edit at `at` inside its window [w0, w0 + k) and a substitution two characters in front of and two behind that window. Without the
    two the edit would never be searched: the mask opens, between two exact hits, only the characters that neither hit's k-mer covers (src/Graph.cpp:102-191),
    and the 1-edit search needs k - 1 open characters for a window; a lone edit leaves k - 1 .. k + 1 windows without a hit and ONE open character. With
    them no window that touches [w0, w0 + k) has a hit, the whole stretch is opened (given an insert size the gap reaches), and the windows that hold
    nothing but the edit at `at` are one edit away from the graph."""
    assert w0 <= at < w0 + k
    for p, kd in ((w0 + k + 1, 0), (at, kind), (w0 - 2, 0)):  # from the right: positions to the left stay where they are
        if 0 <= p < len(s):
            s = _edit(s, p, kd, rnd)
    return s


_N_PALIN = 40


def _palindrome_case(tmp, k):
    """A 6 kb random genome with _N_PALIN palindromic h-mers (equal to their own reverse complement; h = (k - 1) / 2 is even at k = 25 and k = 21) planted 3 k
    and more apart, and the reads: a stretch of the genome around a planted site with one edit -- substitution, inserted base, deleted base in turn
    -- in the half of the covering window that does NOT hold the planted h-mer (and the two substitutions of _lone_edit outside that window), one read with the edit on the left of the site and one with it on the
    right, each on both strands (a place of a palindromic h-mer is a place of both orientations: which of the two the search needs depends on the strand
    the unitig was written on). Returns (prefix, [(read, read position of the edit)] forward strand, the same reads reverse-complemented)."""
    h = (k - 1) // 2
    assert h % 2 == 0
    rnd = random.Random(1000 + k)
    g = [rnd.choice("ACGT") for _ in range(6000)]
    sites = [150 + i * ((6000 - 300) // _N_PALIN) for i in range(_N_PALIN)]
    assert sites[1] - sites[0] >= 3 * k + h
    for p in sites:
        half = "".join(rnd.choice("ACGT") for _ in range(h // 2))
        g[p:p + h] = half + _rc(half)
    g = "".join(g)
    for p in sites:
        assert g[p:p + h] == _rc(g[p:p + h])
    fwd, kind = [], 0
    for p in sites:
        lo, hi = p - 70, p + h + 70
        # in the first half of the window that ENDS with the planted h-mer / in the second half of the one that STARTS with it
        for w0, at in ((p + h - k, p - 2 - h // 2), (p, p + h + 1 + h // 2)):
            fwd.append((_lone_edit(g[lo:hi], w0 - lo, k, at - lo, kind % 3, rnd), at - lo)); kind += 1
    return _index_of(tmp, "palin%d" % k, [g], k), fwd, [(_rc(s), len(s) - 1 - at) for s, at in fwd]


def _check_palindromes(tmp, k, lib_path, monkeypatch):
    """Insert size k: the stretch without exact hits around the edit is some 2 k windows long, and the mask opens a gap for the 1-edit search only from half
    the insert size on (from the whole of it on without asking the colours) -- at the default 500 no such read would be searched at all."""
    pre, fwd, rev = _palindrome_case(tmp, k)
    og, pg = _graphs(pre, k, lib_path)
    oo, po = og.opts(insert_sz=k), pg.opts(insert_sz=k)
    for name, reads in (("forward", fwd), ("reverse", rev)):
        want = [og.seeds(s, oo) for s, _ in reads]
        # non-vacuity: sites where the oracle keeps a weak anchor whose k-mer window covers the edit
        n_sites = sum(1 for (s, at), w in zip(reads, want) if any(a[0] <= at + 1 and at - 1 < a[0] + k for a in w[1]))
        print("B2 palindromes k=%d %s strand: weak anchor over the edit at %d of %d sites" % (k, name, n_sites, len(reads)))
        assert len(reads) == 2 * _N_PALIN and n_sites >= 30
        for enum in (False, True):
            if enum:
                monkeypatch.setenv("RTK_INEXACT_ENUM", "1")
            got = _batch_seeds(pg, [s for s, _ in reads], po)
            monkeypatch.delenv("RTK_INEXACT_ENUM", raising=False)
            for i, (g_, w) in enumerate(zip(got, want)):
                assert g_ == w, (k, name, "enumerating" if enum else "half-k-mer", i)
        for i in range(0, len(reads), 9):  # the single-read entry as well
            assert pg.seeds(reads[i][0], po) == want[i]


@pytest.mark.parametrize("k", [25, 21])
def test_sim_palindromic_half_kmers(tmp_path, monkeypatch, k):
    _check_palindromes(tmp_path, k, SIM_LIB, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 21])
def test_gpu_palindromic_half_kmers(tmp_path, monkeypatch, k):
    _check_palindromes(tmp_path, k, None, monkeypatch)


# ------------------------------------------------------------------------------------------------ B3: the table, asked about itself
def _constructed_graph(tmp, k=31):
    """Hand-made graph: two sequences that share exactly k bases (a unitig of ONE k-mer: two ways in, two ways out), two that share k + 1 (two k-mers), a
    hairpin W + reverse complement of W, and plain flanks"""
    rnd = random.Random(77)
    rs = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))

    def pair(shared):  # different characters on both sides of the shared stretch
        a, b = rs(220), rs(220)
        return [a + "A" + shared + "C" + b, rs(220) + "G" + shared + "T" + rs(220)]

    w = rs(300)
    seqs = pair(rs(k)) + pair(rs(k + 1)) + [w + _rc(w)]
    return _index_of(tmp, "built", seqs, k, step=5, reps=3)


def _unitigs(og):
    return [og.unitig(u)["seq"] for u in range(og.n_unitigs)]


def _hit(u, d, strand):
    return (u << 33) | (d << 1) | strand


def _check_table_both_strands(og, pg, k):
    """(a) every k-mer of the graph, as its unitig spells it and reverse-complemented"""
    us = _unitigs(og)
    for u, s in enumerate(us):
        n = len(s) - k + 1
        f, r = pg.lookup_exact(s), pg.lookup_exact(_rc(s))
        assert f == og.exact(s) and r == og.exact(_rc(s)), u
        assert f == [_hit(u, d, 1) for d in range(n)], u
        if _rc(s) != s:
            assert r == [_hit(u, n - 1 - d, 0) for d in range(n)], u
    return us


def _check_neighbours(og, pg, k, us):
    """(b) the 3 k one-substitution neighbours of every 7th k-mer of the graph, looked up in strings of neighbours separated by N"""
    kmers = [s[d:d + k] for s in us for d in range(len(s) - k + 1)][::7]
    n_var = n_miss = 0
    for at in range(0, len(kmers), 400):
        var = [km[:i] + c + km[i + 1:] for km in kmers[at:at + 400] for i in range(k) for c in "ACGT" if c != km[i]]
        text = "N".join(var)
        want = og.exact(text)
        assert pg.lookup_exact(text) == want, at
        n_var += len(var); n_miss += sum(1 for j in range(len(var)) if want[j * (k + 1)] < 0)
    print("B3 neighbours: %d of %d one-substitution neighbours of %d k-mers are not in the graph" % (n_miss, n_var, len(kmers)))
    assert n_var == 3 * k * len(kmers) and n_miss >= 0.95 * n_var
    return n_miss, n_var


def _check_short_and_n(og, pg, k, us):
    """(c) strings of k - 1, k and k + 1 characters; N at the first and the last character of a window and at the two characters behind it; lower case"""
    s = max(us, key=len)
    assert len(s) >= k + 8
    for n in (0, 1, k - 1, k, k + 1):
        assert pg.lookup_exact(s[:n]) == og.exact(s[:n]) and len(pg.lookup_exact(s[:n])) == max(0, n - k + 1)
    assert pg.lookup_exact(s[:k]) == [_hit(us.index(s), 0, 1)]
    for at in (0, k - 1, k, k + 1):
        t = s[:at] + "N" + s[at + 1:k + 8]
        got = pg.lookup_exact(t)
        assert got == og.exact(t), at
        assert all((h < 0) == (p <= at < p + k) for p, h in enumerate(got)), at
    assert pg.lookup_exact(s[:k + 8].lower()) == og.exact(s[:k + 8]) == pg.lookup_exact(s[:k + 8])  # (upper-cased by the entry, as the worker does: src/Ratatosk.cpp:814)


def _end_reads(us, k, which, rnd):
    """(d) For unitig u on either strand: its last 2 k bases (lengthened to the left by the unitig in front when it is shorter) followed by up to 2 k bases of a
    unitig that follows it, with one substitution / inserted base / deleted base at each offset of the unitig's LAST window (_lone_edit). The first
    window of u is the last one of its reverse complement."""
    by_prefix = {}
    for s in us:
        for t in (s, _rc(s)):
            by_prefix.setdefault(t[:k - 1], []).append(t)
    reads = []
    for u in which:
        for t in (us[u], _rc(us[u])):
            nxt = by_prefix.get(t[-(k - 1):], [])
            prv = by_prefix.get(_rc(t)[-(k - 1):], [])  # (what follows the reverse complement stands in front)
            left = _rc(prv[0])[:-(k - 1)][-2 * k:] if prv and len(t) < 2 * k else ""
            body = left + t[-2 * k:] + (nxt[0][k - 1:3 * k - 1] if nxt else "")
            w0 = len(left) + len(t[-2 * k:]) - k  # the unitig's last window in the read
            for off in range(k):
                for kind in range(3):
                    reads.append(_lone_edit(body, w0, k, w0 + off, kind, rnd))
    return reads


def _check_unitig_ends(og, pg, k, us, which, monkeypatch, tag):
    """Insert size k, as for the palindromes: the gap a lone edit leaves is then opened. The reads go through ONE batch per mode (thousands of reads: a batch of
    one each would take minutes) and every 41st through the single-read entry as well."""
    reads = _end_reads(us, k, which, random.Random(9))
    oo, po = og.opts(insert_sz=k), pg.opts(insert_sz=k)
    want = [og.seeds(s, oo) for s in reads]
    n_weak = sum(1 for w in want if w[1])
    print("B3 unitig ends %s: %d reads, %d with a weak anchor" % (tag, len(reads), n_weak))
    assert n_weak >= len(reads) // 4
    for enum in (False, True):
        if enum:
            monkeypatch.setenv("RTK_INEXACT_ENUM", "1")
        got = _batch_seeds(pg, reads, po)
        single = [pg.seeds(reads[i], po) for i in range(0, len(reads), 41)]
        monkeypatch.delenv("RTK_INEXACT_ENUM", raising=False)
        for i, (g_, w) in enumerate(zip(got, want)):
            assert g_ == w, (tag, "enumerating" if enum else "half-k-mer", i, reads[i])
        assert single == want[::41]


def _check_table_constructed(tmp, lib_path, monkeypatch):
    k = 31
    pre = _constructed_graph(tmp, k)
    og, pg = _graphs(pre, k, lib_path)
    us = _check_table_both_strands(og, pg, k)
    lens = sorted(len(s) for s in us)
    assert k in lens and k + 1 in lens, lens  # the unitig of one k-mer and the one of two
    _check_neighbours(og, pg, k, us)
    _check_short_and_n(og, pg, k, us)
    _check_unitig_ends(og, pg, k, us, range(len(us)), monkeypatch, "constructed")


def _check_table_small(prefix, lib_path):
    k = 31
    og, pg = _graphs(prefix, k, lib_path)
    us = _check_table_both_strands(og, pg, k)
    _check_neighbours(og, pg, k, us)
    _check_short_and_n(og, pg, k, us)


def _check_ends_small(prefix, lib_path, monkeypatch):
    k = 31
    og, pg = _graphs(prefix, k, lib_path)
    us = _unitigs(og)
    which = random.Random(4).sample(range(len(us)), min(50, len(us)))
    _check_unitig_ends(og, pg, k, us, which, monkeypatch, "ds_small")


def test_sim_table_constructed_graph(tmp_path, monkeypatch):
    _check_table_constructed(tmp_path, SIM_LIB, monkeypatch)


def test_sim_table_branching(ds_small):
    _check_table_small(ds_small, SIM_LIB)


def test_sim_unitig_ends_branching(ds_small, monkeypatch):
    _check_ends_small(ds_small, SIM_LIB, monkeypatch)


@pytest.mark.gpu
def test_gpu_table_constructed_graph(tmp_path, monkeypatch):
    _check_table_constructed(tmp_path, None, monkeypatch)


@pytest.mark.gpu
def test_gpu_table_branching(ds_small):
    _check_table_small(ds_small, None)


@pytest.mark.gpu
def test_gpu_unitig_ends_branching(ds_small, monkeypatch):
    _check_ends_small(ds_small, None, monkeypatch)


# ------------------------------------------------------------------------------------------------ B4: odd insert sizes
def _boundary_reads(prefix, insert_sz, k=31, seed=8):
    """Reads whose first hit and last hit lie AT half the insert size, one window either way: random characters in front of / behind a stretch of the
    reference (head and tail rule of the mask)."""
    rnd = random.Random(seed)
    junk = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    ref = _ref_text(prefix)
    reads = []
    for rep in range(4):
        a = 1000 + 2500 * rep
        for d in range(-2, 3):
            h = insert_sz // 2 + d
            reads.append(junk(h) + ref[a:a + 300])                      # head rule: the first hit at h (or a window later)
            reads.append(ref[a:a + 300] + junk(h - k))                  # tail rule: h characters behind the start of the last hit
    return reads


def _gap_boundary_reads(og, prefix, insert_sz, k=31, seed=12):
    """Reads with ONE gap of `diff` windows between two exact hits, diff = half the insert size and the whole of it, one window either way (the gap rules of
    the mask, src/Graph.cpp:102-191): 200 characters of the reference, diff - k near-miss characters (_near_miss) of the reference at a far place, 200
    characters of the reference at a third. The mask opens exactly the characters between the two hits' k-mers: the filling. Its windows have no exact hit
    but lie one edit away from the graph, so that whether the gap was opened shows in the weak anchors (random filling would give none either way). The
    sides are far apart and share no colour: the colour rule opens the gap wherever it is asked. The read's first hit is its first window and its last
    hit its last one: head and tail rule do nothing. Returns [(read, diff)]."""
    rnd = random.Random(seed)
    ref = _ref_text(prefix)
    h, reads = insert_sz // 2, []
    for rep in range(3):
        a, b, c = 1500 + 2100 * rep, 16000 + 2100 * rep, 9000 + 2100 * rep
        for diff in (h - 1, h, h + 1, insert_sz - 1, insert_sz, insert_sz + 1):
            for c2 in range(c, c + 2000, 97):  # the first place whose filling leaves the hits where they are meant to be
                fill = _near_miss(ref[c2:c2 + diff - k], rnd)
                if fill[0] == ref[a + 200]:  # (a filling that goes on as the reference does would move the hit that bounds the gap)
                    fill = _edit(fill, 0, 0, rnd)
                if fill[-1] == ref[b - 1]:
                    fill = _edit(fill, len(fill) - 1, 0, rnd)
                s = ref[a:a + 200] + fill + ref[b:b + 200]
                # hits at every window of the two sides, none between them: the gap is diff windows long
                if [p for p, x in enumerate(og.exact(s)) if x >= 0] == list(range(0, 200 - k + 1)) + list(range(200 - k + diff, len(s) - k + 1)):
                    break
            else:
                raise AssertionError("no filling for a gap of %d windows" % diff)
            reads.append((s, diff))
    return reads


def _reach_reads(og, prefix, insert_sz, ssl=100, k=31, seed=14):
    """Reads whose gap is opened or not by ONE position of the colour rule's reach, insert_sz - diff (src/Graph.cpp:128-160): the colours left of a gap are
    those of the non-branching unitigs with a hit at most that many windows in front of it. At an arm of a bubble -- a unitig of exactly k k-mers along the
    reference, non-branching, followed by the branching unitig the two arms run into -- the read goes on for `ssl` windows behind the arm's last k-mer, then
    comes a near-miss filling that makes a gap of insert_sz - ssl windows, then the reference from the arm's FIRST k-mer on. With a reach of ssl the left side
    has hits on the branching unitig alone and no colour: opened. One position more reaches the arm, which shares all its colours with itself on the
    right: not opened."""
    rnd = random.Random(seed)
    ref = _ref_text(prefix)
    ex = og.exact(ref)
    runs, i = [], 0  # (first window, windows, unitig) of every run of hits on one unitig
    while i < len(ex):
        j = i
        while ex[i] >= 0 and j + 1 < len(ex) and ex[j + 1] >= 0 and (ex[j + 1] >> 33) == (ex[i] >> 33):
            j += 1
        if ex[i] >= 0:
            runs.append((i, j - i + 1, ex[i] >> 33))
        i = j + 1
    reads = []
    for (s0, n0, u0), (s1, n1, u1) in zip(runs, runs[1:]):
        if n0 == k and s1 == s0 + k and n1 >= ssl + 5 and s0 > 300 and len(reads) < 12:
            q, c = s0 + k - 1, (s0 + len(ref) // 2) % (len(ref) - 600)
            reads.append(ref[q - 250:q + ssl + k] + _near_miss(ref[c:c + insert_sz - ssl - k], rnd) + ref[s0:s0 + 200])
    return reads


def _check_gap_reach(og, pg, prefix, insert_sz, segs, monkeypatch):
    """-> the number of _reach_reads whose anchors the oracle changes when the reach grows by one: at insert_sz + 1 the gap, of a length well inside
    (insert_sz / 2, insert_sz) either way, is looked at one position further"""
    reads = _reach_reads(og, prefix, insert_sz)
    if not reads:  # (a graph without bubbles)
        return 0
    want = [og.seeds(s, og.opts(insert_sz=insert_sz)) for s in reads]
    n_diff = sum(1 for s, w in zip(reads, want) if og.seeds(s, og.opts(insert_sz=insert_sz + 1)) != w)
    for seg in segs:
        monkeypatch.setenv("RTK_MASK_SEG", seg)
        got = _batch_seeds(pg, reads, pg.opts(insert_sz=insert_sz))
        for i, (g_, w) in enumerate(zip(got, want)):
            assert g_ == w, (prefix, insert_sz, seg, i)
    monkeypatch.delenv("RTK_MASK_SEG")
    return n_diff


def _check_gap_thresholds(og, pg, prefix, insert_sz, segs, monkeypatch, k=31):
    """The gap rules at their two thresholds: `diff >= insert_sz / 2` asks the colours, `diff >= insert_sz` opens without asking. With min_cov_vertices = 0
    the colour rule never opens (no intersection is smaller than 0), and the second threshold shows by itself."""
    reads = _gap_boundary_reads(og, prefix, insert_sz)
    h = insert_sz // 2
    seqs = [s for s, _ in reads]
    for mcv in (None, 0):
        kw = dict(insert_sz=insert_sz) if mcv is None else dict(insert_sz=insert_sz, min_cov_vertices=0)
        want = [og.seeds(s, og.opts(**kw)) for s in seqs]
        # non-vacuity, on these reads alone: one insert size up, half of it is h + 1 and the whole of it insert_sz + 1 -- the gaps of exactly h (with the
        # colours) and of exactly insert_sz windows (without them) are no longer opened, and the oracle's anchors change
        kw1 = dict(kw, insert_sz=insert_sz + 1)
        edge = h if mcv is None else insert_sz
        n_edge = sum(1 for (s, diff), w in zip(reads, want) if diff == edge and og.seeds(s, og.opts(**kw1)) != w)
        n_open = sum(1 for (s, diff), w in zip(reads, want) if any(200 <= a[0] < 200 + diff - 2 * k for a in w[1]))
        print("B4 %s insert size %d, min_cov_vertices %s: %d of 3 gaps of %d windows change their anchors at insert size %d; weak anchors inside %d of %d gaps"
              % (os.path.basename(prefix), insert_sz, "default" if mcv is None else "0", n_edge, edge, insert_sz + 1, n_open, len(reads)))
        assert n_edge == 3 and n_open == (15 if mcv is None else 6)  # opened: from h on with the colours (5 of the 6 lengths), from insert_sz on without (2 of 6)
        for seg in segs:
            monkeypatch.setenv("RTK_MASK_SEG", seg)
            got = _batch_seeds(pg, seqs, pg.opts(**kw))
            for i, (g_, w) in enumerate(zip(got, want)):
                assert g_ == w, (prefix, insert_sz, mcv, seg, "gap of %d windows" % reads[i][1])
        monkeypatch.delenv("RTK_MASK_SEG")


def _check_odd_insert_sizes(prefixes, reps, segs, lib_path, monkeypatch):
    for insert_sz in (499, 501):
        _check_gap_reads(prefixes, reps, segs, lib_path, monkeypatch, opts=dict(insert_sz=insert_sz))
        n_reach = 0
        for prefix in prefixes:
            og, pg = _graphs(prefix, 31, lib_path)
            reads = _boundary_reads(prefix, insert_sz)
            oo, po = og.opts(insert_sz=insert_sz), pg.opts(insert_sz=insert_sz)
            want = [og.seeds(s, oo) for s in reads]
            # non-vacuity: the reads sit on the thresholds -- the oracle one insert size up (half of it: 250 for 249, 251 for 250) keeps other anchors
            other = [og.seeds(s, og.opts(insert_sz=insert_sz + 1)) for s in reads]
            n_diff = sum(1 for a, b in zip(want, other) if a != b)
            print("B4 %s insert size %d: %d of %d boundary reads change their anchors at %d" % (os.path.basename(prefix), insert_sz, n_diff, len(reads), insert_sz + 1))
            assert n_diff >= 3
            for seg in segs:
                monkeypatch.setenv("RTK_MASK_SEG", seg)
                got = _batch_seeds(pg, reads, po)
                for i, (g_, w) in enumerate(zip(got, want)):
                    assert g_ == w, (prefix, insert_sz, seg, i)
            monkeypatch.delenv("RTK_MASK_SEG")
            _check_gap_thresholds(og, pg, prefix, insert_sz, segs, monkeypatch)
            n_reach += _check_gap_reach(og, pg, prefix, insert_sz, segs, monkeypatch)
        print("B4 insert size %d: one position of the colour rule's reach changes the anchors of %d reads" % (insert_sz, n_reach))
        assert n_reach >= 5


def _check_hits_closer_than_k(tmp, lib_path):
    """Insert sizes below 2 k (`-i`): the gap rules then let through two exact hits FEWER than k windows apart -- a deleted base inside a run of equal bases
    leaves k - 1 - (the rest of the run) windows without a hit. The reference's length of the opened stretch, diff - k, wraps around there and
    std::string::replace cuts it off at the end of the read (src/Graph.cpp:115,124,182): everything behind the first hit's k-mer is opened."""
    k = 31
    og, pg = _graphs(_constructed_graph(tmp, k), k, lib_path)
    reads = []
    for s in _unitigs(og):
        for t in (s, _rc(s)):
            runs = [at for at in range(k, min(len(t) - k, 3 * k)) if t[at] == t[at + 1]]
            reads += [t[:at] + t[at + 1:at + 3 * k] for at in runs[:6]]
    assert len(reads) >= 30
    n_close = 0
    for insert_sz in (1, 2, 20, k, 40, 2 * k - 2, 2 * k):
        oo, po = og.opts(insert_sz=insert_sz), pg.opts(insert_sz=insert_sz)
        want = [og.seeds(s, oo) for s in reads]
        for s in reads:  # non-vacuity: pairs of neighbouring exact hits that pass the size test of the gap rules with fewer than k windows between them
            at = [p for p, h in enumerate(og.exact(s)) if h >= 0]
            n_close += sum(1 for a, b in zip(at, at[1:]) if 1 < b - a < k and b - a >= insert_sz // 2)
        got = _batch_seeds(pg, reads, po)
        for i, (g_, w) in enumerate(zip(got, want)):
            assert g_ == w, (insert_sz, i, reads[i])
    print("B4 hits closer than k: %d gaps of fewer than k windows went through the gap rules" % n_close)
    assert n_close >= 100


def test_sim_mask_hits_closer_than_k(tmp_path):
    _check_hits_closer_than_k(tmp_path, SIM_LIB)


@pytest.mark.gpu
def test_gpu_mask_hits_closer_than_k(tmp_path):
    _check_hits_closer_than_k(tmp_path, None)


def test_sim_mask_odd_insert_sizes(ds_clean, ds_small, monkeypatch):
    _check_odd_insert_sizes((ds_clean, ds_small), 1, ("64", "8192"), SIM_LIB, monkeypatch)


@pytest.mark.gpu
def test_gpu_mask_odd_insert_sizes(ds_clean, ds_small, monkeypatch):
    _check_odd_insert_sizes((ds_clean, ds_small), 1, ("4096", "8192"), None, monkeypatch)
