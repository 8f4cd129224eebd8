"""k_inexact with one index look-up per read position of a tile, shared by the windows that ask for it (rtk_inexact_tile_seeded, csrc/hip/rtk_seed_seeded.h), and
with the window codes taken from the tile's bit planes: the places where the two can go wrong, against the oracle (`op.Graph(...).seeds`). Every comparison of
anchors is exact equality of Batch.seeds(i), under the default, RTK_INEXACT_SHARED=0, RTK_INEXACT_PLANES=0 and RTK_INEXACT_ENUM=1, at [A2] = union, exclusive and
exclusive-ids, at k = 31, 25 and 21. One batch per k (a 9 kb genome, some 250 reads), placed so that
  T1  a one-edit window stands at tile position 0, 63 and at each of the last k + 1 - h positions of a tile: its seeds 1 .. 3 come from the overhang positions behind
      the tile, which the low lanes look up. Every such read is a one-edit stretch directly beside masked characters ('N' of the masked copy on either side)
  T2  reads end exactly at a tile's end and 1, k-1-h, k-h, k+1-h, k+2-h characters past it, on a one-edit stretch: their last windows have k and k + 1 usable
      characters (3 and 4 seeds), and with an 'N' as the read's last character k - 1 (2 seeds)
  T3  two reads meet inside the overhang of the tile before: the first ends on a window that would be one edit away from the graph with ONE more character, the second
      starts with that character, in an opened head. No anchor may come of it (and read boundaries inside a tile are everywhere in the batch)
  T4  an 'N', and a lower-case letter, at each of the k + 1 positions of a one-edit window in turn
  T5  k = 25, 21 (even h): planted palindromic h-mers next to the edit, both strands; the position of the h-mer is asked for by neighbouring windows of one tile
  T6  a window with six distinct one-substitution neighbours in the graph: more than RTK_SEED_REGS hits, the route that visits the window three times
Counters (rtk_stats): n_hits_inexact equal under the four settings; n_probes_inexact under the default smaller than with RTK_INEXACT_SHARED=0; on the device, the three
inexact counters equal to the simulator's on the same batch and the same (host-built) index."""
import random

import pytest

from conftest import SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api
from test_seed_edges import _edit, _index_of, _lone_edit, _rc, _starts

SETTINGS = (("default", {}), ("RTK_INEXACT_SHARED=0", {"RTK_INEXACT_SHARED": "0"}), ("RTK_INEXACT_PLANES=0", {"RTK_INEXACT_PLANES": "0"}),
            ("RTK_INEXACT_ENUM=1", {"RTK_INEXACT_ENUM": "1"}))
A2 = ((0, "union"), (1, None), (2, "exclusive-ids"))  # a2_exclusive, RTK_A2_XOR (read by the oracle and by rtk_opts_default)
COUNTERS = ("n_probes_inexact", "n_slots_inexact", "n_hits_inexact")
N_PALIN = 12
N_FAMILY = 6


def _genome(k, rnd):
    """9 kb of random sequence; behind it N_FAMILY copies of a stretch Q of k + 4 characters, each in flanks of its own and each with ONE substitution, at the
    characters 4 .. 9 of Q in turn: Q itself is not in the graph, each of its five windows holds all six positions and has six one-substitution neighbours there.
    (None of the six is the middle character of a window, h <= 9 at no k used here: a neighbour that keeps BOTH halves of the window is reached through two seeds, and
    a window with more than RTK_SEED_REGS hits counts its visits, not its distinct hits, in n_hits_inexact -- the enumerating search would count one less.)
    At even h, N_PALIN palindromic h-mers are planted 3 k and more apart in the first 6 kb. -> (sequences to index, Q, palindrome sites)"""
    h = (k - 1) // 2
    g = [rnd.choice("ACGT") for _ in range(9000)]
    sites = []
    if h % 2 == 0:
        sites = [200 + i * (5600 // N_PALIN) for i in range(N_PALIN)]
        for p in sites:
            half = "".join(rnd.choice("ACGT") for _ in range(h // 2))
            g[p:p + h] = half + _rc(half)
    g = "".join(g)
    rs = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    q = rs(k + 4)
    fam = [rs(150) + _edit(q, 4 + i, 0, rnd) + rs(150) for i in range(N_FAMILY)]
    return [g] + fam, q, sites


def _reads(k, seqs, q, sites, rnd):
    """-> [(tag, read, offset in the read to place, tile residue to place it at)] (None, None: wherever it falls)"""
    g = seqs[0]
    h = (k - 1) // 2
    d1, d3 = k - 1 - h, k + 1 - h
    out = []
    at_of = (h // 2, k // 2, k - 1 - h // 2)  # the edit in the first half, at the middle character, in the second half of the window
    n = 0
    for x in [0] + list(range(64 - d3, 64)):  # T1
        a = 300 + 97 * n
        body = g[a - 70:a + k + 70]
        out.append(("T1 tile position %d" % x, _lone_edit(body, 70, k, 70 + at_of[n % 3], n % 3, rnd), 70, x)); n += 1
    for e in (0, 1, d1, d1 + 1, d3, d3 + 1):  # T2: the read's END at residue e
        for kind in (0, 1, 2):
            a = 2500 + 113 * n; n += 1
            s = _edit(g[a:a + 150], 150 - k + at_of[n % 3], kind, rnd)
            out.append(("T2 end %d past a tile" % e, s, len(s), e))
            out.append(("T2 end %d past a tile, N" % e, s[:-1] + "N", len(s), e))
    for j in (1, d1, d3 - 1):  # T3: the boundary at residue j, inside the overhang of the tile before
        a = 5200 + 400 * (n % 3); n += 1
        # a base too many in window 100 of the joined text (_lone_edit: substitutions at 98 and, behind the inserted base, at 102 + k), and the cut behind the k characters
        # of that window: with the character behind the cut the window is the graph's k-mer with a read base too many, without it it is nothing. A second substitution
        # puts the second read's first hit behind half the insert size: its head is opened, and the character stands in the masked copy as it is.
        joined = _edit(_lone_edit(g[a:a + 330], 100, k, 100 + k // 2, 1, rnd), 101 + 2 * k, 0, rnd)
        out.append(("T3 first", joined[:100 + k], 100 + k, j))
        out.append(("T3 second", joined[100 + k:], None, None))
    a = 7000
    body = _lone_edit(g[a - 70:a + k + 70], 70, k, 70 + k // 2, 0, rnd)
    for i in range(k + 1):  # T4
        out.append(("T4 N at %d" % i, body[:70 + i] + "N" + body[71 + i:], None, None))
        out.append(("T4 lower case at %d" % i, body[:70 + i] + body[70 + i].lower() + body[71 + i:], None, None))
    kind = 0
    for p in sites:  # T5 (as test_seed_edges._palindrome_case)
        lo, hi = p - 70, p + h + 70
        for w0, at in ((p + h - k, p - 2 - h // 2), (p, p + h + 1 + h // 2)):
            s = _lone_edit(g[lo:hi], w0 - lo, k, at - lo, kind % 3, rnd); kind += 1
            out.append(("T5 palindrome", s, w0 - lo, 20))  # (window w0 and its neighbours, which ask for the same position, inside one tile)
            out.append(("T5 palindrome, other strand", _rc(s), None, None))
    for i in range(N_FAMILY):  # T6: Q between two stretches of the genome, hits on both sides and Q, nothing else, in the gap: the genome goes on with another character than Q's
        # first behind the left stretch and has another than Q's last in front of the right one (else the window with that character is a k-mer of the genome)
        a = next(x for x in range(800 + 300 * i, 1000 + 300 * i) if g[x + 60] != q[0])
        b = next(x for x in range(4000 + 300 * i, 4200 + 300 * i) if g[x - 1] != q[-1])
        out.append(("T6 family", g[a:a + 60] + q + g[b:b + 60], None, None))
    return out


def _place(items, rnd):
    """the reads of the batch in order, with a read of random characters in front of every read that has a place to be at"""
    reads, tags, cur = [], [], 0
    for tag, s, off, res in items:
        if off is not None:
            pad = (res - cur - off) % 64
            if pad:
                reads.append("".join(rnd.choice("ACGT") for _ in range(pad))); tags.append("pad"); cur += pad
            assert (cur + off) % 64 == res
        reads.append(s); tags.append(tag); cur += len(s)
    return reads, tags


def _run(pg, reads, env, monkeypatch, regions):
    """-> (anchors of every read, the inexact counters when the region stage ran: rtk_stats is filled at the end of a whole run)"""
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    b = api.Batch(pg, reads)
    try:
        b.run_seeds(pg.opts(insert_sz=pg.k))
        got = [b.seeds(i) for i in range(len(reads))]
        st = None
        if regions:
            b.run_regions(pg.opts(insert_sz=pg.k))
            st = {c: b.stats()[c] for c in COUNTERS}
    finally:
        b.close()
        for name in env:
            monkeypatch.delenv(name)
    return got, st


def _check(tmp, k, lib_path, monkeypatch, against_sim):
    rnd = random.Random(500 + k)
    seqs, q, sites = _genome(k, rnd)
    pre = _index_of(tmp, "shared%d" % k, seqs, k)
    fa, rt = pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k
    og, pg = op.Graph(fa, rt, k), api.Graph(fa, rt, k, device=0, lib_path=lib_path)
    h = (k - 1) // 2
    reads, tags = _place(_reads(k, seqs, q, sites, rnd), rnd)
    st0 = _starts(reads)
    print("k=%d: %d reads, %d bases" % (k, len(reads), sum(len(r) for r in reads)))
    stats = {}
    for mode, xor in A2:
        if xor:
            monkeypatch.setenv("RTK_A2_XOR", xor)
        assert pg.opts().a2_exclusive == mode
        memo = {}
        for r in reads:
            if r.upper() not in memo:
                memo[r.upper()] = og.seeds(r.upper(), og.opts(insert_sz=k))  # (insert size k: the gap a lone edit leaves is opened; the entries upper-case a read)
        want = [memo[r.upper()] for r in reads]
        # non-vacuity, from the oracle alone
        weak = lambda i: [a[0] for a in want[i][1]]
        t1 = [i for i, t in enumerate(tags) if t.startswith("T1")]
        n_t1 = sum(1 for i in t1 if any(70 - 3 <= p <= 70 + 3 for p in weak(i)))
        t2 = [i for i, t in enumerate(tags) if t.startswith("T2")]
        n_t2 = sum(1 for i in t2 if any(p >= len(reads[i]) - k - 3 for p in weak(i)))
        n_t4 = sum(1 for i, t in enumerate(tags) if t.startswith("T4") and weak(i))
        n_t5 = sum(1 for i, t in enumerate(tags) if t.startswith("T5") and weak(i))
        n_t6 = sum(1 for i, t in enumerate(tags) if t.startswith("T6") and any(60 <= p <= 64 for p in weak(i)))
        print("k=%d a2=%d: weak anchor at the placed window of %d of %d T1 reads, in the last windows of %d of %d T2 reads, in %d T4 reads, %d T5 reads, on Q in %d of %d T6 reads"
              % (k, mode, n_t1, len(t1), n_t2, len(t2), n_t4, n_t5, n_t6, N_FAMILY))
        assert len(t1) == k + 1 - h + 1 and n_t1 >= len(t1) // 2 and n_t2 >= len(t2) // 3 and n_t4 >= k // 2 and n_t5 >= len(sites) // 2
        for i, t in enumerate(tags):
            if t == "T3 first":  # the boundary lies in the overhang of the tile before, the joined text has an anchor the two reads must not have
                assert 0 < st0[i + 1] % 64 < k + 1 - h and tags[i + 1] == "T3 second"
                assert all(p < len(reads[i]) - k for p in weak(i)), "the oracle anchors the first read's last window"
        if mode == 1:
            joined = [og.seeds(reads[i] + reads[i + 1], og.opts(insert_sz=k))[1] for i, t in enumerate(tags) if t == "T3 first"]
            n_join = sum(1 for w in joined if any(100 <= a[0] < 100 + k for a in w))
            print("k=%d: the joined text of %d of %d T3 pairs has a weak anchor in a window the two reads do not have" % (k, n_join, len(joined)))
            assert len(joined) == 3 and n_join >= 1
        for name, env in SETTINGS:
            got, st = _run(pg, reads, env, monkeypatch, regions=(mode == 1))
            for i, (g_, w) in enumerate(zip(got, want)):
                assert g_ == w, (k, "a2=%d" % mode, name, tags[i], "read %d of the batch, %d bases, starts at %d (tile residue %d)" % (i, len(reads[i]), st0[i], st0[i] % 64))
            if st:
                stats[name] = st
                print("k=%d %s: %s" % (k, name, " ".join("%s=%d" % (c, st[c]) for c in COUNTERS)))
        if xor:
            monkeypatch.delenv("RTK_A2_XOR")
    # counters: the same hits under every setting; fewer look-ups when the windows of a tile share them (the batch is near-miss reads)
    assert len(set(st["n_hits_inexact"] for st in stats.values())) == 1, stats
    assert stats["default"]["n_hits_inexact"] >= 6 * 5 * N_FAMILY  # (T6 alone: five windows of Q with six neighbours each)
    assert stats["default"]["n_probes_inexact"] < stats["RTK_INEXACT_SHARED=0"]["n_probes_inexact"], stats
    assert stats["RTK_INEXACT_PLANES=0"]["n_probes_inexact"] == stats["default"]["n_probes_inexact"]
    # the family reads alone (every searched window has more than RTK_SEED_REGS hits): no more look-ups than the windows make on their own
    fam = [r for r, t in zip(reads, tags) if t.startswith("T6")]
    a, b = _run(pg, fam, {}, monkeypatch, True)[1], _run(pg, fam, {"RTK_INEXACT_SHARED": "0"}, monkeypatch, True)[1]
    assert a["n_hits_inexact"] == b["n_hits_inexact"] >= 6 * 5 * N_FAMILY and a["n_probes_inexact"] <= b["n_probes_inexact"], (a, b)
    if against_sim:  # simulator and device on the same batch and the same index image: built on the host by ONE thread. n_slots_inexact counts the slots of every probe chain,
        # and where colliding keys stand in the table follows the order in which the builder's lanes or threads arrive (the device's builder, and the host's with more
        # than one thread, give chains a slot longer or shorter from one load of the graph to the next; the look-ups and the hits do not depend on it)
        sg = api.Graph(fa, rt, k, device=0, lib_path=SIM_LIB, host_tables=True, n_threads=1)
        dg = api.Graph(fa, rt, k, device=0, lib_path=lib_path, host_tables=True, n_threads=1)
        s_got, s_st = _run(sg, reads, {}, monkeypatch, True)
        d_got, d_st = _run(dg, reads, {}, monkeypatch, True)
        print("k=%d simulator %s, device %s" % (k, s_st, d_st))
        assert s_got == d_got and s_st == d_st, (s_st, d_st)


@pytest.mark.parametrize("k", [31, 25, 21])
def test_sim_shared_lookups(tmp_path, monkeypatch, k):
    _check(tmp_path, k, SIM_LIB, monkeypatch, False)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 25, 21])
def test_gpu_shared_lookups(tmp_path, monkeypatch, k):
    _check(tmp_path, k, None, monkeypatch, True)
