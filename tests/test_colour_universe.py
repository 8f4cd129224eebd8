"""The universe of the colour selection's register program: its sort, its bit vectors, and the routes of real regions under the audit.

rtk_choose_colors_small (csrc/hip/rtk_colours.h, device only) gathers every id of every side unitig into LDS with the number of the list it came from (its
tag), sorts the entries by id once (rtk_radix_sort_tagged: as many passes as the largest id has bytes, odd or even; plain LDS adds for the histograms), and
reads universe and bit vectors off the sorted entries (rtk_colour_universe): an entry's rank is the number of run heads up to it, the vectors are
ceil(U / 64) words wide and lie in LDS behind the universe, and a call whose universe and vectors do not fit is handed on (n_colours_declined_fit). Ids below
2^26 carry their tag in the low six bits of their word; larger ones have it in a byte array moved with the words. Up to 512 entries both key buffers are in
LDS, above that the second one is in device memory.

Two operations of the stage entry rtk_sets_batch run those two routines on their own, in the layout of the register program, one problem per wavefront in
one launch (the simulator answers "not in this build"). References: sorted() on (id, input position) for the sort -- equal ids keep their input order and
every tag stays with its id -- and Python sets for the universe; a problem is expected to be declined exactly when U + 2 * lists * ceil(U / 64) > 2048 words
with more than 512 entries.

The routes: two sets whose calls spread over the sizes -- `all` at k = 21 (seed 105; counted on the MI355X before this file: small 809, wide 1230, general
188) and a 40 kb reference under 90x short reads at k = 31, where nearly every call has more than 512 entries and a few hundred have more than 512 distinct ids
(vectors of more than 8 words) -- each under the default setting, RTK_COLOURS_AUDIT=1 and the audit with its test hook. The oracle corrects each set once and
the simulator runs it once; both are shared by the tests of this file."""
import functools
import os
import subprocess

import numpy as np
import pytest

import hard_genomes as hg
import test_index_build as IB
from conftest import BIN, SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

SORT_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1663, 1664)
SORT_MAX_KEYS = (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 26) - 1, 1 << 26, 0xFFFFFFFE)  # one to four passes; 2^26: the tag leaves the word
PATTERNS = ("distinct", "twice", "equal", "few")
LDS_WORDS, SMALL_IDS, MAX_LISTS = 2048, 512, 48


def _keys(r, n, mk, pattern):
    if pattern == "equal" or mk == 0:
        return np.full(n, mk, dtype=np.uint32)  # (every add of a histogram lands on one counter)
    if pattern == "distinct":
        if mk + 1 >= 4 * n:
            s = set([mk])
            while len(s) < n:
                s.update(r.randint(0, mk + 1, size=n, dtype=np.int64).tolist())
            pool = np.array(sorted(s)[-n:] if n else [], dtype=np.int64)
        else:
            pool = mk - (np.arange(n, dtype=np.int64) % (mk + 1))  # as distinct as the range allows
        return r.permutation(pool).astype(np.uint32)
    if pattern == "twice":
        half = _keys(r, (n + 1) // 2, mk, "distinct").astype(np.int64)
        return r.permutation(np.concatenate([half, half])[:n]).astype(np.uint32)
    values = np.unique(np.concatenate([r.randint(0, mk + 1, size=min(300, mk + 1), dtype=np.int64), [mk]]))  # T / U about 2 to 5 at the larger sizes
    keys = values[r.randint(0, len(values), size=n)]
    if n:
        keys[r.randint(0, n)] = mk
    return keys.astype(np.uint32)


def _sort_problems(r):
    out = []
    for n in SORT_SIZES:
        for mk in SORT_MAX_KEYS:
            for pattern in PATTERNS:
                keys = _keys(r, n, mk, pattern)
                tags = r.randint(0, MAX_LISTS, size=n).astype(np.uint32)
                if n >= 2:
                    tags[0], tags[-1] = MAX_LISTS - 1, 0
                order = sorted(range(n), key=lambda i: int(keys[i]))  # stable
                out.append(("RADIX_TAGGED n=%d max_key=%d %s" % (n, mk, pattern), (api.SETS_RADIX_TAGGED, keys, tags, mk),
                            ("list", [int(keys[i]) for i in order] + [int(tags[i]) for i in order])))
    return out


def _universe_problem(name, lists, top=None):
    ids = [x for l in lists for x in l]
    uni = sorted(set(ids))
    rank = dict((x, i) for i, x in enumerate(uni))
    U, T, n = len(uni), len(ids), len(lists)
    VW = max(1, (U + 63) // 64)
    fits = T <= SMALL_IDS or U + 2 * n * VW <= LDS_WORDS
    vectors = [sorted(set(rank[x] for x in l)) for l in lists]
    scalar = max(ids + [0]) if top is None else top
    return ("COLOUR_UNIVERSE %s: %d lists, T=%d U=%d%s" % (name, n, T, U, "" if top is None else " ids up to %d" % top),
            (api.SETS_COLOUR_UNIVERSE, np.array(ids, dtype=np.uint32), np.array([len(l) for l in lists], dtype=np.uint32), scalar), ("universe", fits, uni, vectors))


def _spread(r, U, n_lists, T, hi):
    """n_lists sorted lists without repeats over U distinct ids below hi, T entries in all (U <= T <= U * n_lists): every id in at least one list"""
    s = set()
    while len(s) < U:
        s.update(r.randint(0, hi, size=U, dtype=np.int64).tolist())
    uni = sorted(s)[:U]
    lists = [set() for _ in range(n_lists)]
    for i, x in enumerate(uni):
        lists[i % n_lists].add(x)
    left = T - U
    while left:
        l, x = lists[r.randint(0, n_lists)], uni[r.randint(0, U)]
        if x not in l:
            l.add(x); left -= 1
    return [sorted(l) for l in lists]


def _universe_problems(r):
    out = []
    for hi, top in ((100000, None), (1 << 23, None), (0xFFFFFFFF, 0xFFFFFFFE)):  # three key bytes as on the measured sets; the tag beside the word
        for U in (1, 63, 64, 65, 511, 512):  # at most 512 entries
            out.append(_universe_problem("single", _spread(r, U, 1, U, hi), top))
            if U >= 6:
                out.append(_universe_problem("six lists", _spread(r, U, 6, min(SMALL_IDS, 2 * U), hi), top))
        for U in (63, 64, 65, 511, 512, 513):  # more than 512 entries: second key buffer in device memory, vectors of 1 .. 9 words
            n = max(12, (SMALL_IDS + U) // U + 1)
            out.append(_universe_problem("wide", _spread(r, U, n, max(SMALL_IDS + 1, 2 * U), hi), top))
        for U in (799, 800, 801, 802, 832, 833):  # 48 lists: 800 + 96 * 13 = 2048 words fit, 801 ids do not
            out.append(_universe_problem("fit bound", _spread(r, U, MAX_LISTS, U + 100, hi), top))
        out.append(_universe_problem("24 slots x 2, each id twice", _spread(r, 448, MAX_LISTS, 896, hi), top))
        out.append(_universe_problem("24 slots x 2, small", _spread(r, 448, MAX_LISTS, 448, hi), top))
        out.append(_universe_problem("24 slots x 2, all distinct", _spread(r, 1664, MAX_LISTS, 1664, hi), top))  # declined
        out.append(_universe_problem("2 lists, 26-word vectors", _spread(r, 1664, 2, 1664, hi), top))
        one = _spread(r, 300, 1, 300, hi)[0]
        out.append(_universe_problem("all lists equal", [list(one) for _ in range(5)], top))  # 1500 entries, 300 ids
        out.append(_universe_problem("all lists equal, small", [list(one[:100]) for _ in range(5)], top))
        d = _spread(r, 900, 9, 900, hi)
        out.append(_universe_problem("disjoint lists", d, top))
        out.append(_universe_problem("disjoint lists, small", [l[:50] for l in d], top))
        out.append(_universe_problem("an empty list in the middle", d[:3] + [[]] + d[3:6], top))
        out.append(_universe_problem("empty lists at both ends, small", [[]] + [l[:40] for l in d[:4]] + [[]], top))
        out.append(_universe_problem("only empty lists", [[], [], []], top))
    return out


@functools.lru_cache(maxsize=None)
def _problems():
    r = np.random.RandomState(20250308)
    return _sort_problems(r) + _universe_problems(r)


def _decode(words, n_lists):
    U, VW = words[0], words[1]
    uni, rest = words[2:2 + U], words[2 + U:]
    assert len(rest) == 2 * n_lists * VW
    vectors = []
    for t in range(n_lists):
        bits = []
        for w in range(VW):
            x = rest[2 * (t * VW + w)] | (rest[2 * (t * VW + w) + 1] << 32)
            bits += [64 * w + b for b in range(64) if (x >> b) & 1]
        vectors.append(bits)
    return U, VW, uni, vectors


def test_sim_answers_not_in_this_build():
    got = api.sets_batch([p for _, p, _ in _problems()], lib_path=SIM_LIB)
    assert all(st == api.SETS_NOT_IN_BUILD and words == [] for words, _, st in got)


@pytest.mark.gpu
def test_gpu_sort_and_universe():
    probs = _problems()
    got = api.sets_batch([p for _, p, _ in probs])
    assert len(got) == len(probs)
    bad, declined, widest = [], 0, 0
    for (name, (_, _, b, _), want), (words, res, st) in zip(probs, got):
        if want[0] == "list":
            ok = st == api.SETS_OK and words == want[1]
        else:
            _, fits, uni, vectors = want
            if not fits:
                declined += 1
                ok = st == api.SETS_DECLINED and words == [] and res == len(uni)
            else:
                ok = st == api.SETS_OK and res == len(uni)
                if ok:
                    U, VW, got_uni, got_vectors = _decode(words, len(b))
                    widest = max(widest, VW)
                    ok = U == len(uni) and VW == max(1, (U + 63) // 64) and got_uni == uni and got_vectors == vectors
        if not ok:
            bad.append("%s: status %d result %d, %s" % (name, st, res, str(words)[:100]))
    print("%d problems in one launch, %d declined, widest vector %d words" % (len(probs), declined, widest))
    assert not bad, "%d of %d problems differ from the reference, e.g. %s" % (len(bad), len(probs), bad[:8])
    assert declined >= 6 and widest == 26


def test_sets_batch_refuses_entries_the_layout_cannot_hold():
    for prob in ((api.SETS_RADIX_TAGGED, list(range(1665)), [0] * 1665, 1 << 20), (api.SETS_RADIX_TAGGED, [1, 2], [0, 48], 2), (api.SETS_RADIX_TAGGED, [1, 9], [0, 1], 8),
                 (api.SETS_RADIX_TAGGED, [1, 2], [0], 2), (api.SETS_RADIX_TAGGED, [1], [0], 0xFFFFFFFF), (api.SETS_COLOUR_UNIVERSE, [1, 2, 3], [2], 3),
                 (api.SETS_COLOUR_UNIVERSE, [1, 2, 3], [], 3), (api.SETS_COLOUR_UNIVERSE, list(range(49)), [1] * 49, 48), (api.SETS_COLOUR_UNIVERSE, [5], [1], 4)):
        with pytest.raises(api.RtkError):
            api.sets_batch([prob], lib_path=SIM_LIB)


# ---- the routes of real regions ----
AUDIT, FAULT, ROUTE = "RTK_COLOURS_AUDIT", "RTK_TEST_COLOURS_FAULT", "RTK_COLOURS_ROUTE"
SETTINGS = (("default", {}), ("audit", {AUDIT: "1"}), ("audit+fault", {AUDIT: "1", FAULT: "1"}))
ANSWERED = ("n_colours_small", "n_colours_wide", "n_colours_bits", "n_colours_general")
SETS = ("all-k21", "cov90-k31")


def _set_knobs(monkeypatch, env):
    for knob in (ROUTE, AUDIT, FAULT):
        monkeypatch.delenv(knob, raising=False)
    for knob, value in env.items():
        monkeypatch.setenv(knob, value)  # read on every call (rtk_knobs.h)


def _run(ref, lib, env, monkeypatch):
    fa, rt, k, seqs, quals, want = ref
    _set_knobs(monkeypatch, env)
    pg = api.Graph(fa, rt, k, device=0, lib_path=lib)
    b = api.Batch(pg, seqs, quals)
    b.run(pg.opts())
    got, st = b.fetch(), b.stats()
    b.close()
    _set_knobs(monkeypatch, {})
    assert [(g[0], g[1]) for g in got] == want, "%d reads differ from the oracle" % sum(1 for g, w in zip(got, want) if (g[0], g[1]) != w)
    return st


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """per set, made on first use: files, reads, the oracle's corrected reads, and the simulator's counters under the default setting"""
    made = {}

    def get(name, monkeypatch):
        if name not in made:
            tmp = str(tmp_path_factory.mktemp(name))
            if name == "all-k21":
                pre, k = os.path.join(tmp, "all"), 21
                hg.write_set(pre, seed=105, kind="all")
                IB._build(pre + ".sr.fq", pre, k, [])  # the plain tool with --snps
            else:
                pre, k = os.path.join(tmp, "c90"), 31
                subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "7", "--ref-len", "40000", "--het", "0.002", "--sr-cov", "0", "--lr-cov", "6",
                                       "--lr-len", "4000", "--lr-profile", "ont", "--lr-err", "0.07"], stderr=subprocess.DEVNULL)
                subprocess.check_call([os.path.join(BIN, "rtk_build_index"), "-s", "sample:%s.ref.fa?cov=90&len=150&insert=500&err=0.005&seed=2" % pre, "-o", pre, "--snps"],
                                      stderr=subprocess.DEVNULL)
            fa, rt = pre + ".index.k%d.fasta.gz" % k, pre + ".index.k%d.rtsk" % k
            reads = op.read_fastq(pre + ".lr.fq")
            seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
            want = [(w[0], w[1]) for w in op.Graph(fa, rt, k).correct_batch(seqs, quals, threads=8)[0]]
            ref = (fa, rt, k, seqs, quals, want)
            made[name] = (ref, _run(ref, SIM_LIB, {}, monkeypatch))
        return made[name]
    return get


def _report(where, name, setting, st):
    print("%s %s %s: %d regions; colour selections answered by small %d wide %d bits %d general %d; declined for room %d, audit mismatches %d" % (
        where, name, setting, st["n_regions"], st["n_colours_small"], st["n_colours_wide"], st["n_colours_bits"], st["n_colours_general"],
        st["n_colours_declined_fit"], st["n_colours_audit_mismatch"]))


@pytest.mark.parametrize("name", SETS)
def test_sim_routes(references, monkeypatch, name):
    ref, sim = references(name, monkeypatch)
    _report("simulator", name, "default", sim)
    assert sim["n_colours_small"] == sim["n_colours_wide"] == sim["n_colours_declined_fit"] == 0 and sim["n_colours_audit_mismatch"] == 0  # the simulator has no register program
    assert sim["n_colours_bits"] >= 100
    audit = _run(ref, SIM_LIB, dict(SETTINGS[1][1]), monkeypatch)
    _report("simulator", name, "audit", audit)
    assert audit["n_colours_audit_mismatch"] == 0 and sum(audit[n] for n in ANSWERED) == sum(sim[n] for n in ANSWERED)
    fault = _run(ref, SIM_LIB, dict(SETTINGS[2][1]), monkeypatch)
    assert fault["n_colours_audit_mismatch"] > 0, "the audit did not notice a first answer without its largest id"


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gpu_routes(references, monkeypatch, name):
    ref, sim = references(name, monkeypatch)
    seen = {}
    for setting, env in SETTINGS:
        seen[setting] = st = _run(ref, None, dict(env), monkeypatch)
        _report("MI355X", name, setting, st)
    d, audit, fault = (seen[s] for s, _ in SETTINGS)
    for st in (d, audit):
        assert st["n_colours_audit_mismatch"] == 0
        # a declined call is answered, and counted, by a later program: none is expected on these sets (every call of theirs with at most 1664 entries fits)
        assert st["n_colours_declined_fit"] == 0
        assert sum(st[n] for n in ANSWERED) + st["n_colours_declined_fit"] == sim["n_colours_bits"] + sim["n_colours_general"]
    assert fault["n_colours_audit_mismatch"] > 0, "the audit did not notice a first answer without its largest id"
    if name == "all-k21":
        assert d["n_colours_small"] >= 100 and d["n_colours_wide"] >= 100, d
    else:
        assert d["n_colours_wide"] >= 1000, d
