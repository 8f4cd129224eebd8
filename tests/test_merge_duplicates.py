"""`rtk_build_index --merge-duplicates`: short-read pairs that lie on the same unitigs share one colour id, as the block of the reference's index step that it
announces as "Detecting and removing duplicated reads" gives pairs of equal signature the same read id (src/Graph.cpp:1630-1705, 2089-2134; DESIGN.md section 4 [A13]).

The rule is restated here in Python (`_merge`) from its statement in DESIGN.md, not from the tool's code: U(i) the unitigs of id i, g(u) the splitmix64 finalizer of
u + 1, S(i) the sum of g over U(i) modulo 2^64, low(i) = min U(i); ids with equal (S, low) are one class, the leader is the smallest id, the leaders in ascending
order are numbered from 0, every id takes its leader's number. On every input the restatement also groups the ids by their exact unitig set and asserts that the two
groupings agree: an input on which the 64-bit sum collided would otherwise hide a wrong class. No test passes on a run that merged nothing (`_assert_merged`).

CPU tier: the whole tool, plain and --fast, k = 31 and 63; with --subsample-colours on top; --colour-reads (off); crafted events through rtk_merge_step; the command
line. GPU tier: the device route (csrc/hip/rtk_index.hip k_merge_*) through its stage entry on crafted events, `rtk_build_index --gpu --merge-duplicates` against
`--fast`, the job entry after several sort-and-unique rounds, and one `Ratatosk correct -s ... --merge-duplicates` against the oracle's two passes."""
import gzip
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import BIN, ROOT
from test_colour_subsampling import SETS, _check_against_the_rule, _rule, _units
from test_colour_subsampling import _line as _subsample_line

TOOL = os.path.join(BIN, "rtk_build_index")
STEP = os.path.join(BIN, "rtk_merge_step")
EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
M64 = (1 << 64) - 1
LINE = re.compile(r"rtk_build_index: merge: ids=(\d+)->(\d+) events=(\d+)->(\d+) classes_above_one=(\d+) largest=(\d+)")
OFF = "rtk_build_index: merge: off (--colour-reads)"
RTK_ERR_NO_DEVICE = -4  # include/ratatosk_hip.h


# ---------------------------------------------------------------------------------------------------------------- the rule, restated
def _g(u):
    z = (u + 1) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _key(unitigs):
    return (sum(_g(u) for u in unitigs) & M64, min(unitigs))


def _merge(cols):
    """colours per unitig (sorted ids) -> the rule's colours per unitig and counts"""
    sets = {}
    for u, ids in enumerate(cols):
        for i in ids:
            sets.setdefault(i, []).append(u)
    by_key, by_set = {}, {}
    for i in sorted(sets):
        by_key.setdefault(_key(sets[i]), []).append(i)
        by_set.setdefault(tuple(sets[i]), []).append(i)
    assert sorted(by_key.values()) == sorted(by_set.values()), "the 64-bit sums of two different unitig sets collide on this input"
    classes = list(by_key.values())
    number = {leader: r for r, leader in enumerate(sorted(c[0] for c in classes))}
    new = {i: number[c[0]] for c in classes for i in c}
    out = [sorted({new[i] for i in ids}) for ids in cols]
    return dict(cols=out, ids=(len(sets), len(classes)), events=(sum(len(c) for c in cols), sum(len(c) for c in out)), above=sum(len(c) > 1 for c in classes),
                largest=max((len(c) for c in classes), default=0), alone=sum(len(c) == 1 for c in classes), keys=by_key)


def _counts(want):
    return dict(ids=want["ids"], events=want["events"], above=want["above"], largest=want["largest"])


def _assert_merged(c, alone):
    """the run did merge, and not everything: a test must not pass on a run that merged nothing"""
    assert c["ids"][1] < c["ids"][0] and c["above"] >= 1 and alone >= 1, (c, alone)


def _line(stderr):
    m = LINE.search(stderr)
    assert m, stderr
    v = [int(x) for x in m.groups()]
    return dict(ids=(v[0], v[1]), events=(v[2], v[3]), above=v[4], largest=v[5])


def _events(cols):
    return np.array([(u << 32) | i for u, ids in enumerate(cols) for i in ids], dtype=np.uint64)


def _cols_of(ids_to_unitigs, n_unitigs):
    cols = [[] for _ in range(n_unitigs)]
    for i in sorted(ids_to_unitigs):
        for u in sorted(set(ids_to_unitigs[i])):
            cols[u].append(i)
    return cols


# ---------------------------------------------------------------------------------------------------------------- helpers
def _simulate(tmp, name, args, lr=("--lr-n", "2", "--lr-len", "1000")):
    pre = os.path.join(tmp, name)
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + args + list(lr), stderr=subprocess.DEVNULL)
    return pre


def _build(sr, out, k, extra, env=None):
    r = subprocess.run([TOOL, "-s", sr, "-o", out, "-k", str(k), "--snps"] + extra, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})))
    assert r.returncode == 0, r.stderr
    return open(out + ".index.k%d.fasta.gz" % k, "rb").read(), open(out + ".index.k%d.rtsk" % k, "rb").read(), r.stderr


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("merge_sets"))
    return {name: _simulate(tmp, name, args) + ".sr.fq" for name, args in SETS.items()}


_BASE = {}


def _base(reads, tmp_path_factory, name, k):
    """the files of a run without the option and the rule on them: built and worked out once, left unchanged"""
    if (name, k) not in _BASE:
        out = os.path.join(str(tmp_path_factory.mktemp("merge_base")), "base")
        files = _build(reads[name], out, k, [])
        units = _units(out, k)
        _BASE[(name, k)] = (out, files, units, _merge([c for _, _, c in units]))
    return _BASE[(name, k)]


# ---------------------------------------------------------------------------------------------------------------- CPU tier
# .rtsk files of a run WITHOUT the option, as the commit before the option wrote them (sha256; the FASTA is left out: its bytes are zlib's)
PARENT_RTSK = {
    ("het_repeats", 31): "40bcc320af8a9cbfcc1d0dcfc2ac2e63b0f0a32c16fa4346f81c27e4aa8fdc65",
    ("het_repeats", 63): "232545d89e7d1e63aab272ebc25e3570107b6d45a52a8ca5cf9a925d902f2ba6",
    ("tandem", 31): "131f509108e077c38b8f319f0d4cf435c3bf6d2d4ee27e8f6b3a7625208bba15",
    ("tandem", 63): "13ab02b45821e29e62842fd1d288a2dd29533eed36613f0b110b1eee9891ee6a",
}


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("name", sorted(SETS))
def test_whole_tool_against_the_restated_rule(reads, tmp_path, tmp_path_factory, name, k):
    tmp, sr = str(tmp_path), reads[name]
    base, a, plain, want = _base(reads, tmp_path_factory, name, k)
    assert "merge:" not in a[2]  # no option: no step, and the bytes of the commit before the option
    assert hashlib.sha256(a[1]).hexdigest() == PARENT_RTSK[(name, k)]
    b = _build(sr, os.path.join(tmp, "plain"), k, ["--merge-duplicates"])
    c = _build(sr, os.path.join(tmp, "fast"), k, ["--fast", "--merge-duplicates"])
    d = _build(sr, os.path.join(tmp, "fast3"), k, ["--fast", "--merge-duplicates"], env={"RTK_INDEX_THREADS": "3"})
    line = _line(b[2])
    _assert_merged(line, want["alone"])
    assert b[0] == a[0] and b[1] != a[1]
    assert b[0] == c[0] and b[1] == c[1], "plain and --fast differ"
    assert d[1] == b[1] and d[0] == b[0], "three threads differ"
    assert _line(c[2]) == line and _line(d[2]) == line
    assert line == _counts(want), (line, _counts(want))
    got = _units(os.path.join(tmp, "plain"), k)
    assert [(s, cv) for s, cv, _ in got] == [(s, cv) for s, cv, _ in plain]  # unitigs and coverage as they were
    bad = [u for u in range(len(got)) if got[u][2] != want["cols"][u]]
    assert not bad, ("colour sets differ from the restated rule", len(bad), bad[:5])


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("name", sorted(SETS))
def test_both_options(reads, tmp_path, tmp_path_factory, name, k):
    """subsampling sees the merged ids: the [A12] rule applied to the files of a merge-only run gives the files of a run with both options"""
    tmp, sr = str(tmp_path), reads[name]
    want = _base(reads, tmp_path_factory, name, k)[3]
    m = _build(sr, os.path.join(tmp, "M"), k, ["--merge-duplicates"])
    b = _build(sr, os.path.join(tmp, "B"), k, ["--merge-duplicates", "--subsample-colours"])
    f = _build(sr, os.path.join(tmp, "Bf"), k, ["--fast", "--subsample-colours", "--merge-duplicates"])
    assert b[0] == f[0] and b[1] == f[1] and b[0] == m[0] and b[1] != m[1]
    ml, sl = _line(b[2]), _subsample_line(b[2])
    assert ml == _line(m[2]) == _line(f[2]) == _counts(want) and sl == _subsample_line(f[2])
    _assert_merged(ml, want["alone"])
    assert sl["ids"][0] == ml["ids"][1] and sl["events"][0] == ml["events"][1] and sl["ids"][1] < sl["ids"][0]
    assert b[2].index("merge:") < b[2].index("subsample:")
    _check_against_the_rule(os.path.join(tmp, "M"), os.path.join(tmp, "B"), k, sl)


def test_colour_reads_switch_it_off(reads, tmp_path):
    tmp, sr = str(tmp_path), reads["het_repeats"]
    lr = sr[:-len(".sr.fq")] + ".lr.fq"
    for mode in ([], ["--fast"]):
        a = _build(sr, os.path.join(tmp, "a"), 31, mode + ["--colour-reads", lr])
        b = _build(sr, os.path.join(tmp, "b"), 31, mode + ["--colour-reads", lr, "--merge-duplicates"])
        assert OFF in b[2] and not LINE.search(b[2]) and "merge:" not in a[2]
        assert a[0] == b[0] and a[1] == b[1]
    # ... while the same reads as pairs do merge
    _assert_merged(_line(_build(sr, os.path.join(tmp, "c"), 31, ["--merge-duplicates"])[2]), 1)


def _crafted():
    """name -> colours per unitig, for the host rule and for the device route alike"""
    rnd = random.Random(5)
    cases = {}
    cases["no_events"] = [[]]
    cases["one_event"] = [[], [7]]
    cases["one_class"] = _cols_of({i: [1, 4, 6] for i in (2, 3, 50, 51, 900)}, 8)
    cases["nothing_merges"] = _cols_of({0: [0], 1: [1], 2: [0, 1], 3: [2], 4: [0, 2], 5: [1, 2], 6: [0, 1, 2]}, 3)
    cases["ids_without_events"] = _cols_of({3: [0, 2], 4: [1], 10: [0, 2], 11: [1, 2], 1000: [1]}, 3)  # ids 0, 1, 2 and others colour nothing
    cases["largest_ids"] = _cols_of({0: [0, 1], (1 << 32) - 2: [1, 2], (1 << 32) - 1: [1, 2], 5: [2]}, 3)
    cases["equal_low_different_sum"] = _cols_of({1: [0, 1], 2: [0, 2], 3: [0, 1], 4: [0, 2], 5: [0]}, 3)
    cases["equal_count_different_sets"] = _cols_of({1: [3, 4], 2: [3, 5], 3: [4, 5], 4: [3, 5], 5: [3, 4], 6: [4, 5], 7: [6, 7]}, 8)
    # the class met first in unitig order, {9, 12} on unitig 0, has the larger leader: numbering is by leader, so it is numbered after {2, 4} of unitig 1
    cases["leader_not_first_in_unitig_order"] = _cols_of({9: [0], 12: [0], 2: [1], 4: [1], 7: [0, 1]}, 2)
    pool = [sorted(rnd.sample(range(500), rnd.randint(1, 13))) for _ in range(150)]  # 1 000 ids on 1-13 of 500 unitigs, with many repeats
    ids = rnd.sample(range(1 << 20), 1000)
    cases["random_1000"] = _cols_of({i: (rnd.choice(pool) if rnd.randrange(10) else sorted(rnd.sample(range(500), rnd.randint(1, 13)))) for i in ids}, 500)
    return cases


CRAFTED = _crafted()


def _step(cols, tmp, threads):
    src, dst = os.path.join(tmp, "ev.bin"), os.path.join(tmp, "out.%d.bin" % threads)
    _events(cols).tofile(src)
    r = subprocess.run([STEP, str(threads), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, dtype=np.uint64), _line(r.stderr)


def test_rule_on_crafted_events(tmp_path):
    tmp = str(tmp_path)
    total = dict(before=0, after=0, above=0, alone=0)
    for name, cols in sorted(CRAFTED.items()):
        want = _merge(cols)
        got, line = _step(cols, tmp, 1)
        got4, line4 = _step(cols, tmp, 4)
        assert (got == got4).all() and line == line4, name  # one thread and four: the same
        assert line == _counts(want), (name, line, _counts(want))
        assert got.tolist() == _events(want["cols"]).tolist(), name
        total["before"] += want["ids"][0]; total["after"] += want["ids"][1]; total["above"] += want["above"]; total["alone"] += want["alone"]
    _assert_merged(dict(ids=(total["before"], total["after"]), above=total["above"]), total["alone"])
    w = {name: _merge(cols) for name, cols in CRAFTED.items()}
    assert w["no_events"]["ids"] == (0, 0) and w["one_event"]["cols"] == [[], [0]]
    assert w["one_class"]["ids"] == (5, 1) and w["one_class"]["largest"] == 5
    assert w["nothing_merges"]["ids"] == (7, 7) and w["nothing_merges"]["above"] == 0
    assert w["ids_without_events"]["cols"] == [[0], [1, 2], [0, 2]]  # 3 and 10 -> 0, 4 and 1000 -> 1, 11 -> 2
    assert w["largest_ids"]["cols"] == [[0], [0, 2], [1, 2]] and w["largest_ids"]["ids"] == (4, 3)
    assert w["equal_low_different_sum"]["ids"] == (5, 3) and w["equal_count_different_sets"]["ids"] == (7, 4)
    assert w["leader_not_first_in_unitig_order"]["cols"] == [[1, 2], [0, 1]]  # 2 and 4 -> 0, 7 -> 1, 9 and 12 -> 2
    assert w["random_1000"]["above"] > 50 and w["random_1000"]["alone"] > 50
    # what is not ascending and distinct is refused
    for words in ([5, 5], [(1 << 32) | 1, 3]):
        np.array(words, dtype=np.uint64).tofile(os.path.join(tmp, "bad.bin"))
        r = subprocess.run([STEP, "1", os.path.join(tmp, "bad.bin"), os.path.join(tmp, "bad.out")], capture_output=True, text=True)
        assert r.returncode == 2 and "ascending and distinct" in r.stderr
    assert subprocess.run([STEP], capture_output=True, text=True).returncode == 2


def test_command_line(tmp_path):
    tmp = str(tmp_path)
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    sr = os.path.join(tmp, "missing.fq")
    for exe in (EXE, SIM_EXE):
        # handed to the index step (the child command is shown with -v; without a GPU the step then fails and ends the run)
        r = subprocess.run([exe, "correct", "-v", "-s", sr, "--merge-duplicates", "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
        step1 = [l for l in r.stderr.splitlines() if "step 1" in l and "rtk_build_index" in l and " -s " in l]
        assert r.returncode != 0 and step1 and "--merge-duplicates" in step1[0], r.stderr
        r = subprocess.run([exe, "correct", "-v", "-s", sr, "--merge-duplicates", "--subsample-colours", "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
        step1 = [l for l in r.stderr.splitlines() if "step 1" in l and "rtk_build_index" in l and " -s " in l]
        assert step1 and "--merge-duplicates --subsample-colours" in step1[0], r.stderr
        r = subprocess.run([exe, "correct", "-v", "-s", sr, "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
        assert "--merge-duplicates" not in r.stderr
        # not next to a pre-built index
        r = subprocess.run([exe, "correct", "-1", "-g", "a", "-d", "b", "-l", lr, "-o", os.path.join(tmp, "out"), "--merge-duplicates"], capture_output=True, text=True)
        assert r.returncode == 1 and "--merge-duplicates belongs to the index build" in r.stderr and "-g" in r.stderr, r.stderr
        # the seed of the other option still needs its own option
        r = subprocess.run([exe, "correct", "-s", sr, "--merge-duplicates", "--subsample-seed", "3", "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
        assert r.returncode != 0 and "--subsample-seed without --subsample-colours" in r.stderr, r.stderr
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert "--merge-duplicates" in r.stderr
    r = subprocess.run([TOOL, "-s", sr, "--merge-duplicates", "--subsample-seed", "3", "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
    assert r.returncode == 2 and "--subsample-seed without --subsample-colours" in r.stderr
    r = subprocess.run([TOOL, "-s", sr, "--merge-duplicate", "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
    assert r.returncode == 2 and "unknown option --merge-duplicate" in r.stderr
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode == 2 and "--merge-duplicates" in r.stderr


def test_stage_entry_needs_a_device():
    """the stage entry exists in the library and, like every compute entry, does not fall back to the host"""
    from ratatosk_amd import api
    try:
        out, before, after = api.index_merge_events([5, 6, (1 << 32) | 5, (1 << 32) | 6, (1 << 32) | 9], 2)
    except api.RtkError as e:
        assert "rtk error %d:" % RTK_ERR_NO_DEVICE in str(e) and "no such HIP device" in str(e)
    else:  # (a machine with a GPU)
        assert out.tolist() == [0, (1 << 32) | 0, (1 << 32) | 1] and (before, after) == (3, 2)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _sorted_keys(cols):
    """the entries (S, low, id) in the order the device sorts them in, and per id the place of its first event in the id-major order of the events"""
    sets = {}
    for u, ids in enumerate(cols):
        for i in ids:
            sets.setdefault(i, []).append(u)
    first, at = {}, 0
    for i in sorted(sets):
        first[i] = at
        at += len(sets[i])
    return sorted(_key(us) + (i,) for i, us in sets.items()), first


def _run_case(n_units, start, filler_from=1000):
    """an id on n_units unitigs whose first event is event number `start` of the id-major order, a second id on the same unitigs, single-unitig ids around them"""
    ids = {i: [2000 + i] for i in range(start)}  # `start` ids of one event each, all below the long one
    ids[filler_from] = list(range(n_units)); ids[filler_from + 1] = list(range(n_units))
    ids[filler_from + 2] = [3000]; ids[filler_from + 3] = [0]
    cols = _cols_of(ids, 3001)
    assert _sorted_keys(cols)[1][filler_from] == start
    return cols


def _class_case(size, lane, seed):
    """a class of `size` ids whose first entry is entry number = lane (mod 64) of the sorted runs, behind at least one whole wave of other classes"""
    rnd = random.Random(seed)
    members = rnd.sample(range(100000), size)
    ids = {i: [7, 11, 400] for i in members}
    nxt = 200000
    for _ in range(100):  # single-unitig ids and pairs of them, each on unitigs of their own
        ids[nxt] = [500 + nxt % 5000]; nxt += 1
    for _ in range(2000):
        keys, _ = _sorted_keys(_cols_of(ids, 6000))
        at = keys.index(_key([7, 11, 400]) + (min(members),))
        if at >= 64 and at % 64 == lane:
            break
        ids[nxt] = [500 + nxt % 5000]; nxt += 1
    else:
        raise AssertionError("no such arrangement")
    return _cols_of(ids, 6000)


def _check_stage(api, cols, total, name):
    want = _merge(cols)
    got, before, after = api.index_merge_events(_events(cols), len(cols))
    assert (before, after) == want["ids"], name
    assert got.dtype == np.uint64 and got.tolist() == _events(want["cols"]).tolist(), name
    total["before"] += want["ids"][0]; total["after"] += want["ids"][1]; total["above"] += want["above"]; total["alone"] += want["alone"]
    return want


def _total():
    return dict(before=0, after=0, above=0, alone=0)


def _assert_total_merged(total):
    _assert_merged(dict(ids=(total["before"], total["after"]), above=total["above"]), total["alone"])


@pytest.mark.gpu
def test_gpu_stage_entry_event_counts_and_long_runs():
    from ratatosk_amd import api
    total = _total()
    for n in (0, 1, 63, 64, 65):  # events in all: pairs of ids on the same unitig, the last id alone when n is odd
        cols = [[2 * u, 2 * u + 1] for u in range(n // 2)] + ([[5000]] if n % 2 else []) or [[]]
        assert sum(len(c) for c in cols) == n
        _check_stage(api, cols, total, "n_events_%d" % n)
    for n_units in (65, 130):  # a run over one and over two wave boundaries, starting at lane 0, at lane 63 and mid-wave
        for start in (0, 63, 30, 64 + 63):
            w = _check_stage(api, _run_case(n_units, start), total, "run_%d_at_%d" % (n_units, start))
            assert w["largest"] == 2 and w["above"] == 1
    _assert_total_merged(total)


@pytest.mark.gpu
def test_gpu_stage_entry_classes_over_wave_boundaries():
    from ratatosk_amd import api
    total = _total()
    for size in (65, 200):  # leaders over wave boundaries: the waves after the first find the start of the class by bisection
        for lane in (0, 63):
            w = _check_stage(api, _class_case(size, lane, 10 * size + lane), total, "class_%d_at_lane_%d" % (size, lane))
            assert w["largest"] == size
    w = _check_stage(api, [[u] for u in range(64)], total, "64_classes_in_one_wave")  # 64 classes of one id each
    assert w["ids"] == (64, 64)
    _assert_total_merged(total)


@pytest.mark.gpu
def test_gpu_stage_entry_large_ids_and_random_sets():
    """ids 2^32 - 2 and 2^32 - 1 next to id 0: the tables are sized by the ids that have events -- tables indexed by the id would take 60 GB here"""
    from ratatosk_amd import api
    total = _total()
    for name in sorted(CRAFTED):
        _check_stage(api, CRAFTED[name], total, name)
    _assert_total_merged(total)


@pytest.mark.gpu
def test_gpu_stage_entry_refuses_what_breaks_its_bounds():
    import ctypes as C
    from ratatosk_amd import api
    for ev, n_u in (([(1 << 32) | 4, 3], 2), ([5, 5], 1), ([(2 << 32) | 1], 2)):  # descending, repeated, a unitig >= n_unitigs
        with pytest.raises(api.RtkError):
            api.index_merge_events(ev, n_u)
    L = api.load_library()
    ev = np.array([1, 2], dtype=np.uint64)
    n = C.c_uint64()
    u64 = C.POINTER(C.c_uint64)
    assert L.rtk_index_merge_events(0, ev.ctypes.data_as(u64), 2, 1, None, C.byref(n), C.byref(n), C.byref(n)) != 0  # no room for the output
    assert L.rtk_index_merge_events(0, ev.ctypes.data_as(u64), 2, 1, ev.ctypes.data_as(u64), None, C.byref(n), C.byref(n)) != 0
    got, before, after = api.index_merge_events([1, 2], 1)  # ... and the same events with room: one class
    assert got.tolist() == [0] and (before, after) == (2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_tool_writes_the_files_of_the_host_route(reads, tmp_path, tmp_path_factory, name, k):
    tmp, sr = str(tmp_path), reads[name]
    want = _base(reads, tmp_path_factory, name, k)[3]
    a = _build(sr, os.path.join(tmp, "fast"), k, ["--fast", "--merge-duplicates"])
    b = _build(sr, os.path.join(tmp, "gpu"), k, ["--gpu", "--merge-duplicates"])
    _assert_merged(_line(a[2]), want["alone"])
    assert "ids merged on the device" in b[2] and "ids merged on the host threads" not in b[2] and "colours on the host threads" not in b[2], b[2]  # the device merged the events
    assert _line(a[2]) == _line(b[2]) == _counts(want)
    assert a[0] == b[0] and a[1] == b[1]
    c = _build(sr, os.path.join(tmp, "fast_both"), k, ["--fast", "--merge-duplicates", "--subsample-colours"])
    d = _build(sr, os.path.join(tmp, "gpu_both"), k, ["--gpu", "--merge-duplicates", "--subsample-colours"])
    assert "ids merged on the device" in d[2] and "left after subsampling" in d[2] and "ids merged on the host threads" not in d[2] and "colours on the host threads" not in d[2], d[2]
    assert _line(c[2]) == _line(d[2]) == _line(a[2]) and _subsample_line(c[2]) == _subsample_line(d[2])
    assert c[0] == d[0] and c[1] == d[1] and c[1] != a[1]
    if (name, k) == ("het_repeats", 31):  # the host step on events of the host threads
        e = _build(sr, os.path.join(tmp, "gpu_host"), k, ["--gpu", "--merge-duplicates"], env={"RTK_INDEX_HOST_COLOURS": "1"})
        assert "ids merged on the device" not in e[2] and a[1] == e[1]


@pytest.mark.gpu
def test_gpu_job_entry_after_several_sort_and_unique_rounds(reads, tmp_path, monkeypatch, capfd):
    """rtk_index_colour_merge through the C ABI, the reads fed in eight chunks into an event buffer of twice the distinct events, so that the buffer is sorted and
    thinned out several times before the merge. The job goes on afterwards: its coverage is that of a plain job, its events those of a plain job merged by the
    stage entry, which are the restated rule's."""
    import ctypes as C
    from ratatosk_amd import api
    from oracle import oracle_py as op
    tmp, sr, k = str(tmp_path), reads["het_repeats"], 31
    base = os.path.join(tmp, "base")
    _build(sr, base, k, ["--fast"])
    seqs = [l for l in gzip.open(base + ".index.k31.fasta.gz", "rt").read().split("\n") if l and l[0] != ">"]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(s) for s in seqs])
    pool = "".join(seqs).encode()
    rd = [r[1] for r in op.read_fastq(sr)]
    L = api.load_library()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.rtk_index_colour_begin.argtypes = [C.c_int, C.c_int, C.c_char_p, u64p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.rtk_index_colour_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, u64p, u32p, C.c_uint32]
    L.rtk_index_colour_end.argtypes = [C.c_void_p, C.POINTER(u64p), u64p, C.POINTER(u64p)]

    def ok(rc):
        assert rc == 0, L.rtk_last_error().decode()

    def feed(n_chunks):
        job = C.c_void_p()
        ok(L.rtk_index_colour_begin(0, k, pool, off.ctypes.data_as(u64p), len(seqs), C.byref(job)))
        per = (len(rd) + n_chunks - 1) // n_chunks
        for c in range(0, len(rd), per):
            part = rd[c:c + per]
            chars = ("\n".join(part) + "\n").encode()
            starts = np.zeros(len(part), dtype=np.uint64); starts[1:] = np.cumsum([len(s) + 1 for s in part[:-1]])
            ids = np.array([(c + i) // 2 for i in range(len(part))], dtype=np.uint32)  # a pair keeps one id
            ok(L.rtk_index_colour_chunk(job, chars, len(chars), starts.ctypes.data_as(u64p), ids.ctypes.data_as(u32p), len(part)))
        return job

    def take(p, n):
        a = np.ctypeslib.as_array(p, shape=(max(1, n),))[:n].copy()
        L.rtk_free(p)
        return a

    monkeypatch.setenv("RTK_INDEX_TRACE", "1")
    job = feed(1)
    ev_p, cov_p, n_ev = u64p(), u64p(), C.c_uint64()
    ok(L.rtk_index_colour_end(job, C.byref(ev_p), C.byref(n_ev), C.byref(cov_p)))
    events, cov = take(ev_p, n_ev.value), take(cov_p, len(seqs))
    assert n_ev.value > 10000
    cols = [[] for _ in seqs]
    for e in events.tolist():
        cols[e >> 32].append(e & 0xFFFFFFFF)
    rule = _merge(cols)
    _assert_merged(_counts(rule), rule["alone"])
    want, w_before, w_after = api.index_merge_events(events, len(seqs))
    assert want.tolist() == _events(rule["cols"]).tolist() and (w_before, w_after) == rule["ids"]
    capfd.readouterr()
    monkeypatch.setenv("RTK_INDEX_EVENTS", str(2 * n_ev.value))
    job = feed(8)
    e0, e1, i0, i1, above, largest = (C.c_uint64() for _ in range(6))
    ok(L.rtk_index_colour_merge(job, C.byref(e0), C.byref(e1), C.byref(i0), C.byref(i1)))
    ok(L.rtk_index_colour_merge_classes(job, C.byref(above), C.byref(largest)))
    assert (e0.value, e1.value, i0.value, i1.value, above.value, largest.value) == (len(events), len(want), w_before, w_after, rule["above"], rule["largest"])
    ok(L.rtk_index_colour_cov(job, C.byref(cov_p)))
    assert (take(cov_p, len(seqs)) == cov).all()
    ok(L.rtk_index_colour_end(job, C.byref(ev_p), C.byref(n_ev), C.byref(cov_p)))
    got = take(ev_p, n_ev.value)
    assert (take(cov_p, len(seqs)) == cov).all()
    assert got.shape == want.shape and (got == want).all()
    rounds = re.search(r"thinned out (\d+) times", capfd.readouterr().err)
    assert rounds and int(rounds.group(1)) >= 2, "one round only"


@pytest.mark.gpu
def test_gpu_one_command_with_merged_ids(tmp_path):
    """`Ratatosk correct -s ... --merge-duplicates` on the device against the oracle's two passes on the index files of the merged HOST build: the correction path
    on merged ids. Both index steps receive the option, the first merges, the second colours by long reads and says `off`; the run ends with OUT.fastq alone."""
    from oracle import oracle_py as op
    tmp = str(tmp_path)
    pre = _simulate(tmp, "both", ["--seed", "17", "--ref-len", "30000", "--het", "0.003", "--repeat-frac", "0.05", "--sr-cov", "60", "--sr-err", "0.002"], lr=("--lr-n", "40", "--lr-len", "3000", "--lr-err", "0.08"))
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    raw = op.read_fastq(lr)
    # the oracle's passes on the host build's files
    _build(sr, os.path.join(tmp, "h0"), 31, ["--fast"])
    rule = _merge([c for _, _, c in _units(os.path.join(tmp, "h0"), 31)])
    a = _build(sr, os.path.join(tmp, "h1"), 31, ["--fast", "--merge-duplicates"])
    host_line = _line(a[2])
    assert host_line == _counts(rule)
    _assert_merged(host_line, rule["alone"])
    g1 = op.Graph(os.path.join(tmp, "h1.index.k31.fasta.gz"), os.path.join(tmp, "h1.index.k31.rtsk"), 31)
    p1, _ = g1.correct_batch([r[1] for r in raw], [r[2] for r in raw], threads=8)
    mid = os.path.join(tmp, "h.2.fastq")
    with open(mid, "w") as f:
        for r, (s, q) in zip(raw, p1):
            f.write("@%s\n%s\n+\n%s\n" % (r[0], s, q))
    h2 = _build(sr, os.path.join(tmp, "h2"), 63, ["--fast", "--merge-duplicates", "--colour-reads", mid])
    assert OFF in h2[2]
    g2 = op.Graph(os.path.join(tmp, "h2.index.k63.fasta.gz"), os.path.join(tmp, "h2.index.k63.rtsk"), 63)
    want = g2.correct_batch2([s for s, _ in p1], [q for _, q in p1], [r[1] for r in raw], g2.opts(long_read_correct=1), threads=8)
    # one command on the device
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = subprocess.run([EXE, "correct", "-v", "-c", "2", "-s", sr, "--merge-duplicates", "-l", lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    steps = [l for l in r.stderr.splitlines() if "rtk_build_index)" in l and ("step 1" in l or "step 3" in l)]
    assert len(steps) == 2 and all("--merge-duplicates" in l and "--gpu" in l for l in steps), r.stderr
    assert _line(r.stderr) == host_line and len(LINE.findall(r.stderr)) == 1  # the first index step merged ...
    assert r.stderr.count(OFF) == 1 and r.stderr.index(OFF) > r.stderr.index("merge: ids=")  # ... the second said `off`
    got = op.read_fastq(out + ".fastq")
    assert [g[0] for g in got] == [x[0] for x in raw]
    assert [(g[1], g[2]) for g in got] == want
    assert sum(1 for (s, _), x in zip(want, raw) if s != x[1]) > 0
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)
