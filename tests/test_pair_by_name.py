"""`rtk_build_index --pair-by-name` / `Ratatosk correct -s R1 -s R2 --pair-by-name`: the colour id of a short read is the rank of its NAME by first appearance over
all -s files, as the reference's name_hmap hands ids out (addCoverage, src/Graph.cpp:1595-1608, 1800-1804; DESIGN.md section 4 [A18]), so that mates in separate files
share one id. Without the option the id is the number of name changes before the read, which pairs the mates of an interleaved file only.

The rule and the input layouts are restated in tests/pair_ids_restatement.py. The point of the feature is held byte for byte: the split files with the option write the
files of the interleaved file without it. The ids are held to the restatement on a layout where the two differ (a third file, singletons, a name of three records).

CPU tier: the whole tool, plain and --fast, threads, k = 31 and 63, with the later colour steps on top; /1-/2 names, a shuffled R2, gzip inputs; the ids; small byte
ranges; the refusals; the summary line and its warning; the command line of `correct`. GPU tier: the device stage (csrc/hip/rtk_index_pairs.h k_pair_*) through its
entry on crafted hashes, in one pass and in forced and memory-driven passes, its plan and its refusal; `rtk_build_index --gpu --pair-by-name` against --fast and
against the interleaved file; one `Ratatosk correct` on split files against the run on the interleaved file."""
import gzip
import os
import random
import re
import subprocess

import pytest

import pair_ids_restatement as PR
from conftest import BIN, ROOT, SIM_LIB
from ratatosk_amd import api
from test_colour_subsampling import _units

TOOL = os.path.join(BIN, "rtk_build_index")
EXE = os.path.join(BIN, "Ratatosk")
SIM_EXE = os.path.join(ROOT, "tests", "hostsim", "Ratatosk_sim")
RTK_ERR_UNSUPPORTED, RTK_ERR_DEVICE = -6, -5  # include/ratatosk_hip.h
SUMMARY = re.compile(r"rtk_build_index: --pair-by-name: (\d+) records, (\d+) names: (\d+) with one record, (\d+) with two, (\d+) with more")
WARNING = "the mates do not seem to share their names"
LATER = ["--snps", "--merge-duplicates", "--subsample-colours"]
CHILD_TIMEOUT = 300  # seconds: a child that opens the GPU never runs without one


def _build(files, out, k, extra, env=None, ok=True):
    args = [TOOL] + [a for f in files for a in ("-s", f)] + ["-o", out, "-k", str(k)] + extra
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=CHILD_TIMEOUT)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return open(out + ".index.k%d.fasta.gz" % k, "rb").read(), open(out + ".index.k%d.rtsk" % k, "rb").read(), r.stderr


def _side_by_side(*calls):
    """the results of calls (function, args...) that start one child each, run side by side. At most one of them opens the GPU: the index tool sizes its buffers
    by the free device memory, so two of them on one device take each other's."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(calls)) as pool:
        return [f.result() for f in [pool.submit(*c) for c in calls]]


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """the short reads of a set of the size of ds_small, interleaved as rtk_simulate writes them, and the same reads in the layouts of the restatement"""
    tmp = str(tmp_path_factory.mktemp("pair_by_name"))
    pre = os.path.join(tmp, "set")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "40", "--sr-err", "0.01",
                           "--lr-n", "8", "--lr-len", "3000", "--lr-profile", "ont", "--lr-err", "0.08"], stderr=subprocess.DEVNULL)
    inter = pre + ".sr.fq"
    L = dict(tmp=tmp, inter=inter, lr=pre + ".lr.fq", split=PR.split(inter, os.path.join(tmp, "split")), slash=PR.split(inter, os.path.join(tmp, "slash"), slash=True),
             shuffled=PR.split(inter, os.path.join(tmp, "shuffled"), shuffle_r2=5), mixed=PR.split(inter, os.path.join(tmp, "mixed"), slash=True, shuffle_r2=7, keep_interleaved=900, singletons=40, triple=True))
    L["gz"] = []
    for f in L["split"]:
        with open(f, "rb") as src, gzip.open(f + ".gz", "wb") as dst:
            dst.write(src.read())
        L["gz"].append(f + ".gz")
    return L


_BASE = {}


def _base(layouts, k, extra):
    """the files of the interleaved input WITHOUT the option (the bytes of the commit before it): built once, left unchanged"""
    key = (k, tuple(extra))
    if key not in _BASE:
        _BASE[key] = _build([layouts["inter"]], os.path.join(layouts["tmp"], "base_k%d_%d" % (k, len(extra))), k, extra)
    return _BASE[key]


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_name_hash_is_the_stated_rule():
    assert PR.name_hash("") == api.name_hash("") and PR.name_hash("sr17") == api.name_hash("sr17") == api.name_hash(b"sr17")
    assert api.name_hash("a") != api.name_hash("b") and 0 <= api.name_hash("x" * 300) < 1 << 64
    h = 0xcbf29ce484222325  # FNV-1a of "a" by hand, then the mixer
    h = ((h ^ ord("a")) * 0x100000001b3) & PR.M64
    assert h == 0xaf63dc4c8601ec8c  # (the published FNV-1a test vector)
    assert PR.read_name("X/1 comment") == "X" and PR.read_name("X/3") == "X/3" and PR.read_name("/1") == "/1"


@pytest.mark.parametrize("extra", [[], LATER], ids=["alone", "with_later_steps"])
@pytest.mark.parametrize("k", [31, 63])
def test_split_files_write_the_files_of_the_interleaved_file(layouts, tmp_path, k, extra):
    base = _base(layouts, k, extra)
    for mode, threads in (([], "3"), (["--fast"], "1"), (["--fast"], "3"), (["--fast"], "4")):
        got = _build(layouts["split"], os.path.join(str(tmp_path), "o"), k, extra + mode + ["--pair-by-name"], {"RTK_INDEX_THREADS": threads})
        assert got[0] == base[0] and got[1] == base[1], (k, extra, mode, threads)
        m = SUMMARY.search(got[2])
        assert m and int(m.group(1)) == 2 * int(m.group(2)) == 2 * int(m.group(4)) and m.group(3) == m.group(5) == "0" and WARNING not in got[2], got[2]
    # the option on the interleaved file changes nothing
    same = _build([layouts["inter"]], os.path.join(str(tmp_path), "i"), k, extra + ["--pair-by-name"])
    assert same[:2] == base[:2] and not SUMMARY.search(same[2])  # (one file, no trace: no line)


@pytest.mark.parametrize("layout", ["slash", "shuffled", "gz"])
def test_other_names_orders_and_readers(layouts, tmp_path, layout):
    base = _base(layouts, 31, [])
    for mode in ([], ["--fast"]):
        got = _build(layouts[layout], os.path.join(str(tmp_path), "o"), 31, mode + ["--pair-by-name"], {"RTK_INDEX_THREADS": "3"})
        assert got[:2] == base[:2], (layout, mode)


def test_without_the_option_the_mates_do_not_share_an_id(layouts, tmp_path):
    """the gap the option closes: every read an id of its own, twice the ids"""
    base = _base(layouts, 31, [])
    got = _build(layouts["split"], os.path.join(str(tmp_path), "o"), 31, [])
    assert got[0] == base[0] and got[1] != base[1]
    n_base = max(i for _, _, c in _units(os.path.join(layouts["tmp"], "base_k31_0"), 31) for i in c) + 1
    n_split = max(i for _, _, c in _units(os.path.join(str(tmp_path), "o"), 31) for i in c) + 1
    assert n_split > 1.9 * n_base, (n_base, n_split)


def _predicted_colours(units, k, files):
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))  # noqa: E731
    where = {}
    for u, (seq, _, _) in enumerate(units):
        for p in range(len(seq) - k + 1):
            w = seq[p:p + k]
            where[min(w, rc(w))] = u
    recs, n_ids = PR.predicted_ids(files)
    cols = [set() for _ in units]
    for i, seq in recs:
        seq = seq.upper()
        for p in range(len(seq) - k + 1):
            w = seq[p:p + k]
            u = where.get(min(w, rc(w)))
            if u is not None:
                cols[u].add(i)
    return [sorted(c) for c in cols], recs, n_ids


@pytest.mark.parametrize("mode,env", [([], {}), (["--fast"], {"RTK_INDEX_THREADS": "4"}), (["--fast"], {"RTK_INDEX_THREADS": "3", "RTK_INDEX_CHUNK": "1024"})], ids=["plain", "fast", "fast_small_ranges"])
def test_the_ids_are_those_of_the_rule(layouts, tmp_path, mode, env):
    """a third file with interleaved pairs, singletons, /1-/2 names, a shuffled R2 and a name of three records: the ids differ from those of any interleaved file.
    Small ranges (RTK_INDEX_CHUNK): some thousand ranges over the three files, the pairs of the third file straddle their boundaries."""
    out = os.path.join(str(tmp_path), "o")
    got = _build(layouts["mixed"], out, 31, mode + ["--pair-by-name"], env)
    units = _units(out, 31)
    want, recs, n_ids = _predicted_colours(units, 31, layouts["mixed"])
    assert [c for _, _, c in units] == want
    per = {}
    for i, _ in recs:
        per[i] = per.get(i, 0) + 1
    m = SUMMARY.search(got[2])
    assert m and [int(x) for x in m.groups()] == [len(recs), n_ids, sum(v == 1 for v in per.values()), sum(v == 2 for v in per.values()), sum(v > 2 for v in per.values())], got[2]
    assert int(m.group(3)) >= 30 and int(m.group(5)) == 1  # the singletons and the triple are there
    if "RTK_INDEX_CHUNK" in env:
        assert os.path.getsize(layouts["mixed"][2]) > 100 * 1024 and got[1] == _build(layouts["mixed"], out + "b", 31, ["--pair-by-name"])[1]


def test_the_summary_warns_when_no_name_is_shared(layouts, tmp_path):
    r2 = os.path.join(str(tmp_path), "renamed_R2.fq")
    PR.write_fastq(r2, [("mate_" + n, s, q) for n, s, q in PR.read_fastq(layouts["split"][1])])
    for mode in ([], ["--fast"]):
        got = _build([layouts["split"][0], r2], os.path.join(str(tmp_path), "o"), 31, mode + ["--pair-by-name"])
        m = SUMMARY.search(got[2])
        assert m and m.group(1) == m.group(2) == m.group(3) and m.group(4) == "0" and WARNING in got[2], got[2]
    # one file: the line comes with the trace only, and a file of single reads is no case for the warning
    got = _build([layouts["split"][0]], os.path.join(str(tmp_path), "o"), 31, ["--pair-by-name"], {"RTK_INDEX_TRACE": "1"})
    assert SUMMARY.search(got[2]) and WARNING not in got[2] and "read names paired" in got[2] and re.search(r"read names: sweep [0-9.]+ s \(one reader\), ids [0-9.]+ s \(host threads\)", got[2]), got[2]


def test_refusals(layouts, tmp_path):
    out, sr = os.path.join(str(tmp_path), "o"), layouts["split"]
    r = _build(sr, out, 31, ["--pair-by-name", "--colour-reads", layouts["lr"]], ok=False)
    assert r.returncode == 2 and "--pair-by-name next to --colour-reads" in r.stderr and "nothing to pair" in r.stderr, r.stderr
    r = _build(sr, out, 31, ["--pair-by-name", "--graph-only"], ok=False)
    assert r.returncode == 2 and "--graph-only writes the unitig FASTA and stops: --pair-by-name does not go with it" in r.stderr, r.stderr
    r = _build([sr[0], "sample:ref.fa?cov=10&len=150"], out, 31, ["--pair-by-name"], ok=False)
    assert r.returncode == 2 and "--pair-by-name with the source sample:ref.fa" in r.stderr and "numbered by construction" in r.stderr, r.stderr
    assert not os.path.exists(out + ".index.k31.rtsk")
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode == 2 and "--pair-by-name" in r.stderr
    r = subprocess.run([TOOL, "-s", sr[0], "--pair-by-nam", "-o", out], capture_output=True, text=True)
    assert r.returncode == 2 and "unknown option --pair-by-nam" in r.stderr


def _steps(stderr, step):
    return [l for l in stderr.splitlines() if ("%s (" % step) in l and "rtk_build_index --gpu " in l]  # (the command line of the step, as -v shows it)


def test_command_line_of_correct(tmp_path):
    tmp = str(tmp_path)
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    r1, r2, out = os.path.join(tmp, "missing_R1.fq"), os.path.join(tmp, "missing_R2.fq"), os.path.join(tmp, "out")
    for exe in (EXE, SIM_EXE):
        # handed to step 1 (the child command is shown with -v; without a GPU the step then fails and ends the run)
        r = subprocess.run([exe, "correct", "-v", "-s", r1, "-s", r2, "--pair-by-name", "--merge-duplicates", "--subsample-colours", "-l", lr, "-o", out], capture_output=True, text=True)
        step1 = _steps(r.stderr, "step 1")
        assert r.returncode != 0 and len(step1) == 1 and "--pair-by-name" in step1[0] and "-s %s -s %s" % (r1, r2) in step1[0] and "--merge-duplicates" in step1[0], r.stderr
        # not to the step that builds the k2 graph alone
        r = subprocess.run([exe, "correct", "-v", "-s", r1, "-s", r2, "--pair-by-name", "--k1-from-k2", "--cover-edges", "-l", lr, "-o", out], capture_output=True, text=True)
        step1a = _steps(r.stderr, "step 1a")
        assert r.returncode != 0 and len(step1a) == 1 and "--graph-only" in step1a[0] and "--pair-by-name" not in step1a[0], r.stderr
        # -2 alone: accepted, and the second-pass index (coloured by the long reads) does not get it
        r = subprocess.run([exe, "correct", "-v", "-2", "-s", r1, "-s", r2, "--pair-by-name", "-l", lr, "-L", lr, "-o", out], capture_output=True, text=True)
        step3 = _steps(r.stderr, "step 3")
        assert len(step3) == 1 and "--colour-reads" in step3[0] and "--pair-by-name" not in step3[0] and "--pair-by-name" not in r.stderr.replace(step3[0], ""), r.stderr
        r = subprocess.run([exe, "correct", "-v", "-s", r1, "-l", lr, "-o", out], capture_output=True, text=True)
        assert "--pair-by-name" not in r.stderr
        # not next to a pre-built index
        r = subprocess.run([exe, "correct", "-1", "-g", "a", "-d", "b", "-l", lr, "-o", out, "--pair-by-name"], capture_output=True, text=True)
        assert r.returncode == 1 and "--pair-by-name belongs to the index build" in r.stderr and "-g" in r.stderr, r.stderr
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert "--pair-by-name" in r.stderr


def test_interfaces_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "ratatosk_hip.h")).read()
    assert re.search(r"\bint\s+rtk_index_pair_ids\s*\(", hdr) and re.search(r"\bint\s+rtk_index_pair_plan\s*\(", hdr)
    knobs = open(os.path.join(ROOT, "ratatosk_amd", "csrc", "hip", "rtk_knobs.h")).read()
    assert "RTK_INDEX_PAIR_PASSES" in knobs and "RTK_INDEX_PAIR_MEM" in knobs
    for fn, args in ((api.index_pair_ids, ([1, 2, 1],)), (api.index_pair_plan, (1000,))):  # the simulator build has the entries and refuses them
        with pytest.raises(api.RtkError) as e:
            fn(*args, lib_path=SIM_LIB)
        assert "rtk error %d:" % RTK_ERR_UNSUPPORTED in str(e.value) and "not part of the simulator build" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the stage
def _top(byte, low):
    return (byte << 56) | low


def _stage_cases():
    rnd, C = random.Random(20), {}

    def draw(n, names):
        pool = [rnd.getrandbits(64) for _ in range(names)]
        return [pool[rnd.randrange(names)] for _ in range(n)]

    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025):
        C["n%d" % n] = draw(n, max(1, (n + 1) // 2))
    C["all_equal"] = [0x0123456789abcdef] * 300
    C["all_distinct"] = [rnd.getrandbits(64) for _ in range(700)]
    half = [rnd.getrandbits(64) for _ in range(333)]
    C["r1_r2"] = half + half
    shuffled = list(half); rnd.shuffle(shuffled)
    C["r1_r2_shuffled"] = half + shuffled
    C["runs_of_3"] = [h for h in half[:100] for _ in range(3)]
    C["runs_of_100"] = [h for _ in range(100) for h in half[:7]]  # (the members of a run lie 7 apart)
    C["head_at_the_last_ordinal"] = half[:50] + half[:50] + [rnd.getrandbits(64)]
    C["extreme_values"] = [PR.M64, 0, 5, PR.M64, 0, PR.M64 - 1, 1, 0]
    C["one_top_range"] = [_top(0x5a, rnd.getrandbits(20)) for _ in range(900)]  # every pass but one is empty, whatever P
    C["one_hash_per_range"] = [_top(b, rnd.getrandbits(56)) for b in range(256)] + [_top(b, 0) for b in range(0, 256, 5)]
    return C


CASES = _stage_cases()
_WANT = {}


def _want(name):
    if name not in _WANT:
        _WANT[name] = PR.pair_ids(CASES[name])
    return _WANT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [0, 1, 2, 3, 8, 256])
def test_gpu_stage_against_the_restatement(passes, monkeypatch):
    monkeypatch.setenv("RTK_INDEX_PAIR_PASSES", str(passes))  # read at the call (rtk_knobs.h); 0: as few as fit
    monkeypatch.delenv("RTK_INDEX_PAIR_MEM", raising=False)
    for name in sorted(CASES):
        ids, n_ids = api.index_pair_ids(CASES[name])
        assert (ids, n_ids) == _want(name), (name, passes)


@pytest.fixture(scope="module")
def many():
    rnd = random.Random(77)
    names = [rnd.getrandbits(64) for _ in range(1000000)]
    hashes = [names[rnd.randrange(1000000)] for _ in range(2000000)]
    return hashes, PR.pair_ids(hashes)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2, 3, 8, 256])
def test_gpu_stage_across_many_blocks(many, passes, monkeypatch, capfd):
    """2 x 10^6 records of 10^6 names: sorts and scans over many blocks, two staging chunks per pass"""
    hashes, want = many
    monkeypatch.setenv("RTK_INDEX_PAIR_PASSES", str(passes))
    monkeypatch.setenv("RTK_INDEX_TRACE", "1")
    capfd.readouterr()
    got = api.index_pair_ids(hashes)
    assert got[1] == want[1] and got[0] == want[0], passes
    m = re.search(r"rtk_index_pairs: 2000000 records, (\d+) names, (\d+) pass", capfd.readouterr().err)
    assert m and int(m.group(1)) == want[1] and int(m.group(2)) == passes


@pytest.mark.gpu
def test_gpu_plan_passes_and_refusal(many, monkeypatch):
    """The room decides: with less than the single pass needs the stage runs in passes, with less than the smallest plan it refuses with both numbers."""
    hashes, want = many
    n = len(hashes)
    monkeypatch.delenv("RTK_INDEX_PAIR_PASSES", raising=False)
    monkeypatch.delenv("RTK_INDEX_PAIR_MEM", raising=False)
    p, one, mn = api.index_pair_plan(n)
    print("records %d, plan: passes %d, one pass %d bytes, smallest %d bytes" % (n, p, one, mn))
    assert p == 1 and 12 * n < mn < one and one > 28 * n  # (leader, rank and ids are 12 n bytes; leader and the sort's buffers of one pass 28 n)
    assert api.index_pair_plan(n, room=one)[0] == 1 and api.index_pair_plan(n, room=(one + mn) // 2)[0] >= 2 and api.index_pair_plan(n, room=mn - 1)[0] == 0
    assert api.index_pair_plan(0) == (1, 0, 0) and api.index_pair_ids([]) == ([], 0)
    with pytest.raises(api.RtkError) as e:
        api.index_pair_plan(1 << 32)
    assert "rtk error %d:" % RTK_ERR_UNSUPPORTED in str(e.value) and "2^32 records" in str(e.value)
    monkeypatch.setenv("RTK_INDEX_PAIR_MEM", str((one + mn) // 2))
    assert api.index_pair_plan(n)[0] >= 2
    assert api.index_pair_ids(hashes) == want
    monkeypatch.setenv("RTK_INDEX_PAIR_MEM", str(mn - 1))
    with pytest.raises(api.RtkError) as e:
        api.index_pair_ids(hashes)
    m = re.search(r"need (\d+) bytes of device memory, (\d+) are to be had", str(e.value))
    assert "rtk error %d:" % RTK_ERR_DEVICE in str(e.value) and m and int(m.group(1)) == mn and int(m.group(2)) == mn - 1, str(e.value)


# ---------------------------------------------------------------------------------------------------------------- GPU tier: the tool and the one command
@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], LATER], ids=["alone", "with_later_steps"])
@pytest.mark.parametrize("k", [31, 63])
def test_gpu_tool_writes_the_files_of_the_host_route(layouts, tmp_path, k, extra):
    tmp = str(tmp_path)
    trace = {"RTK_INDEX_TRACE": "1"}
    fast, inter = _side_by_side((_build, layouts["split"], os.path.join(tmp, "fast"), k, extra + ["--fast", "--pair-by-name"]),
                                (_build, [layouts["inter"]], os.path.join(tmp, "inter"), k, extra + ["--gpu"], trace))
    dev = _build(layouts["split"], os.path.join(tmp, "dev"), k, extra + ["--gpu", "--pair-by-name"], trace)
    assert dev[:2] == fast[:2] == inter[:2], (k, extra)
    assert "rtk_index_pairs:" in dev[2] and "paired on the host threads" not in dev[2] and re.search(r"ids [0-9.]+ s \(device\)", dev[2]) and "rtk_index_colour:" in dev[2], dev[2]
    assert "rtk_index_pairs:" not in inter[2]


@pytest.mark.gpu
def test_gpu_tool_in_passes_and_back_on_the_host(layouts, tmp_path):
    tmp = str(tmp_path)
    fast, dev = _side_by_side((_build, layouts["mixed"], os.path.join(tmp, "fast"), 31, ["--fast", "--pair-by-name"]),
                              (_build, layouts["mixed"], os.path.join(tmp, "dev"), 31, ["--gpu", "--pair-by-name"], {"RTK_INDEX_TRACE": "1", "RTK_INDEX_PAIR_PASSES": "5"}))
    low = _build(layouts["mixed"], os.path.join(tmp, "low"), 31, ["--gpu", "--pair-by-name"], {"RTK_INDEX_PAIR_MEM": "1000"})
    assert dev[:2] == fast[:2] and "5 passes over the hash space" in dev[2], dev[2]
    m = re.search(r"--gpu: read names paired on the host threads \(.*need (\d+) bytes of device memory, (\d+) are to be had", low[2])
    assert low[:2] == fast[:2] and m and int(m.group(1)) > 1000 and m.group(2) == "1000", low[2]


@pytest.mark.gpu
def test_gpu_one_command_on_split_files(layouts, tmp_path):
    """`Ratatosk correct -s R1 -s R2 --pair-by-name` corrects as the run on the interleaved file does; step 1 gets the option, step 3 does not"""
    a, b = os.path.join(str(tmp_path), "A"), os.path.join(str(tmp_path), "B")
    run = lambda args: subprocess.run([EXE, "correct", "-c", "2"] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT)  # noqa: E731
    r = run(["-v", "-s", layouts["split"][0], "-s", layouts["split"][1], "--pair-by-name", "-l", layouts["lr"], "-o", a])
    rb = run(["-s", layouts["inter"], "-l", layouts["lr"], "-o", b])
    assert r.returncode == 0 and rb.returncode == 0, r.stderr + rb.stderr
    step1, step3 = _steps(r.stderr, "step 1"), _steps(r.stderr, "step 3")
    assert len(step1) == 1 and "--pair-by-name" in step1[0] and len(step3) == 1 and "--pair-by-name" not in step3[0], r.stderr
    assert SUMMARY.search(r.stderr) and WARNING not in r.stderr, r.stderr
    got, want = open(a + ".fastq").read(), open(b + ".fastq").read()
    assert got == want and len(got) > 8 * 3000
    assert got != open(layouts["lr"]).read()  # something was corrected
