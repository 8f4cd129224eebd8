"""The two host steps of the device side's k-mer count (csrc/hip/rtk_index_count.h), alone, through rtk_chunks_step (csrc/tools/chunks_step.cpp):
`chunks` -- the threaded readers that hand the sequences of the read files out in chunks (common/sequence_chunks.hpp: a plain file by byte ranges, gzip through one
reader, a `sample:` source by pair ranges) give the multiset of sequences that FastxReader gives over the same files (the tool's --reader);
`merge` -- the threaded merge of the sorted partitions (common/sorted_runs.hpp) gives the sorted union of its runs. CPU tier only."""
import gzip
import os
import random
import subprocess

import pytest

from conftest import BIN

STEP = os.path.join(BIN, "rtk_chunks_step")


def _chunks(files, threads, chunk_bytes, reader=False):
    r = subprocess.run([STEP, "chunks"] + files + ["--threads", str(threads), "--chunk-bytes", str(chunk_bytes)] + (["--reader"] if reader else []), capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n")[:-1] if r.stdout else [], r.stderr


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """200 reads of 30 to 249 bases in a plain FASTQ file, the same text as one gzip member and as five; the sequences in file order"""
    tmp = str(tmp_path_factory.mktemp("chunks"))
    rnd = random.Random(3)
    seqs = ["".join(rnd.choice("ACGTN" if i % 17 == 0 else "ACGT") for _ in range(rnd.randrange(30, 250))) for i in range(200)]
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)).encode()
    plain, one, several = (os.path.join(tmp, n) for n in ("r.fq", "r1.fq.gz", "r5.fq.gz"))
    open(plain, "wb").write(text)
    open(one, "wb").write(gzip.compress(text))
    cuts = [0, 1001, 9000, 9001, 30011, len(text)]  # (members end inside records)
    open(several, "wb").write(b"".join(gzip.compress(text[a:b]) for a, b in zip(cuts, cuts[1:])))
    return {"tmp": tmp, "seqs": seqs, "plain": plain, "one": one, "several": several}


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_chunks_of_a_plain_file(reads, threads):
    rc, want, err = _chunks([reads["plain"]], 1, 1024, reader=True)
    assert rc == 0 and want == reads["seqs"], err
    rc, got, err = _chunks([reads["plain"]], threads, 1024)
    assert rc == 0 and sorted(got) == sorted(want), err


@pytest.mark.parametrize("which", ["one", "several"])
def test_chunks_of_a_gzip_file(reads, which):
    rc, want, err = _chunks([reads[which]], 1, 1024, reader=True)
    assert rc == 0 and want == reads["seqs"], err
    for threads in (1, 3):
        rc, got, err = _chunks([reads[which]], threads, 1024)
        assert rc == 0 and got == want, err  # (one reader thread: file order)


def test_chunks_of_an_empty_file_and_of_several_files(reads):
    empty = os.path.join(reads["tmp"], "empty.fq")
    open(empty, "wb").close()
    rc, got, err = _chunks([empty], 3, 1024)
    assert rc == 0 and got == [], err
    files = [reads["plain"], empty, reads["several"]]
    rc, want, err = _chunks(files, 1, 1024, reader=True)
    assert rc == 0 and want == 2 * reads["seqs"], err
    rc, got, err = _chunks(files, 3, 1024)
    assert rc == 0 and sorted(got) == sorted(want), err
    assert sorted(got[:200]) == sorted(reads["seqs"]) and got[200:] == reads["seqs"]  # the files in their order


def test_chunks_of_a_sampled_source(reads):
    pre = os.path.join(reads["tmp"], "smp")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "4", "--ref-len", "3030", "--het", "0.002", "--sr-cov", "0", "--lr-n", "2", "--lr-len", "1000"], stderr=subprocess.DEVNULL)
    spec = "sample:%s.ref.fa?cov=5&len=100&insert=300&err=0.01&seed=9" % pre
    rc, want, err = _chunks([spec], 1, 1024, reader=True)
    assert rc == 0 and len(want) % 2 == 0 and (len(want) // 2) % 2 == 1 and all(len(s) == 100 for s in want), err  # an odd number of pairs
    for threads, chunk_bytes in ((1, 50), (3, 50), (16, 50), (3, 1000)):  # 50: below one pair (202 characters), so a pair per chunk; 1000: four pairs, the last chunk short
        rc, got, err = _chunks([spec], threads, chunk_bytes)
        assert rc == 0 and sorted(got) == sorted(want), (threads, chunk_bytes, err)
        pairs = lambda seq: sorted(zip(seq[0::2], seq[1::2]))
        assert pairs(got) == pairs(want), (threads, chunk_bytes)  # the mates stay side by side


def test_chunks_of_a_cut_short_gzip_file(reads):
    cut = os.path.join(reads["tmp"], "cut.fq.gz")
    whole = open(reads["one"], "rb").read()
    open(cut, "wb").write(whole[:len(whole) // 2])
    rc, got, err = _chunks([cut], 3, 1024)
    assert rc == 1 and err.strip() == "rtk_chunks_step: %s ends in a damaged or cut-short gzip stream" % cut, (rc, err)


def _merge(k, threads, runs):
    text = "".join("run\n" + "".join("%x\n" % v for v in run) for run in runs)
    r = subprocess.run([STEP, "merge", "--k", str(k), "--threads", str(threads)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [int(x, 16) for x in r.stdout.split()]


def _runs(rnd, k, n_keys, shape):
    """n_keys distinct keys below 4^k, 0 and 4^k - 1 among them, dealt to the non-empty runs of `shape` (a list of booleans: run r takes keys or stays empty)"""
    top = 4 ** k - 1
    keys = {0, top}
    while len(keys) < n_keys:
        keys.add(rnd.randrange(top + 1) if rnd.random() < 0.7 else rnd.choice([rnd.randrange(64), top - rnd.randrange(64)]))  # (crowded at both ends of the key space)
    runs = [[] for _ in shape]
    open_runs = [r for r, takes in enumerate(shape) if takes]
    for v in keys:
        runs[rnd.choice(open_runs)].append(v)
    return [sorted(run) for run in runs], sorted(keys)


@pytest.mark.parametrize("k", [5, 31, 33, 63])
def test_merge_of_sorted_runs(k):
    rnd = random.Random(k)
    shapes = [[True], [True, True], [True] * 7,
              [False, True, False, False, True, True, False],  # empty runs at both ends and in the middle
              [False], [False, False, False]]
    for shape in shapes:
        for n_keys, threads in ((300, 1), (300, 3), (300, 16), (3, 16), (2, 300)):  # (3, 16), (2, 300): more threads than keys
            if not any(shape):
                runs, want = [[] for _ in shape], []
            else:
                runs, want = _runs(rnd, k, n_keys, shape)
            assert _merge(k, threads, runs) == want, (k, shape, n_keys, threads)
    assert _merge(k, 4, []) == []  # no run at all


def test_merge_refuses_what_is_no_run():
    for text in ("5\n", "run\n5\n5\n", "run\n7\n3\n", "run\n400\n", "run\nxyz\n"):  # a key outside a run, twice, descending, of more than 2 * 5 bits, no number
        r = subprocess.run([STEP, "merge", "--k", "5", "--threads", "2"], input=text, capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("rtk_chunks_step: "), (text, r.stderr)
