"""`Ratatosk correct -s SHORT -l LONG -o OUT` (the reference's one-command run, src/Ratatosk.cpp:1040-1277) and its two-step form `correct -1 -s` /
`correct -2 -s`: the driver builds each pass's index with `rtk_build_index --gpu` and runs the passes, every step a child process. Without a GPU:
argument handling (a failing step is named and ends the run; calls with -g / -d keep their messages). On the GPU: the output is the bytes of the
four commands run by hand, temporary files are removed."""
import gzip
import os
import subprocess

import pytest

from conftest import BIN

EXE = os.path.join(BIN, "Ratatosk")
TOOL = os.path.join(BIN, "rtk_build_index")
SIM_ARGS = ["--seed", "17", "--ref-len", "60000", "--het", "0.003", "--repeat-frac", "0.05", "--sr-cov", "30", "--sr-err", "0.005",
            "--lr-n", "40", "--lr-len", "3000", "--lr-err", "0.08"]


def _sim(tmp, name="s"):
    pre = os.path.join(tmp, name)
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + SIM_ARGS, stderr=subprocess.DEVNULL)
    return pre


def test_one_command_stops_at_the_failing_index_step(tmp_path):
    tmp = str(tmp_path)
    out = os.path.join(tmp, "out")
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    for mode in ([], ["-1"], ["-2", "-L", lr]):
        r = subprocess.run([EXE, "correct"] + mode + ["-s", os.path.join(tmp, "missing.fq"), "-l", lr, "-o", out], capture_output=True, text=True)
        assert r.returncode != 0, (mode, r.stderr)
        assert "index" in r.stderr and "failed" in r.stderr and "step" in r.stderr, (mode, r.stderr)
        assert "-1 or -2" not in r.stderr
        assert not [f for f in os.listdir(tmp) if f.startswith("out")], os.listdir(tmp)
    r = subprocess.run([EXE, "correct", "-2", "-s", lr, "-l", lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "-L" in r.stderr
    r = subprocess.run([EXE, "correct", "-s", lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 1 and "-l" in r.stderr


def test_calls_with_a_prebuilt_index_keep_their_messages():
    r = subprocess.run([EXE, "correct", "-g", "a", "-d", "b", "-l", "c", "-o", "d"], capture_output=True, text=True)
    assert r.returncode == 1 and "-1 or -2" in r.stderr
    r = subprocess.run([EXE, "correct", "-s", "x", "-g", "a", "-d", "b", "-l", "c", "-o", "d"], capture_output=True, text=True)
    assert r.returncode == 1 and "-1 or -2" in r.stderr and "ignored" in r.stderr
    r = subprocess.run([EXE, "index", "-s", "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "not in scope" in r.stderr


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r


@pytest.mark.gpu
def test_gpu_one_command_equals_the_four_steps(tmp_path):
    tmp = str(tmp_path)
    pre = _sim(tmp)
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    # the four commands by hand
    hand = os.path.join(tmp, "hand")
    _run([TOOL, "--gpu", "-k", "31", "-s", sr, "--snps", "-o", hand + "_i1"])
    _run([EXE, "correct", "-1", "-c", "2", "-g", hand + "_i1.index.k31.fasta.gz", "-d", hand + "_i1.index.k31.rtsk", "-l", lr, "-o", hand])
    _run([TOOL, "--gpu", "-k", "63", "-s", sr, "--colour-reads", hand + ".2.fastq", "--snps", "-o", hand + "_i2"])
    _run([EXE, "correct", "-2", "-c", "2", "-g", hand + "_i2.index.k63.fasta.gz", "-d", hand + "_i2.index.k63.rtsk", "-l", hand + ".2.fastq", "-L", lr, "-o", hand])
    want = open(hand + ".fastq", "rb").read()
    assert want.count(b"\n") >= 4 * 40
    # one command
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = _run([EXE, "correct", "-v", "-c", "2", "-s", sr, "-l", lr, "-o", out])
    assert "Building graph" in r.stderr and "(2/2)" in r.stderr
    assert open(out + ".fastq", "rb").read() == want
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)  # temporary indexes and OUT.2.fastq removed
    # -G: the same reads, gzipped
    subg = os.path.join(tmp, "gz"); os.mkdir(subg)
    _run([EXE, "correct", "-G", "-c", "2", "-s", sr, "-l", lr, "-o", os.path.join(subg, "out")])
    assert gzip.open(os.path.join(subg, "out.fastq.gz")).read() == want
    assert sorted(os.listdir(subg)) == ["out.fastq.gz"], os.listdir(subg)
    # two steps: -1 -s then -2 -s
    subt = os.path.join(tmp, "two"); os.mkdir(subt)
    out = os.path.join(subt, "out")
    _run([EXE, "correct", "-1", "-c", "2", "-s", sr, "-l", lr, "-o", out])
    assert open(out + ".2.fastq", "rb").read() == open(hand + ".2.fastq", "rb").read()
    _run([EXE, "correct", "-2", "-c", "2", "-s", sr, "-l", out + ".2.fastq", "-L", lr, "-o", out])
    assert open(out + ".fastq", "rb").read() == want
    assert sorted(os.listdir(subt)) == ["out.2.fastq", "out.fastq"], os.listdir(subt)
