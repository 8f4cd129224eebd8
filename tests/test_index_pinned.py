"""The bytes rtk_build_index writes, pinned: SHA-256 of the .rtsk file and of the inflated unitig FASTA on one small simulated set (heterozygous
sites, repeats, tandem repeats; 30 kb), at k = 21, 31 and 63 with --snps and at k = 63 coloured by the long reads (--colour-reads). The hashes were
taken from the tool as it stood before its host code was cut into named steps (tools/index/), not from the code under test: whoever restructures the
tool next has the bytes to hold on to. Every route writes them: plain, --fast, 1 and 7 threads, and --gpu in the gpu tier. The simulator's files are
pinned as well, so that a change to rtk_simulate shows up as a changed input and not as a changed index."""
import gzip
import hashlib
import os
import subprocess

import pytest

from conftest import BIN

SIM_ARGS = ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--tandem", "5", "--sr-cov", "40", "--sr-err", "0.01",
            "--lr-n", "12", "--lr-len", "3000", "--lr-profile", "ont", "--lr-err", "0.08"]
INPUTS = {".sr.fq": "d5e84ee4ba572acfa3d8269e453426eff3f9b55e60892b6b2fcdab44320993ad",
          ".lr.fq": "f805f1a1c1d7153c5b139d5d7bb695728bf1197fa7996f5ef9dd6fd13058507c"}
PINNED = {  # case -> (k, --snps, --colour-reads, SHA-256 of the .rtsk, SHA-256 of the inflated FASTA)
    "k21": (21, True, False, "729f0b8e0a02e0018740fb18a308044d9dddf586803516729f2ba7faf7b6a604", "ccdbbd6e41a16034b8aa65dfcf90c2eddc7efa7c1e3cdea683bd52b4ca90767a"),
    "k31": (31, True, False, "e5a3411c2f65b0ccf4f4167227f3200c8b3cb3dfbe4598572eeea9f1bca58f6b", "0e4f751e76a8bd51ed776c3eafa8fda95b68cee711b5d55dc168fb76d5d9272e"),
    "k63": (63, True, False, "5de767bbaa28524f6f4cbb9da97c7c1a8d9f888d0e6a5b4f8f10791241bb59b0", "095cec2fb82e3167b216e5afd7b5ba49838352e33eedd9237e2368e33cc2b3b4"),
    "k63_coloured_by_long_reads": (63, False, True, "62b2f0ef8fe74aac64032890715d426b7d4490dbec1c2de9d4edd414d543cdb3", "095cec2fb82e3167b216e5afd7b5ba49838352e33eedd9237e2368e33cc2b3b4"),
}
GPU_STEP_TIMEOUT = 300  # seconds, every child process that opens the GPU


def _sha(data):
    return hashlib.sha256(data).hexdigest()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    pre = os.path.join(str(tmp_path_factory.mktemp("pinned")), "s")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + SIM_ARGS, stderr=subprocess.DEVNULL)
    return pre


def _check(reads, tmp, case, extra, env=None, timeout=None):
    k, snps, coloured, want_rtsk, want_fasta = PINNED[case]
    out = os.path.join(str(tmp), case)
    args = ["-s", reads + ".sr.fq", "-o", out, "-k", str(k)] + (["--snps"] if snps else []) + (["--colour-reads", reads + ".lr.fq"] if coloured else []) + extra
    r = subprocess.run([os.path.join(BIN, "rtk_build_index")] + args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})), timeout=timeout)
    assert r.returncode == 0, r.stderr
    assert _sha(open(out + ".index.k%d.rtsk" % k, "rb").read()) == want_rtsk, (case, extra, env, ".rtsk")
    assert _sha(gzip.open(out + ".index.k%d.fasta.gz" % k, "rb").read()) == want_fasta, (case, extra, env, "unitig FASTA")
    return r.stderr


def test_simulated_reads_are_pinned(reads):
    for ext, want in INPUTS.items():
        assert _sha(open(reads + ext, "rb").read()) == want, ext


@pytest.mark.parametrize("mode", ["plain", "--fast"])
@pytest.mark.parametrize("case", sorted(PINNED))
def test_plain_and_fast_write_the_pinned_bytes(reads, tmp_path, case, mode):
    _check(reads, tmp_path, case, [] if mode == "plain" else [mode])


@pytest.mark.parametrize("threads", ["1", "7"])
@pytest.mark.parametrize("case", sorted(PINNED))
def test_any_number_of_threads_writes_the_pinned_bytes(reads, tmp_path, case, threads):
    for extra in ([], ["--fast"]):
        _check(reads, tmp_path, case, extra, env={"RTK_INDEX_THREADS": threads})


@pytest.mark.gpu
def test_gpu_writes_the_pinned_bytes(reads, tmp_path):
    """counting, unitigs and colours on the device (the trace says so)"""
    for case in sorted(PINNED):
        trace = _check(reads, tmp_path, case, ["--gpu"], timeout=GPU_STEP_TIMEOUT)
        assert "rtk_index_unitigs:" in trace and "unitigs on the host threads" not in trace, trace
        assert "rtk_index_colour:" in trace and "colours on the host threads" not in trace, trace
