"""Index build at two-word k-mers (33 <= k <= 63; the second-pass index uses k2 = 63). `rtk_build_index --fast` (host threads) and `--gpu` (counting,
unitigs and colours on the device: csrc/hip/rtk_index.hip with 128-bit keys) must write the plain tool's two files byte for byte, and the device
build must match the independent oracle (oracle/oracle_index.py). Seeded sets with heterozygous SNPs, repeats and tandem repeats; the genomes
whose chains of k-mers meet themselves; reads with N and reads shorter than k; records cut across the device's staging chunks."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import BIN, ROOT
from test_index_build import SETS, _build, _index_vs_oracle, _rc, _self_meeting_genomes, _simulated

TOOL = os.path.join(BIN, "rtk_build_index")


def _files(sr, out, k, extra, env=None):
    r = subprocess.run([TOOL, "-s", sr, "-o", out, "-k", str(k)] + extra, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})))
    assert r.returncode == 0, r.stderr
    assert "takes the plain path" not in r.stderr, r.stderr
    return open(out + ".index.k%d.fasta.gz" % k, "rb").read(), open(out + ".index.k%d.rtsk" % k, "rb").read(), r.stderr


def _same_as_plain(tmp, name, sr, k, mode, extra, env=None):
    a = _files(sr, os.path.join(tmp, "%s_k%d_plain" % (name, k)), k, extra)
    b = _files(sr, os.path.join(tmp, "%s_k%d_%s" % (name, k, mode.strip("-"))), k, [mode] + extra, env)
    assert a[0] == b[0], (name, k, mode, extra, "unitig FASTA differs")
    assert a[1] == b[1], (name, k, mode, extra, ".rtsk differs")
    return b[2]


def _odd_reads(tmp):
    """reads with N inside, reads shorter than k, lower-case bases, on a small random genome"""
    rnd = random.Random(9)
    g = "".join(rnd.choice("ACGT") for _ in range(8000))
    sr = os.path.join(tmp, "odd.sr.fq")
    with open(sr, "w") as f:
        n = 0
        for rep in range(4):
            for start in range(rep, len(g) - 150, 9):
                s = list(g[start:start + 150] if (start // 9) % 2 else _rc(g[start:start + 150]))
                if n % 5 == 0: s[rnd.randrange(150)] = "N"
                if n % 7 == 0: s = s[:rnd.randrange(20, 62)]
                if n % 11 == 0: s = [c.lower() for c in s]
                s = "".join(s)
                f.write("@r%d\n%s\n+\n%s\n" % (n, s, "I" * len(s))); n += 1
    return sr


def test_fast_two_word_index_writes_the_plain_files(tmp_path):
    tmp = str(tmp_path)
    for name, args in SETS[:2] + SETS[3:]:
        sr = _simulated(tmp, name, args)
        for k in (63, 33, 61):
            _same_as_plain(tmp, name, sr, k, "--fast", ["--snps"])
    sr = _simulated(tmp, "p2", SETS[0][1])
    lr = os.path.join(tmp, "p2.lr.fq")
    _same_as_plain(tmp, "p2", sr, 63, "--fast", ["--colour-reads", lr])
    _same_as_plain(tmp, "p2s", sr, 63, "--fast", ["--colour-reads", lr, "--snps"])
    _same_as_plain(tmp, "odd", _odd_reads(tmp), 63, "--fast", ["--snps"])


def test_fast_two_word_index_of_self_meeting_chains(tmp_path):
    tmp = str(tmp_path)
    trace = _same_as_plain(tmp, "self", _self_meeting_genomes(tmp), 63, "--fast", ["--snps"])
    n_plain = [int(l.split(":")[1].split()[0]) for l in trace.splitlines() if "chains that meet themselves" in l]
    assert n_plain and n_plain[0] >= 2, trace


def test_fast_two_word_index_against_the_oracle(tmp_path):
    tmp = str(tmp_path)
    sr = _simulated(tmp, "o", ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "30", "--sr-err", "0.01"])
    assert _index_vs_oracle(sr, os.path.join(tmp, "o_fast"), 63, ["--fast"], colour=os.path.join(tmp, "o.lr.fq")) > 10


def _device_steps_ran(trace):
    assert "rtk_index_count_kmers:" in trace, trace                                                       # counted on the device
    assert "rtk_index_unitigs:" in trace and "unitigs on the host threads" not in trace, trace          # chains walked there
    assert "rtk_index_colour:" in trace and "colours on the host threads" not in trace, trace           # reads mapped there


@pytest.mark.gpu
def test_gpu_two_word_index_writes_the_plain_files(tmp_path):
    tmp = str(tmp_path)
    for name, args in SETS[:2]:
        sr = _simulated(tmp, name, args)
        for k in (63, 33):
            _device_steps_ran(_same_as_plain(tmp, name, sr, k, "--gpu", ["--snps"]))
        lr = os.path.join(tmp, name + ".lr.fq")
        _device_steps_ran(_same_as_plain(tmp, name + "_c", sr, 63, "--gpu", ["--colour-reads", lr, "--snps"]))
    # small staging chunks: records cut across the pieces the device counts
    sr = _simulated(tmp, "chunks", SETS[0][1])
    _device_steps_ran(_same_as_plain(tmp, "chunks", sr, 63, "--gpu", [], env={"RTK_INDEX_CHUNK": "4096"}))
    _device_steps_ran(_same_as_plain(tmp, "odd", _odd_reads(tmp), 63, "--gpu", ["--snps"]))
    _device_steps_ran(_same_as_plain(tmp, "self", _self_meeting_genomes(tmp), 63, "--gpu", []))
    # the host fallbacks keep working at k = 63
    _same_as_plain(tmp, "hostcol", sr, 63, "--gpu", [], env={"RTK_INDEX_HOST_COLOURS": "1", "RTK_INDEX_HOST_UNITIGS": "1"})


@pytest.mark.gpu
def test_gpu_two_word_index_against_the_oracle(tmp_path):
    tmp = str(tmp_path)
    sr = _simulated(tmp, "o", ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "30", "--sr-err", "0.01"])
    for k in (63, 33):
        assert _index_vs_oracle(sr, os.path.join(tmp, "o_gpu%d" % k), k, ["--gpu"]) > 10
    assert _index_vs_oracle(sr, os.path.join(tmp, "o_gpu_c"), 63, ["--gpu"], colour=os.path.join(tmp, "o.lr.fq")) > 10


@pytest.mark.gpu
def test_gpu_count_kmers_two_words_through_the_c_abi(tmp_path):
    """rtk_index_count_kmers at k = 63: two words per k-mer, low word first, sorted, the k-mers seen >= min_count times (a Python count)"""
    tmp = str(tmp_path)
    sr = _odd_reads(tmp)
    k, mc = 63, 2
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    counts = {}
    with open(sr) as f:
        lines = f.read().split("\n")
    for seq in lines[1::4]:
        seq = seq.upper()
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if "N" in w:
                continue
            c = min(w, _rc(w))
            x = 0
            for ch in c:
                x = (x << 2) | code[ch]
            counts[x] = counts.get(x, 0) + 1
    want = sorted(x for x, n in counts.items() if n >= mc)
    lib = ctypes.CDLL(os.path.join(ROOT, "ratatosk_amd", "libratatosk_hip.so"))
    lib.rtk_index_count_kmers.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                          ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64)), ctypes.POINTER(ctypes.c_uint64)]
    lib.rtk_last_error.restype = ctypes.c_char_p
    files = (ctypes.c_char_p * 1)(sr.encode())
    out = ctypes.POINTER(ctypes.c_uint64)(); n = ctypes.c_uint64(0)
    assert lib.rtk_index_count_kmers(0, k, files, 1, mc, 4, ctypes.byref(out), ctypes.byref(n)) == 0, lib.rtk_last_error()
    got = [out[2 * i] | (out[2 * i + 1] << 64) for i in range(n.value)]
    lib.rtk_free(out)
    assert len(want) > 1000 and got == want
