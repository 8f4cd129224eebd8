"""What colouring the second-pass index by base confidence and read length ([A14]: rtk_build_index --colour-min-conf / --colour-min-len, `correct -s ... -M -C`) does
to the two-pass output and to the colouring lap of the k2 index build (profiles/second_pass_colouring.txt). One MI355X, the 2 Mb diploid set of
profiles/colour_subsampling.txt and profiles/merge_duplicates.txt at 30x short reads, 500 long reads of 8 kb with their truth.
  python profiles/scripts/second_pass_colouring.py --work DIR [--parent-tool PATH/bin/rtk_build_index] [--runs 5] > profiles/second_pass_colouring.txt
--parent-tool: the index tool of the commit before (with its own libratatosk_hip.so one directory up), run alternating with this one."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "ratatosk_amd", "bin")
LAP = re.compile(r"rtk_build_index: \[ *([0-9.]+) s\] (.*)")
LEFT = re.compile(r"(\d+) colouring reads shorter than")
EVENTS = re.compile(r"-> (\d+) distinct \(unitig, read\) events")


def run(args, timeout=600, env=None):
    t0 = time.time()
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", RTK_INDEX_THREADS="16", **(env or {})), timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("%s\n%s" % (" ".join(args), r.stderr))
    return r.stderr, time.time() - t0


def build(tool, sr, out, k, extra, env=None):
    err, wall = run([tool, "-s", sr, "-o", out, "-k", str(k), "--snps", "--gpu"] + extra, timeout=120, env=env)
    laps, prev = {}, 0.0
    for m in LAP.finditer(err):
        laps[m.group(2)] = float(m.group(1)) - prev
        prev = float(m.group(1))
    left, ev = LEFT.search(err), EVENTS.search(err)
    return dict(wall=wall, laps=laps, left=int(left.group(1)) if left else 0, events=int(ev.group(1)) if ev else -1)


def med(v):
    return "median %.3f (%s) spread %.3f" % (statistics.median(v), " ".join("%.3f" % x for x in v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True); ap.add_argument("--parent-tool"); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lr-n", type=int, default=500); ap.add_argument("--cov", type=int, default=30)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    from ratatosk_amd import api
    from oracle import oracle_py as op
    tool, exe = os.path.join(BIN, "rtk_build_index"), os.path.join(BIN, "Ratatosk")
    pre, out = os.path.join(a.work, "T"), os.path.join(a.work, "o")
    print("Second-pass index coloured by base confidence and read length (rtk_build_index --colour-reads --colour-min-conf M --colour-min-len N; correct -s ... -M -C)")
    print("One MI355X. Input: rtk_simulate --seed 2 --ref-len 2000000 --het 0.001 --sr-cov %d, %d long reads of 8 kb (ont profile) at 8 %% errors with their truth;" % (a.cov, a.lr_n))
    print("RTK_INDEX_THREADS=16. Both indexes with --gpu --snps, k1 = 31, k2 = 63; the passes with -c 16. A lap is the time since the lap before it in the tool's RTK_INDEX_TRACE output.\n")
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "2000000", "--het", "0.001", "--sr-cov", str(a.cov),
                           "--lr-n", str(a.lr_n), "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.08", "--lr-truth"], stderr=subprocess.DEVNULL, timeout=300)
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    rcs = lambda x: x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    ref = [l for l in open(pre + ".ref.fa").read().split("\n") if l and l[0] != ">"]
    truth = []
    for l in open(pre + ".lr.truth.tsv").read().splitlines():
        _, hap, start, ln, strand = l.split("\t")
        s = ref[int(hap)][int(start):int(start) + int(ln)]
        truth.append(rcs(s) if strand.strip() == "-" else s)
    tot = sum(len(t) for t in truth)

    def identity(path):
        reads = op.read_fastq(path)
        assert len(reads) == len(truth), (path, len(reads))
        return 1.0 - sum(r[0] for r in api.myers_batch([r[1] for r in reads], truth, [-1] * len(reads), [0] * len(reads))) / tot

    print("== accuracy: identity of the reads to their truth (edit distance over the truth's bases)")
    print("  uncorrected reads                         %.5f" % identity(lr))
    build(tool, sr, out + "_1", 31, [])
    run([exe, "correct", "-1", "-c", "16", "-g", out + "_1.index.k31.fasta.gz", "-d", out + "_1.index.k31.rtsk", "-l", lr, "-o", out])
    p1 = out + ".2.fastq"
    first = op.read_fastq(p1)
    n_bases = sum(len(r[1]) for r in first)
    print("  first pass                                %.5f   (%d reads, %d bases; %d bases of quality '!' = %.2f %%; %d reads below 3000 bases)"
          % (identity(p1), len(first), n_bases, sum(r[2].count("!") for r in first), 100.0 * sum(r[2].count("!") for r in first) / n_bases, sum(len(r[1]) < 3000 for r in first)))
    variants = (("no option (the parent's behaviour)", []), ("-M 0 -C 3000 (the reference's default)", ["--colour-min-conf", "0", "--colour-min-len", "3000"]),
                ("-C 3000 alone", ["--colour-min-len", "3000"]), ("-M 0 alone", ["--colour-min-conf", "0"]))
    for i, (name, extra) in enumerate(variants):
        o = out + "_2%d" % i
        b = build(tool, sr, o, 63, ["--colour-reads", p1] + extra)
        run([exe, "correct", "-2", "-c", "16", "-g", o + ".index.k63.fasta.gz", "-d", o + ".index.k63.rtsk", "-l", p1, "-L", lr, "-o", o])
        print("  two passes, k2 index with %-38s %.5f   (events %d, reads left out by length %d, .rtsk bytes %d)" % (name, identity(o + ".fastq"), b["events"], b["left"], os.path.getsize(o + ".index.k63.rtsk")))
        sys.stdout.flush()

    legs = ([("parent, no option", a.parent_tool, [])] if a.parent_tool else []) + [("(a) this commit, no option", tool, []), ("(b) this commit, --colour-min-conf 0 --colour-min-len 3000", tool, ["--colour-min-conf", "0", "--colour-min-len", "3000"])]
    # the second table: the job's event buffer sized by hand (RTK_INDEX_EVENTS), which takes the seconds of opening a job with 60 % of the device memory out of the lap
    for title, env in (("", None), (", RTK_INDEX_EVENTS=16000000 (room for 16 M events instead of 60 % of the device memory)", {"RTK_INDEX_EVENTS": "16000000"})):
        print("\n== speed: rtk_build_index --gpu --snps -k 63 --colour-reads FIRST_PASS.fastq%s, %d runs each, alternating" % (title, a.runs))
        rows = {name: [] for name, _, _ in legs}
        for _ in range(a.runs):
            for j, (name, t, extra) in enumerate(legs):
                rows[name].append(build(t, sr, out + "_s%d" % j, 63, ["--colour-reads", p1] + extra, env=env))
        if a.parent_tool:
            same = all(open(out + "_s0.index.k63" + e, "rb").read() == open(out + "_s1.index.k63" + e, "rb").read() for e in (".rtsk", ".fasta.gz"))
            print("  files without the options against the parent's: %s" % ("the same bytes" if same else "DIFFERENT"))
        for name, _, _ in legs:
            print("  %-60s lap 'colours and coverage done' %s" % (name, med([r["laps"].get("colours and coverage done", 0.0) for r in rows[name]])))
            print("  %-60s wall                            %s" % (name, med([r["wall"] for r in rows[name]])))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
