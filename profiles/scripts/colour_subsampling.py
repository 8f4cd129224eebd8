"""What `rtk_build_index --subsample-colours` does to sizes, to the laps of the build and to the first correction pass (profiles/colour_subsampling.txt).
One MI355X, the 2 Mb diploid set of profiles/index_build_steps.txt at 30x and 60x short reads, k = 31 and 63.
  python profiles/scripts/colour_subsampling.py --work DIR [--parent-tool PATH/bin/rtk_build_index] [--runs 5] [--host-only] > profiles/colour_subsampling.txt
--host-only: sizes and the host step's lap only (no GPU needed); the device laps and the correction legs are left out and the output says so.
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
LINE = re.compile(r"subsample: hap_cov=(\d+) rate=([0-9.]+) ids=(\d+)->(\d+) events=(\d+)->(\d+) bins=(\d+) sampled_bins=(\d+)")
LAP = re.compile(r"rtk_build_index: \[ *([0-9.]+) s\] (.*)")


def build(tool, sr, out, k, extra):
    t0 = time.time()
    r = subprocess.run([tool, "-s", sr, "-o", out, "-k", str(k), "--snps"] + extra, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", RTK_INDEX_THREADS="16"), timeout=120)
    wall = time.time() - t0
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    laps, prev = {}, 0.0
    for m in LAP.finditer(r.stderr):
        laps[m.group(2)] = float(m.group(1)) - prev
        prev = float(m.group(1))
    return dict(wall=wall, laps=laps, line=LINE.search(r.stderr), err=r.stderr)


def med(v):
    return "median %.3f (%s) spread %.3f" % (statistics.median(v), " ".join("%.3f" % x for x in v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True); ap.add_argument("--parent-tool"); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lr-n", type=int, default=500); ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    tool = os.path.join(BIN, "rtk_build_index")
    print("Colour subsampling (rtk_build_index --subsample-colours): sizes, laps, and the first correction pass on the thinned colours")
    if a.host_only:
        print("HOST ONLY: taken without a GPU on %d hardware threads. The --gpu laps (the step on the device, 'colours and coverage' with and without the option against the parent commit) and the correction legs (correct -1 bases/s, identity to the truth) are NOT in this file: not measured yet." % (os.cpu_count() or 0))
    else:
        print("One MI355X; the host laps (--fast) are taken on the same machine's 16 threads. A lap is the time since the lap before it in the tool's RTK_INDEX_TRACE output, which prints hundredths of a second.")
    print("Input: rtk_simulate --seed 2 --ref-len 2000000 --het 0.001 --sr-cov C (C = 30, 60), %d long reads of 8 kb at 8 %% errors with their truth; RTK_INDEX_THREADS=16; %d runs each, alternating.\n" % (a.lr_n, a.runs))
    for cov in (30, 60):
        pre = os.path.join(a.work, "T%d" % cov)
        subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "2000000", "--het", "0.001", "--sr-cov", str(cov),
                               "--lr-n", str(a.lr_n), "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.08", "--lr-truth"], stderr=subprocess.DEVNULL, timeout=300)
        sr = pre + ".sr.fq"
        for k in (31, 63):
            print("== %dx, k = %d" % (cov, k))
            out = os.path.join(a.work, "o")
            plain = build(tool, sr, out + "_p", k, ["--fast"])
            sub = build(tool, sr, out + "_s", k, ["--fast", "--subsample-colours"])
            size = lambda o: os.path.getsize(o + ".index.k%d.rtsk" % k)
            if sub["line"] is None:
                print("  " + [l for l in sub["err"].splitlines() if "subsample:" in l][0].strip())
                print("  .rtsk bytes %d -> %d (nothing subsampled)" % (size(out + "_p"), size(out + "_s")))
            else:
                g = sub["line"].groups()
                print("  hap_cov %s rate %s ids %s -> %s events %s -> %s bins %s sampled %s; .rtsk bytes %d -> %d" % (g + (size(out + "_p"), size(out + "_s"))))
            host = [build(tool, sr, out + "_h", k, ["--fast", "--subsample-colours"])["laps"].get("colours subsampled", 0.0) for _ in range(a.runs)]
            print("  lap 'colours subsampled', --fast (host step):  " + med(host))
            if a.host_only:
                print()
                continue
            rows = {"parent --gpu": [], "--gpu": [], "--gpu --subsample-colours": []}
            step = []
            for _ in range(a.runs):
                if a.parent_tool:
                    rows["parent --gpu"].append(build(a.parent_tool, sr, out + "_gp", k, ["--gpu"]))
                rows["--gpu"].append(build(tool, sr, out + "_g", k, ["--gpu"]))
                r = build(tool, sr, out + "_gs", k, ["--gpu", "--subsample-colours"])
                rows["--gpu --subsample-colours"].append(r)
                step.append(r["laps"].get("colours subsampled", 0.0))
            same = open(out + "_gs.index.k%d.rtsk" % k, "rb").read() == open(out + "_s.index.k%d.rtsk" % k, "rb").read()
            print("  lap 'colours subsampled', --gpu (structure + plan on the host, events on the device, kept events copied back): " + med(step) + ("" if same else "  FILES DIFFER FROM --fast"))
            for name, rs in rows.items():
                if rs:
                    print("  %-28s lap 'colours and coverage done' %s" % (name, med([r["laps"].get("colours and coverage done", 0.0) for r in rs])))
                    print("  %-28s that lap + 'colours subsampled'   %s" % (name, med([r["laps"].get("colours and coverage done", 0.0) + r["laps"].get("colours subsampled", 0.0) for r in rs])))
                    print("  %-28s wall                              %s" % (name, med([r["wall"] for r in rs])))
            if k == 31:
                correction(a, pre, out, cov)
            print()


def correction(a, pre, out, cov):
    """`Ratatosk correct -1` file to file with the plain and the subsampled index (two seeds), and the corrected reads' identity to their truth"""
    from ratatosk_amd import api
    from oracle import oracle_py as op
    tool, exe, lr = os.path.join(BIN, "rtk_build_index"), os.path.join(BIN, "Ratatosk"), pre + ".lr.fq"
    raw = op.read_fastq(lr)
    n_bases = sum(len(r[1]) for r in raw)
    rcs = lambda x: x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    ref = [l for l in open(pre + ".ref.fa").read().split("\n") if l and l[0] != ">"]
    truth = []
    for l in open(pre + ".lr.truth.tsv").read().splitlines():
        _, hap, start, ln, strand = l.split("\t")
        s = ref[int(hap)][int(start):int(start) + int(ln)]
        truth.append(rcs(s) if strand.strip() == "-" else s)
    tot = sum(len(t) for t in truth)
    d_raw = sum(r[0] for r in api.myers_batch([r[1] for r in raw], truth, [-1] * len(raw), [0] * len(raw)))
    print("  first pass, %d reads / %d bases, raw identity to the truth %.5f" % (len(raw), n_bases, 1.0 - d_raw / tot))
    for name, extra in (("plain index", []), ("subsampled, seed 1", ["--subsample-colours"]), ("subsampled, seed 2", ["--subsample-colours", "--subsample-seed", "2"])):
        build(tool, pre + ".sr.fq", out + "_c", 31, ["--gpu"] + extra)
        walls = []
        for _ in range(3):
            t0 = time.time()
            subprocess.check_call([exe, "correct", "-1", "-c", "16", "-g", out + "_c.index.k31.fasta.gz", "-d", out + "_c.index.k31.rtsk", "-l", lr, "-o", out + "_c"], stderr=subprocess.DEVNULL, timeout=120)
            walls.append(time.time() - t0)
        got = op.read_fastq(out + "_c.2.fastq")
        d = sum(r[0] for r in api.myers_batch([g[1] for g in got], truth, [-1] * len(got), [0] * len(got)))
        print("  %-20s correct -1 file to file: wall s %s = %.3g bases/s at the median (process start and graph load included); identity to the truth %.5f" % (
            name, med(walls), n_bases / statistics.median(walls), 1.0 - d / tot))


if __name__ == "__main__":
    main()
