"""What `rtk_build_index --merge-duplicates` does to sizes, to the laps of the build, to what the region stage reads and to the first correction pass
(profiles/merge_duplicates.txt). One MI355X, the 2 Mb diploid set of profiles/colour_subsampling.txt at 30x and 60x short reads, k = 31 and 63.
  python profiles/scripts/merge_duplicates.py --work DIR [--cov 30 --cov 60] [--parent-tool PATH/bin/rtk_build_index] [--runs 5] [--host-only] >> profiles/merge_duplicates.txt
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
MERGE = re.compile(r"merge: ids=(\d+)->(\d+) events=(\d+)->(\d+) classes_above_one=(\d+) largest=(\d+)")
SUB = re.compile(r"subsample: hap_cov=(\d+) rate=([0-9.]+) ids=(\d+)->(\d+) events=(\d+)->(\d+)")
LAP = re.compile(r"rtk_build_index: \[ *([0-9.]+) s\] (.*)")
DEV = re.compile(r"ids merged on the device: .*\(([0-9.]+) s\)")


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
    dev = DEV.search(r.stderr)
    return dict(wall=wall, laps=laps, merge=MERGE.search(r.stderr), sub=SUB.search(r.stderr), err=r.stderr, dev=float(dev.group(1)) if dev else 0.0)


def med(v):
    return "median %.3f (%s) spread %.3f" % (statistics.median(v), " ".join("%.3f" % x for x in v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True); ap.add_argument("--parent-tool"); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lr-n", type=int, default=500); ap.add_argument("--host-only", action="store_true"); ap.add_argument("--cov", type=int, action="append")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    tool = os.path.join(BIN, "rtk_build_index")
    print("Merged ids (rtk_build_index --merge-duplicates): sizes, laps, what the region stage reads, and the first correction pass on the merged ids")
    if a.host_only:
        print("HOST ONLY: taken without a GPU on %d hardware threads. The --gpu laps and the correction legs are NOT in this part: not measured." % (os.cpu_count() or 0))
    else:
        print("One MI355X; the host laps (--fast) are taken on the same machine's 16 threads. A lap is the time since the lap before it in the tool's RTK_INDEX_TRACE output, which prints hundredths of a second.")
    print("Input: rtk_simulate --seed 2 --ref-len 2000000 --het 0.001 --sr-cov C, %d long reads of 8 kb at 8 %% errors with their truth; RTK_INDEX_THREADS=16; %d runs each, alternating.\n" % (a.lr_n, a.runs))
    for cov in (a.cov or [30, 60]):
        pre = os.path.join(a.work, "T%d" % cov)
        subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", "2000000", "--het", "0.001", "--sr-cov", str(cov),
                               "--lr-n", str(a.lr_n), "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.08", "--lr-truth"], stderr=subprocess.DEVNULL, timeout=300)
        sr = pre + ".sr.fq"
        for k in (31, 63):
            print("== %dx, k = %d" % (cov, k))
            out = os.path.join(a.work, "o")
            size = lambda o: os.path.getsize(o + ".index.k%d.rtsk" % k)
            build(tool, sr, out + "_p", k, ["--fast"])
            mrg = build(tool, sr, out + "_m", k, ["--fast", "--merge-duplicates"])
            sub = build(tool, sr, out + "_s", k, ["--fast", "--subsample-colours"])
            both = build(tool, sr, out + "_b", k, ["--fast", "--merge-duplicates", "--subsample-colours"])
            g = mrg["merge"].groups()
            print("  without the option      ids %s events %s .rtsk bytes %d" % (g[0], g[2], size(out + "_p")))
            print("  --merge-duplicates      ids %s events %s .rtsk bytes %d (classes above one id %s, largest %s)" % (g[1], g[3], size(out + "_m"), g[4], g[5]))
            for name, r, o in (("--subsample-colours", sub, "_s"), ("both options", both, "_b")):
                print("  %-23s %s .rtsk bytes %d" % (name, "ids %s events %s (hap_cov %s)" % (r["sub"].group(4), r["sub"].group(6), r["sub"].group(1)) if r["sub"] else "nothing subsampled (hap_cov below 10)", size(out + o)))
            host = [build(tool, sr, out + "_h", k, ["--fast", "--merge-duplicates"])["laps"].get("duplicates merged", 0.0) for _ in range(a.runs)]
            print("  lap 'duplicates merged', --fast (host step):  " + med(host))
            if a.host_only:
                print()
                continue
            rows = {"parent --gpu": [], "--gpu": [], "--gpu --merge-duplicates": []}
            for _ in range(a.runs):
                if a.parent_tool:
                    rows["parent --gpu"].append(build(a.parent_tool, sr, out + "_gp", k, ["--gpu"]))
                rows["--gpu"].append(build(tool, sr, out + "_g", k, ["--gpu"]))
                rows["--gpu --merge-duplicates"].append(build(tool, sr, out + "_gm", k, ["--gpu", "--merge-duplicates"]))
            same = open(out + "_gm.index.k%d.rtsk" % k, "rb").read() == open(out + "_m.index.k%d.rtsk" % k, "rb").read()
            unchanged = not a.parent_tool or open(out + "_gp.index.k%d.rtsk" % k, "rb").read() == open(out + "_g.index.k%d.rtsk" % k, "rb").read()
            ms = rows["--gpu --merge-duplicates"]
            print("  lap 'duplicates merged', --gpu (events merged in HBM, then copied back): " + med([r["laps"].get("duplicates merged", 0.0) for r in ms]) + ("" if same else "  FILES DIFFER FROM --fast"))
            print("  of it inside rtk_index_colour_merge: " + med([r["dev"] for r in ms]))
            print("  files without the option against the parent's: %s" % ("the same bytes" if unchanged else "DIFFERENT"))
            for name, rs in rows.items():
                if rs:
                    print("  %-26s lap 'colours and coverage done' %s" % (name, med([r["laps"].get("colours and coverage done", 0.0) for r in rs])))
                    print("  %-26s that lap + 'duplicates merged'  %s" % (name, med([r["laps"].get("colours and coverage done", 0.0) + r["laps"].get("duplicates merged", 0.0) for r in rs])))
                    print("  %-26s wall                            %s" % (name, med([r["wall"] for r in rs])))
            if k == 31:
                correction(a, pre, out, cov)
            print()
            sys.stdout.flush()


def correction(a, pre, out, cov):
    """The first pass through the library on the index without and with the option, in alternating visits: what the region stage reads and how long it takes,
    and the corrected reads' identity to their truth"""
    from ratatosk_amd import api
    from oracle import oracle_py as op
    tool, lr = os.path.join(BIN, "rtk_build_index"), pre + ".lr.fq"
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
    print("  first pass on the 2 Mb set (not the 60 Mb set of bench.py), %d reads / %d bases, raw identity to the truth %.5f" % (len(raw), n_bases, 1.0 - d_raw / tot))
    legs = (("plain index", []), ("merged ids", ["--merge-duplicates"]))
    graphs, got, visits = {}, {}, {name: [] for name, _ in legs}
    for name, extra in legs:
        build(tool, pre + ".sr.fq", out + "_c" + str(len(extra)), 31, ["--gpu"] + extra)
        graphs[name] = api.Graph(out + "_c%d.index.k31.fasta.gz" % len(extra), out + "_c%d.index.k31.rtsk" % len(extra), 31, device=0)
    seqs, quals = [r[1] for r in raw], [r[2] for r in raw]
    for visit in range(6):  # (the first visit of each index warms up and is not counted)
        for name, _ in legs:
            b = api.Batch(graphs[name], seqs, quals)
            b.run()
            st = b.stats()
            if visit:
                visits[name].append(st)
            else:
                got[name] = b.fetch()
            b.close()
    for name, _ in legs:
        st = visits[name][0]
        d = sum(r[0] for r in api.myers_batch([g[0] for g in got[name]], truth, [-1] * len(raw), [0] * len(raw)))
        print("  %-12s graph colour ids %d; per batch: colour ids read by k_regions (n_colour_elem) %d, chooseColors calls small / wide / bits / general %d / %d / %d / %d, cyc_colour %d of cyc_total %d"
              % (name, graphs[name].info().n_colour_ids, st["n_colour_elem"], st["n_colours_small"], st["n_colours_wide"], st["n_colours_bits"], st["n_colours_general"], st["cyc_colour"], st["cyc_total"]))
        print("  %-12s k_regions ms (5 alternating visits): %s; ms_total %s" % (name, med([s["ms_regions"] for s in visits[name]]), med([s["ms_total"] for s in visits[name]])))
        print("  %-12s identity to the truth %.5f" % (name, 1.0 - d / tot))


if __name__ == "__main__":
    main()
