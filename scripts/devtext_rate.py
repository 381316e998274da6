#!/usr/bin/env python3
"""What keeping GPU-inflated text on the device is worth (--gpu-text).

The input is scripts/inflate_rate.py's: the BGZF of a synthetic PE pair
(--text-mib MiB of FASTQ text over both mates, 65,280-byte members) at deflate
levels 1 and 6.  Per level, after one warm-up, the median and the spread of
  kernels alone (mate 1, page-locked input)
    members      sa_inflate_members: H2D, kernel, D2H of the text, wall time
    members_dev  sa_inflate_members_dev into a devtext: H2D, kernel, newline
                 count, wall time -- what dropping the D2H saves
    count        k_dt_count over the inflated text (HIP events): GB/s, and that
                 as a fraction of --hbm-peak
    cut          k_dt_cut over both mates at --block-mib (HIP events):
                 microseconds per PE block
  full -c (not ingest-only), three ways alternating in one call
    host         the host inflate (the baseline: code this path does not touch)
    gpu_inflate  --gpu-inflate
    gpu_text     --gpu-text, under -v: its per-input lines say where the time goes
One JSON document on stdout and in --out.  Rates are MB/s of inflated text.
"""
import argparse
import json
import multiprocessing as mp
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from inflate_rate import bgzf, rate, stats   # noqa: E402


def note(msg):
    print(f"[devtext_rate] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--text-mib", type=int, default=3800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--block-mib", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16, help="-t of the command line and the compressing processes")
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="the device's HBM peak, GB/s (MI355X: 8 TB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "devtext_rate.json"))
    a = ap.parse_args()

    import synth
    import fastqueeze_amd as fq
    from fastqueeze_amd import build

    n_pairs = max(1000, a.text_mib * (1 << 20) // 640)   # ~320 bytes a record
    t0 = time.time()
    t1, t2 = synth.generate(n_pairs, paired=True, seed=4242, workers=min(a.threads, 16))
    res = {"text_bytes": [len(t1), len(t2)], "pairs": n_pairs, "generate_s": round(time.time() - t0, 2),
           "hbm_peak_GBps": a.hbm_peak, "block_mib": a.block_mib, "levels": {}}
    note(f"{n_pairs} pairs, {len(t1) + len(t2)} bytes of text in {res['generate_s']} s")
    first = t1[:t1.index(b"\n") + 1]
    infl = fq.Inflater(0)
    tmp = tempfile.mkdtemp(prefix="devtext_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        with mp.Pool(min(a.threads, 16)) as pool:
            for level in [int(x) for x in a.levels.split(",")]:
                t0 = time.time()
                z1, z2 = bgzf(t1, level, pool), bgzf(t2, level, pool)
                r = {"bgzf_bytes": [len(z1), len(z2)], "compress_s": round(time.time() - t0, 2)}
                ms1, consumed, total = fq.bgzf_scan(z1)
                ms2, _, total2 = fq.bgzf_scan(z2)
                assert consumed == len(z1) and total == len(t1) and total2 == len(t2)
                r["members"] = int(ms1.size)
                note(f"level {level}: {len(z1) + len(z2)} bytes of BGZF in {r['compress_s']} s")
                # ---- kernels alone ----
                hin, hout = fq.HostBuffer(len(z1)), fq.HostBuffer(total)
                hin.array[:] = np.frombuffer(z1, np.uint8)
                wall, kern = [], []
                for k in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    rc, _ = infl.inflate_into(hin.array, ms1, hout.array)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert rc == 0
                    if k:   # (the first run is the warm-up: slabs allocated, code loaded)
                        wall.append(dt)
                        kern.append(infl.last_kernel_ms)
                hout.close()
                r["members_ms"], r["members_kernel_ms"] = stats(wall), stats(kern)
                d1, d2 = fq.DevText(total + (1 << 20)), fq.DevText(total2 + (1 << 20))
                wall, kern, count, count_rate = [], [], [], []
                for k in range(a.repeats + 1):
                    if d1.avail:
                        d1.take(d1.avail).close()
                    t0 = time.perf_counter()
                    rc, _ = infl.inflate_to(d1, hin.array, ms1)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert rc == 0 and d1.avail == total
                    if k:
                        wall.append(dt)
                        kern.append(infl.last_kernel_ms)
                        count.append(d1.kernel_ms[0])
                        count_rate.append(d1.count_bytes / 1e6 / d1.kernel_ms[0])   # GB/s
                hin.close()
                r["members_dev_ms"], r["members_dev_kernel_ms"] = stats(wall), stats(kern)
                r["count_ms"], r["count_GBps"] = stats(count), stats(count_rate)
                r["count_of_hbm_peak"] = r["count_GBps"]["median"] / a.hbm_peak
                for key in ("members_ms", "members_dev_ms"):
                    r[key.replace("_ms", "_MBps")] = rate(total, r[key])
                r["dev_over_members"] = r["members_ms"]["median"] / r["members_dev_ms"]["median"]
                rc, _ = infl.inflate_to(d2, z2, ms2)
                assert rc == 0
                cut, nblocks = [], 0
                for k in range(a.repeats + 1):
                    blocks, end = d1.cut(a.block_mib << 20, first, mate=d2)
                    assert end == fq.CUT_DONE
                    nblocks = len(blocks)
                    if k:
                        cut.append(d1.kernel_ms[1] * 1e3 / nblocks)
                assert sum(b[0] for b in blocks) == total and sum(b[1] for b in blocks) == total2
                r["cut_blocks"], r["cut_us_per_block"] = nblocks, stats(cut)
                d1.close()
                d2.close()
                note(f"level {level}: members {r['members_ms']['median']:.0f} ms, into a devtext "
                     f"{r['members_dev_ms']['median']:.0f} ms; count {r['count_GBps']['median']:.0f} GB/s; cut "
                     f"{r['cut_us_per_block']['median']:.0f} us a block over {nblocks}")
                # ---- the command line, full -c ----
                p1, p2 = os.path.join(tmp, f"l{level}_1.fq.gz"), os.path.join(tmp, f"l{level}_2.fq.gz")
                with open(p1, "wb") as f:
                    f.write(z1)
                with open(p2, "wb") as f:
                    f.write(z2)
                ways = (("host", []), ("gpu_inflate", ["--gpu-inflate", "-v"]), ("gpu_text", ["--gpu-text", "-v"]))
                cli = {how: [] for how, _ in ways}
                sizes = set()
                for k in range(a.cli_repeats + 1):
                    for how, extra in ways:
                        t0 = time.perf_counter()
                        p = subprocess.run([build.CLI, "-c", "-f", "-t", str(a.threads)] + extra +
                                           ["-1", p1, "-2", p2, "-o", os.path.join(tmp, "x")], capture_output=True, timeout=900)
                        dt = time.perf_counter() - t0
                        if p.returncode != 0:
                            raise SystemExit(f"seqarc_amd {how} failed: {p.stderr.decode()[-500:]}")
                        err = p.stderr.decode().splitlines()
                        line = [ln for ln in err if "block(s), " in ln][0]
                        sizes.add(os.path.getsize(os.path.join(tmp, "x.arc")))
                        if k:
                            cli[how].append({"wall_s": dt, "reported_MBps": float(line.split()[-2]),
                                             "inputs": [ln.split(": ", 1)[1] for ln in err
                                                        if "--gpu-text: " in ln or "sa_inflate_members " in ln]})
                assert len(sizes) == 1, sizes   # (the three ways write archives of one size; the tests compare the bytes)
                r["compress"] = {how: {"wall_s": stats([x["wall_s"] for x in v]),
                                       "reported_MBps": stats([x["reported_MBps"] for x in v])} for how, v in cli.items()}
                r["compress"]["gpu_text"]["inputs_per_run"] = [x["inputs"] for x in cli["gpu_text"]]
                base = r["compress"]["host"]["reported_MBps"]["median"]
                for how in ("gpu_inflate", "gpu_text"):
                    r["compress"][how + "_over_host"] = r["compress"][how]["reported_MBps"]["median"] / base
                note(f"level {level}: -c host {base:.0f} MB/s, --gpu-inflate x{r['compress']['gpu_inflate_over_host']:.2f}, "
                     f"--gpu-text x{r['compress']['gpu_text_over_host']:.2f}")
                os.unlink(p1)
                os.unlink(p2)
                res["levels"][str(level)] = r
    finally:
        infl.close()
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
