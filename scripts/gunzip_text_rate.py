#!/usr/bin/env python3
"""What keeping GPU-gunzipped text on the device is worth (DESIGN 2.1,
--gpu-text with --gpu-gunzip).

The input is scripts/gunzip_rate.py's: a synthetic PE pair (--text-mib MiB of
FASTQ text over both mates) gzipped at deflate levels 1 and 6, one member per
mate.  Per level, after one warm-up, the median and the spread of
  calls (mate 1 in slabs of 32 MiB, page-locked input; --call-repeats runs)
    run      sa_gunzip_run into a page-locked buffer: wall time, and the sum
             of the five kernels' HIP-event times
    run_dev  sa_gunzip_run_dev into a devtext: wall time (the newline count
             included), the same kernels' sum, and the count's time
  full -c (not ingest-only), three ways alternating in one call
    host        the host inflate (the baseline: code this path does not touch)
    gpu_gunzip  --gpu-gunzip
    gpu_text    --gpu-gunzip --gpu-text, under -v: its per-input lines say
                where the time goes
--parts picks `calls`, `cli` or both.  One JSON document on stdout and in --out
(merged under the key --key when the file exists, so that two input sizes share
a file).  Rates are MB/s of inflated text.
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

from gunzip_rate import SLAB, _gzip, rate, run_file, stats   # noqa: E402

STAGES = ("find_ms", "spec_ms", "chain_ms", "resolve_ms", "crc_ms")


def note(msg):
    print(f"[gunzip_text_rate] {msg}", file=sys.stderr, flush=True)


def run_file_dev(fq, g, hin, n_in, dt):
    """run_file with sa_gunzip_run_dev: the text into the devtext, which is emptied
    after every call (a take of nothing but the read position: not timed apart, it
    is a pointer move and one device-to-device copy the command line makes too).
    (wall ms, kernels' sum ms, newline count ms, calls, text bytes)"""
    state = fq.GunzipState()
    pos, total, calls, kern, count = 0, 0, 0, 0.0, 0.0
    wall_take = 0.0
    t0 = time.perf_counter()
    while True:
        end = min(pos + SLAB, n_in)
        rc, tb, used = g.run_to(dt, hin[pos:end], state, end == n_in)
        if rc:
            raise SystemExit(f"sa_gunzip_run_dev: status {rc} at byte {pos}")
        calls += 1
        kern += sum(g.last_info[k] for k in STAGES)
        count += dt.kernel_ms[0] if tb else 0.0
        t1 = time.perf_counter()
        if dt.avail:
            dt.take(dt.avail).close()
        wall_take += time.perf_counter() - t1
        total += tb
        pos += used
        if state.ended or pos == n_in:
            break
        if not used and not tb:
            raise SystemExit(f"sa_gunzip_run_dev makes no progress at byte {pos} (end_why {g.last_info['end_why']})")
    return (time.perf_counter() - t0 - wall_take) * 1e3, kern, count, calls, total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--text-mib", type=int, default=384, help="384: 2 x 225 MB of text; 3800: 2 x 2.23 GB")
    ap.add_argument("--call-repeats", type=int, default=5)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--parts", default="calls,cli")
    ap.add_argument("--threads", type=int, default=16, help="-t of the command line and the compressing processes")
    ap.add_argument("--key", default=None, help="the result's key in --out (default: text_<MiB>mib)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_text_rate.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")

    import synth
    import fastqueeze_amd as fq
    from fastqueeze_amd import build

    n_pairs = max(1000, a.text_mib * (1 << 20) // 640)   # ~320 bytes a record
    t0 = time.time()
    t1, t2 = synth.generate(n_pairs, paired=True, seed=4242, workers=min(a.threads, 16))
    res = {"text_bytes": [len(t1), len(t2)], "pairs": n_pairs, "generate_s": round(time.time() - t0, 2), "slab": SLAB,
           "levels": {}}
    note(f"{n_pairs} pairs, {len(t1) + len(t2)} bytes of text in {res['generate_s']} s")
    tmp = tempfile.mkdtemp(prefix="gunzip_text_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        with mp.Pool(2) as pool:
            for level in [int(x) for x in a.levels.split(",")]:
                t0 = time.time()
                z1, z2 = pool.map(_gzip, [(t1, level), (t2, level)])
                r = {"gzip_bytes": [len(z1), len(z2)], "compress_s": round(time.time() - t0, 2)}
                note(f"level {level}: {len(z1) + len(z2)} bytes of gzip in {r['compress_s']} s")
                if "calls" in parts:
                    g = fq.Gunzipper(0)
                    hin, hout = fq.HostBuffer(len(z1)), fq.HostBuffer(768 << 20)
                    hin.array[:] = np.frombuffer(z1, np.uint8)
                    dt = fq.DevText(768 << 20)
                    wall, kern, wall_d, kern_d, count_d = [], [], [], [], []
                    for k in range(a.call_repeats + 1):   # (the two calls alternate)
                        ms, stages, calls, _, total = run_file(fq, g, hin.array, len(z1), hout.array)
                        assert total == len(t1)
                        ms_d, k_d, c_d, calls_d, total_d = run_file_dev(fq, g, hin.array, len(z1), dt)
                        assert total_d == len(t1) and calls_d == calls
                        if k:   # (the first run is the warm-up: slabs allocated, code loaded)
                            wall.append(ms)
                            kern.append(sum(stages.values()))
                            wall_d.append(ms_d)
                            kern_d.append(k_d)
                            count_d.append(c_d)
                    for x in (dt, hin, hout, g):
                        x.close()
                    c = {"calls": calls, "run_ms": stats(wall), "run_kernels_ms": stats(kern), "run_dev_ms": stats(wall_d),
                         "run_dev_kernels_ms": stats(kern_d), "run_dev_count_ms": stats(count_d)}
                    c["run_MBps"], c["run_dev_MBps"] = rate(len(t1), c["run_ms"]), rate(len(t1), c["run_dev_ms"])
                    c["dev_over_run"] = c["run_ms"]["median"] / c["run_dev_ms"]["median"]
                    r["call"] = c
                    note(f"level {level}: sa_gunzip_run {c['run_ms']['median']:.0f} ms (kernels "
                         f"{c['run_kernels_ms']['median']:.1f}), sa_gunzip_run_dev {c['run_dev_ms']['median']:.0f} ms (kernels "
                         f"{c['run_dev_kernels_ms']['median']:.1f}, count {c['run_dev_count_ms']['median']:.2f})")
                if "cli" in parts:
                    p1, p2 = os.path.join(tmp, f"l{level}_1.fq.gz"), os.path.join(tmp, f"l{level}_2.fq.gz")
                    with open(p1, "wb") as f:
                        f.write(z1)
                    with open(p2, "wb") as f:
                        f.write(z2)
                    ways = (("host", []), ("gpu_gunzip", ["--gpu-gunzip", "-v"]),
                            ("gpu_text", ["--gpu-gunzip", "--gpu-text", "-v"]))
                    cli = {how: [] for how, _ in ways}
                    sizes = set()
                    for k in range(a.cli_repeats + 1):
                        for how, extra in ways:
                            t0 = time.perf_counter()
                            p = subprocess.run([build.CLI, "-c", "-f", "-t", str(a.threads)] + extra +
                                               ["-1", p1, "-2", p2, "-o", os.path.join(tmp, "x")], capture_output=True, timeout=900)
                            dt_s = time.perf_counter() - t0
                            if p.returncode != 0:
                                raise SystemExit(f"seqarc_amd {how} failed: {p.stderr.decode()[-500:]}")
                            err = p.stderr.decode().splitlines()
                            line = [ln for ln in err if "block(s), " in ln][0]
                            sizes.add(os.path.getsize(os.path.join(tmp, "x.arc")))
                            note(f"level {level} run {k} {how}: {dt_s:.1f} s, {line.split()[-2]} MB/s")
                            if k:
                                cli[how].append({"wall_s": dt_s, "reported_MBps": float(line.split()[-2]),
                                                 "inputs": [ln.split(": ", 1)[1] for ln in err
                                                            if "sa_gunzip_run" in ln or "the host takes over" in ln]})
                    assert len(sizes) == 1, sizes   # (the three ways write archives of one size; the tests compare the bytes)
                    r["compress"] = {how: {"wall_s": stats([x["wall_s"] for x in v]),
                                           "reported_MBps": stats([x["reported_MBps"] for x in v])} for how, v in cli.items()}
                    for how in ("gpu_gunzip", "gpu_text"):
                        r["compress"][how]["inputs_last_run"] = cli[how][-1]["inputs"]
                    base = r["compress"]["host"]["reported_MBps"]["median"]
                    for how in ("gpu_gunzip", "gpu_text"):
                        r["compress"][how + "_over_host"] = r["compress"][how]["reported_MBps"]["median"] / base
                    r["compress"]["gpu_text_over_gpu_gunzip"] = (r["compress"]["gpu_text"]["reported_MBps"]["median"] /
                                                                 r["compress"]["gpu_gunzip"]["reported_MBps"]["median"])
                    note(f"level {level}: -c host {base:.0f} MB/s, --gpu-gunzip x{r['compress']['gpu_gunzip_over_host']:.2f}, "
                         f"with --gpu-text x{r['compress']['gpu_text_over_host']:.2f}")
                    os.unlink(p1)
                    os.unlink(p2)
                res["levels"][str(level)] = r
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
    key = a.key or f"text_{a.text_mib}mib"
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[key] = res
    text = json.dumps(doc, indent=1)
    print(json.dumps({key: res}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
