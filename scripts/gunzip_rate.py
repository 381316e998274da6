#!/usr/bin/env python3
"""Rate of the device gunzip (ordinary gzip, by speculation) against the host
inflate.

Gzips a synthetic PE pair (--text-mib MiB of FASTQ text over both mates) at
deflate levels 1 and 6, each as one member per mate and as members of 16 MiB of
text (bench.py's form), and reports per level and form, for each chunk size of
--chunks (SA_GUNZIP_CHUNK, read when a gunzipper is created), after one
warm-up, the median and the spread (min .. max) of --repeats runs of
  kernels  the five kernels alone, staged: the sum of their HIP-event times
           over the calls of mate 1 (k_gz_find, k_gz_spec, k_gz_chain,
           k_gz_resolve, k_gz_crc), and each stage's share
  call     sa_gunzip_run over mate 1 in slabs of 32 MiB, wall time with the
           H2D and D2H copies, from sa_host_alloc (page-locked) buffers
  ingest   seqarc_amd -c --ingest-only -t 16 on the pair, without (the host
           inflate: the baseline) and with --gpu-gunzip, alternating in the
           same call; the switch's runs under -v, whose per-input line says
           where the time went
One JSON document on stdout and in --out.  Rates are MB/s of inflated text.
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLAB = 32 << 20
MEMBER_TEXT = 16 << 20


def _gzip(args):
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def note(msg):
    print(f"[gunzip_rate] {msg}", file=sys.stderr, flush=True)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def rate(nbytes, ms):
    """MB/s at the median time, and at the slowest and the fastest run."""
    return {"median": nbytes / 1e3 / ms["median"], "low": nbytes / 1e3 / ms["max"], "high": nbytes / 1e3 / ms["min"]}


def run_file(fq, g, hin, n_in, hout):
    """sa_gunzip_run over hin[0..n_in) in slabs, each call starting where the last
    one's confirmed prefix ended: (wall ms, per-stage kernel ms, calls, CRC-32 and
    length of the text)."""
    state = fq.GunzipState()
    pos, crc, total, calls = 0, 0, 0, 0
    stages = dict.fromkeys(("find_ms", "spec_ms", "chain_ms", "resolve_ms", "crc_ms"), 0.0)
    t0 = time.perf_counter()
    wall_crc = 0.0
    while True:
        end = min(pos + SLAB, n_in)
        rc, ob, used = g.run(hin[pos:end], state, hout, end == n_in)
        if rc:
            raise SystemExit(f"sa_gunzip_run: status {rc} at byte {pos}")
        calls += 1
        for k in stages:
            stages[k] += g.last_info[k]
        t1 = time.perf_counter()
        crc = zlib.crc32(hout[:ob], crc)   # (not part of the call: taken out of the wall time)
        wall_crc += time.perf_counter() - t1
        total += ob
        pos += used
        if state.ended or pos == n_in:
            break
        if not used and not ob:
            raise SystemExit(f"sa_gunzip_run makes no progress at byte {pos} (end_why {g.last_info['end_why']})")
    return (time.perf_counter() - t0 - wall_crc) * 1e3, stages, calls, crc, total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--text-mib", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--chunks", default="65536,262144,1048576")
    ap.add_argument("--threads", type=int, default=16, help="-t of the command line and the compressing processes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_rate.json"))
    a = ap.parse_args()

    import synth
    import fastqueeze_amd as fq
    from fastqueeze_amd import build

    n_pairs = max(1000, a.text_mib * (1 << 20) // 640)   # ~320 bytes a record
    t0 = time.time()
    t1, t2 = synth.generate(n_pairs, paired=True, seed=4242, workers=min(a.threads, 16))
    res = {"text_bytes": [len(t1), len(t2)], "pairs": n_pairs, "generate_s": round(time.time() - t0, 2), "slab": SLAB,
           "levels": {}}
    note(f"{n_pairs} pairs, {len(t1) + len(t2)} bytes of text in {res['generate_s']} s")
    chunks = [int(x) for x in a.chunks.split(",")]
    tmp = tempfile.mkdtemp(prefix="gunzip_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    hout = fq.HostBuffer(768 << 20)
    try:
        with mp.Pool(min(a.threads, 16)) as pool:
            for level in [int(x) for x in a.levels.split(",")]:
                t0 = time.time()
                jobs = [(t, level) for t in (t1, t2)]
                for t in (t1, t2):
                    jobs += [(t[i:i + MEMBER_TEXT], level) for i in range(0, len(t), MEMBER_TEXT)]
                done = pool.map(_gzip, jobs)
                n1 = -(-len(t1) // MEMBER_TEXT)
                forms = {"one_member": (done[0], done[1]),
                         "members_16mib": (b"".join(done[2:2 + n1]), b"".join(done[2 + n1:]))}
                note(f"level {level}: compressed in {time.time() - t0:.1f} s")
                res["levels"][str(level)] = {}
                for form, (z1, z2) in forms.items():
                    r = {"gzip_bytes": [len(z1), len(z2)], "chunks": {}}
                    hin = fq.HostBuffer(len(z1))
                    hin.array[:] = np.frombuffer(z1, np.uint8)
                    p1, p2 = os.path.join(tmp, "r_1.fq.gz"), os.path.join(tmp, "r_2.fq.gz")
                    with open(p1, "wb") as f:
                        f.write(z1)
                    with open(p2, "wb") as f:
                        f.write(z2)
                    for chunk in chunks:
                        os.environ["SA_GUNZIP_CHUNK"] = str(chunk)
                        g = fq.Gunzipper(0)
                        assert g.chunk == chunk
                        kern, wall, per_stage = [], [], []
                        for k in range(a.repeats + 1):
                            ms, stages, calls, crc, total = run_file(fq, g, hin.array, len(z1), hout.array)
                            assert total == len(t1) and crc == zlib.crc32(t1)
                            if k:   # (the first run is the warm-up: slabs allocated, code loaded)
                                kern.append(sum(stages.values()))
                                wall.append(ms)
                                per_stage.append(stages)
                        g.close()
                        c = {"calls": calls, "kernels_ms": stats(kern), "call_pinned_ms": stats(wall),
                             "stage_ms_median": {k: statistics.median(s[k] for s in per_stage) for k in per_stage[0]}}
                        c["kernels_MBps"] = rate(len(t1), c["kernels_ms"])
                        c["call_pinned_MBps"] = rate(len(t1), c["call_pinned_ms"])
                        # the command line's ingest, host inflate and device gunzip alternating
                        cli = {"host": [], "gpu": []}
                        for k in range(a.cli_repeats + 1):
                            for how, extra in (("host", []), ("gpu", ["--gpu-gunzip", "-v"])):
                                t0 = time.perf_counter()
                                p = subprocess.run([build.CLI, "-c", "-f", "--ingest-only", "-t", str(a.threads)] + extra +
                                                   ["-1", p1, "-2", p2, "-o", os.path.join(tmp, "x")], capture_output=True,
                                                   timeout=600)
                                dt = time.perf_counter() - t0
                                if p.returncode != 0:
                                    raise SystemExit(f"seqarc_amd {how} failed: {p.stderr.decode()[-500:]}")
                                line = [ln for ln in p.stderr.decode().splitlines() if "block(s)" in ln][0]
                                if k:
                                    cli[how].append({"wall_s": dt, "reported_MBps": float(line.split()[-2]),
                                                     "inputs": [ln.split("--gpu-gunzip: ", 1)[1] for ln in
                                                                p.stderr.decode().splitlines() if "sa_gunzip_run" in ln]})
                        c["ingest"] = {how: {"wall_s": stats([x["wall_s"] for x in v]),
                                             "reported_MBps": stats([x["reported_MBps"] for x in v])} for how, v in cli.items()}
                        c["ingest"]["gpu"]["inputs_last_run"] = cli["gpu"][-1]["inputs"]
                        c["ingest"]["gpu_over_host"] = (c["ingest"]["gpu"]["reported_MBps"]["median"] /
                                                        c["ingest"]["host"]["reported_MBps"]["median"])
                        note(f"level {level} {form} chunk {chunk}: kernels {c['kernels_MBps']['median']:.0f} MB/s, call "
                             f"{c['call_pinned_MBps']['median']:.0f} MB/s, ingest gpu/host {c['ingest']['gpu_over_host']:.2f}")
                        r["chunks"][str(chunk)] = c
                    hin.close()
                    os.unlink(p1)
                    os.unlink(p2)
                    res["levels"][str(level)][form] = r
    finally:
        hout.close()
        os.environ.pop("SA_GUNZIP_CHUNK", None)
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
