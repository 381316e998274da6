#!/usr/bin/env python3
"""Rate of the device BGZF inflate against the host inflate.

Builds the BGZF of a synthetic PE pair (--text-mib MiB of FASTQ text over both
mates, bgzip's 65,280-byte members; the default 3,800 MiB gives about 1 GiB of
BGZF, so that start-up costs are small in the runs) at deflate levels 1 and 6 and reports, per
level, after one warm-up, the median and the spread (min .. max) of --repeats
runs of
  kernel   k_inflate_bgzf alone (sa_inflater_kernel_ms, HIP events) on mate 1
  call     sa_inflate_members on mate 1, wall time with the H2D and D2H copies,
           from pageable numpy buffers and from sa_host_alloc (page-locked) ones
  ingest   seqarc_amd -c --ingest-only on the pair, without (the host inflate:
           the baseline) and with --gpu-inflate, alternating in the same call;
           the switch's runs under -v, whose per-input line says where the
           time went (inflater create, slab allocation, sa_inflate_members,
           host copy, queue wait, waiting for slabs)
One JSON document on stdout and in --out.  Rates are MB/s of inflated text.
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _members(args):
    data, level = args
    out = bytearray()
    for i in range(0, len(data), 65280):
        part = data[i:i + 65280]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        cd = c.compress(part) + c.flush()
        out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
        out += struct.pack("<H", 18 + len(cd) + 8 - 1) + cd + struct.pack("<II", zlib.crc32(part), len(part))
    return bytes(out)


def bgzf(text: bytes, level: int, pool) -> bytes:
    step = 65280 * 256
    parts = pool.map(_members, [(text[i:i + step], level) for i in range(0, len(text), step)])
    return b"".join(parts) + EOF_MEMBER


def note(msg):
    print(f"[inflate_rate] {msg}", file=sys.stderr, flush=True)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def rate(nbytes, ms):
    """MB/s at the median time, and at the slowest and the fastest run."""
    return {"median": nbytes / 1e3 / ms["median"], "low": nbytes / 1e3 / ms["max"], "high": nbytes / 1e3 / ms["min"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--text-mib", type=int, default=3800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--threads", type=int, default=16, help="-t of the command line and the compressing processes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_rate.json"))
    a = ap.parse_args()

    import synth
    import fastqueeze_amd as fq
    from fastqueeze_amd import build

    n_pairs = max(1000, a.text_mib * (1 << 20) // 640)   # ~320 bytes a record
    t0 = time.time()
    t1, t2 = synth.generate(n_pairs, paired=True, seed=4242, workers=min(a.threads, 16))
    res = {"text_bytes": [len(t1), len(t2)], "pairs": n_pairs, "generate_s": round(time.time() - t0, 2), "levels": {}}
    note(f"{n_pairs} pairs, {len(t1) + len(t2)} bytes of text in {res['generate_s']} s")
    infl = fq.Inflater(0)
    tmp = tempfile.mkdtemp(prefix="inflate_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        with mp.Pool(min(a.threads, 16)) as pool:
            for level in [int(x) for x in a.levels.split(",")]:
                t0 = time.time()
                z1, z2 = bgzf(t1, level, pool), bgzf(t2, level, pool)
                r = {"bgzf_bytes": [len(z1), len(z2)], "compress_s": round(time.time() - t0, 2)}
                ms, consumed, total = fq.bgzf_scan(z1)
                assert consumed == len(z1) and total == len(t1)
                r["members"] = int(ms.size)
                note(f"level {level}: {len(z1) + len(z2)} bytes of BGZF in {r['compress_s']} s")
                # pageable buffers
                out = np.empty(total, np.uint8)
                kern, wall = [], []
                for k in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    rc, _ = infl.inflate_into(z1, ms, out)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert rc == 0
                    if k:   # (the first run is the warm-up: slabs allocated, code loaded)
                        kern.append(infl.last_kernel_ms)
                        wall.append(dt)
                assert zlib.crc32(out) == zlib.crc32(t1)
                r["kernel_ms"], r["call_pageable_ms"] = stats(kern), stats(wall)
                # page-locked buffers
                hin, hout = fq.HostBuffer(len(z1)), fq.HostBuffer(total)
                hin.array[:] = np.frombuffer(z1, np.uint8)
                wall = []
                for k in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    rc, _ = infl.inflate_into(hin.array, ms, hout.array)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert rc == 0
                    if k:
                        wall.append(dt)
                assert zlib.crc32(hout.array) == zlib.crc32(t1)
                hin.close()
                hout.close()
                r["call_pinned_ms"] = stats(wall)
                note(f"level {level}: kernel {r['kernel_ms']['median']:.1f} ms, call {r['call_pinned_ms']['median']:.1f} ms")
                for key in ("kernel_ms", "call_pageable_ms", "call_pinned_ms"):
                    r[key.replace("_ms", "_MBps")] = rate(total, r[key])
                # the command line's ingest, host inflate and device inflate alternating
                p1, p2 = os.path.join(tmp, f"l{level}_1.fq.gz"), os.path.join(tmp, f"l{level}_2.fq.gz")
                with open(p1, "wb") as f:
                    f.write(z1)
                with open(p2, "wb") as f:
                    f.write(z2)
                cli = {"host": [], "gpu": []}
                for k in range(a.cli_repeats + 1):
                    for how, extra in (("host", []), ("gpu", ["--gpu-inflate", "-v"])):
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
                                             "inputs": [ln.split("--gpu-inflate: ", 1)[1] for ln in
                                                        p.stderr.decode().splitlines() if "sa_inflate_members" in ln]})
                r["ingest"] = {how: {"wall_s": stats([x["wall_s"] for x in v]),
                                     "reported_MBps": stats([x["reported_MBps"] for x in v])} for how, v in cli.items()}
                r["ingest"]["gpu"]["inputs_per_run"] = [x["inputs"] for x in cli["gpu"]]
                r["ingest"]["gpu_over_host"] = (r["ingest"]["gpu"]["reported_MBps"]["median"] /
                                                r["ingest"]["host"]["reported_MBps"]["median"])
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
