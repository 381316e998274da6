#!/usr/bin/env python3
"""Rate of the device block decode against the host decode.

The synthetic PE pair of scripts/inflate_rate.py (--text-mib MiB of FASTQ text
over both mates; the default 4,460 MiB gives about 85 blocks of 50 MiB) is
written to tmpfs and encoded once with the defaults by seqarc_amd -c.  Then
  (a) sa_decode_blocks: one seqarc_amd -d --gpu-decode -v run, whose last line
      carries sa_decode_info summed over the calls: per-phase ms, launches,
      blocks in flight.  From them: the mean launch time of a QUAL and of a SEQ
      slice (every launch but a chain's last decodes `slice` symbols a wave, so
      the mean is close to the slowest), and symbols per second per wave =
      slice / that time (the slowest wave of a launch).  With --qlevel3 the
      same for an archive made and decoded with --qlevel 3, whose QUAL launch
      is the slowest one there is (the 302 MB table): SA_DEC_SLICE's default is
      the largest power of two that keeps it under 250 ms.
  (b) seqarc_amd -d -t T against seqarc_amd -d -t T --gpu-decode, alternating,
      one warm-up each, --repeats runs: wall seconds, median and range, MB/s
      of FASTQ text.  The outputs of both are compared byte for byte once.
One JSON document on stdout and in --out."""
import argparse
import filecmp
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INFO = re.compile(r"sa_decode_blocks: (.*)$", re.M)


def note(msg):
    print(f"[decode_rate] {msg}", file=sys.stderr, flush=True)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def run(cmd, env=None):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}: exit {p.returncode}\n{p.stderr[-2000:]}")
    return dt, p.stderr


def info_of(stderr):
    m = INFO.search(stderr)
    if not m:
        raise SystemExit("no sa_decode_blocks line in the -v output:\n" + stderr[-2000:])
    d = {}
    for part in m.group(1).split(", "):
        k, v = part.rsplit(" ", 1)
        d[k] = float(v) if "." in v else int(v)
    host = len(re.findall(r"the host decodes it", stderr))
    d["host_blocks"] = host
    return d


def derive(i):
    """Mean launch times and the per-wave rates from an info dict."""
    out = dict(i)
    for ch in ("qual", "seq"):
        n = i[f"{ch}_launches"]
        ms = i[f"{ch}_ms"] / n if n else 0.0
        out[f"{ch}_launch_ms_mean"] = ms
        out[f"{ch}_symbols_per_s_per_wave"] = i["slice"] / (ms / 1e3) if ms else 0.0
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--text-mib", type=int, default=4460)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--qlevel3", action="store_true", help="also one device run of an archive made with --qlevel 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_rate.json"))
    a = ap.parse_args()

    import synth
    from fastqueeze_amd import build

    cli = build.CLI
    n_pairs = max(1000, a.text_mib * (1 << 20) // 640)   # ~320 bytes a record
    t0 = time.time()
    t1, t2 = synth.generate(n_pairs, paired=True, seed=4242, workers=min(a.threads, 16))
    text = len(t1) + len(t2)
    res = {"text_bytes": [len(t1), len(t2)], "pairs": n_pairs, "generate_s": round(time.time() - t0, 2), "threads": a.threads,
           "slice_env": os.environ.get("SA_DEC_SLICE"), "inflight_env": os.environ.get("SA_DEC_INFLIGHT")}
    note(f"{n_pairs} pairs, {text} bytes of text in {res['generate_s']} s")
    tmp = tempfile.mkdtemp(prefix="decode_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        p1, p2 = os.path.join(tmp, "r_1.fq"), os.path.join(tmp, "r_2.fq")
        with open(p1, "wb") as f:
            f.write(t1)
        with open(p2, "wb") as f:
            f.write(t2)
        del t1, t2
        arc = os.path.join(tmp, "r")
        dt, _ = run([cli, "-c", "-f", "-t", str(a.threads), "-1", p1, "-2", p2, "-o", arc])
        res["encode_s"] = round(dt, 2)
        res["arc_bytes"] = os.path.getsize(arc + ".arc")
        note(f"encoded in {dt:.1f} s: {res['arc_bytes']} bytes")
        host = [cli, "-d", "-f", "-t", str(a.threads), arc + ".arc", os.path.join(tmp, "h")]
        dev = [cli, "-d", "-f", "-v", "-t", str(a.threads), "--gpu-decode", arc + ".arc", os.path.join(tmp, "g")]
        th, tg, infos = [], [], []
        for k in range(a.repeats + 1):   # (run 0 of each is the warm-up)
            dt, _ = run(host)
            dg, err = run(dev)
            note(f"run {k}: host {dt:.2f} s, device {dg:.2f} s")
            if k == 0:
                same = all(filecmp.cmp(os.path.join(tmp, f"h_{m}.fastq"), os.path.join(tmp, f"g_{m}.fastq"), shallow=False) and
                           filecmp.cmp(os.path.join(tmp, f"h_{m}.fastq"), p, shallow=False) for m, p in ((1, p1), (2, p2)))
                res["outputs_equal_the_input"] = same
                if not same:
                    raise SystemExit("the decoded files differ")
                continue
            th.append(dt)
            tg.append(dg)
            infos.append(info_of(err))
        res["a_sa_decode_blocks"] = derive(infos[len(infos) // 2])
        res["b_cli"] = {"host_s": stats(th), "gpu_decode_s": stats(tg),
                        "host_MBps": text / 1e6 / statistics.median(th), "gpu_decode_MBps": text / 1e6 / statistics.median(tg)}
        note(json.dumps(res["b_cli"]))
        if a.qlevel3:
            for f in ("h_1.fastq", "h_2.fastq", "g_1.fastq", "g_2.fastq"):
                os.remove(os.path.join(tmp, f))
            run([cli, "-c", "-f", "-t", str(a.threads), "--qlevel", "3", "-1", p1, "-2", p2, "-o", arc + "q3"])
            dg, err = run(dev[:1] + ["--qlevel", "3"] + dev[1:-2] + [arc + "q3.arc", os.path.join(tmp, "q")])
            ok = filecmp.cmp(os.path.join(tmp, "q_1.fastq"), p1, shallow=False)
            res["qlevel3"] = dict(derive(info_of(err)), wall_s=round(dg, 2), output_equals_the_input=ok)
            note(json.dumps(res["qlevel3"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
