"""Host planning checked without a GPU, through tests/cpu_emu: the SEQ bucket
replay's digit width (plan_bkt, sa_plan.h) over every Slevel and SA_BKT_DB
value, and the two inputs that sit on either side of the dense AUX sort's
512-model limit (tests/test_gpu_paths.py runs them on the device)."""
import os
import re
import subprocess

import pytest

import synth
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu") / "emu"
    src = os.path.join(ROOT, "tests", "cpu_emu", "emu.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), src,
                    os.path.join(ROOT, "fastqueeze_amd", "csrc", "fastq_host.cpp"),
                    os.path.join(ROOT, "oracle", "fqz_oracle.c"), os.path.join(ROOT, "oracle", "hash_oracle.c"),
                    os.path.join(ROOT, "oracle", "align_oracle.c"), "-lm"], check=True)
    return str(exe)


def test_bucket_plan_sweep(emu):
    """plan_bkt for Slevel 0..9 x SA_BKT_DB in {unset, 7, 8, 9, 10, 11} x
    SA_SEQ_INV: where the bucket replay applies (contexts of <= 22 bits) a
    wave's models fit the 64 KiB a launch gets without raising the kernel's
    limit, a wave keeps at least 4 context bits, 10 digit bits only with the
    inverse-permutation pass, an override that is refused gives the default,
    and the default is 8 bits up to 20-bit contexts and 9 above."""
    r = subprocess.run([emu, "--bkt-plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [dict(zip(w[0::2], map(int, w[1::2]))) for w in (l.split() for l in r.stdout.splitlines())]
    assert len(rows) == 10 * 6 * 2
    seen = set()
    for p in rows:
        seen.add((p["slevel"], p["env"], p["inv"]))
        assert p["bits"] == (2 * (p["slevel"] + 7)) & 31
        assert p["applies"] == (1 if p["slevel"] <= 4 else 0), p
        default = 8 if p["bits"] <= 20 else 9
        assert p["db"] in (8, 9, 10) and p["sb"] == p["bits"] - p["db"], p
        if p["env"] == 0 or p["env"] not in (8, 9, 10):
            assert p["db"] == default, p
        assert p["db"] in (default, p["env"]), p
        if p["db"] == 10:
            assert p["inv"] == 1 and p["env"] == 10, p
        if p["applies"]:
            assert p["lds"] == 5 * ((1 << p["sb"]) + 64) <= 65536, p
            assert p["sb"] >= 4, p
            # an override the conditions allow is taken
            fits = 5 * ((1 << (p["bits"] - p["env"])) + 64) <= 65536 if 8 <= p["env"] <= 10 else False
            allowed = 8 <= p["env"] <= (10 if p["inv"] else 9) and p["bits"] - p["env"] >= 4 and fits
            assert p["db"] == (p["env"] if allowed else default), p
    assert len(seen) == len(rows)
    # the launch that was rejected: 8 digit bits at Slevel 4 would hold 2^14 contexts, 82,240 B
    s4 = [p for p in rows if p["slevel"] == 4 and p["env"] == 8]
    assert s4 and all(p["db"] == 9 and p["sb"] == 13 and p["lds"] == 41280 for p in s4)


@pytest.mark.parametrize("reads,models", [(synth.MODELS_512_READS, 512), (synth.MODELS_513_READS, 513)])
def test_model_boundary_inputs(emu, tmp_path, reads, models):
    """synth.model_boundary_fastq at its two pinned read counts has exactly 512 /
    513 distinct AUX models in its one block (the same AUX keys the device
    emits, through sa_logic.h), and the decomposition of it equals the oracle."""
    p = tmp_path / "b.fq"
    p.write_bytes(synth.model_boundary_fastq(reads))
    r = subprocess.run([emu, "-M", str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert re.findall(r"^models block (\d+): (\d+)$", r.stdout, re.M) == [("0", str(models))], r.stdout
    r = subprocess.run([emu, str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
