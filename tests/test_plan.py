"""Host planning checked without a GPU, through tests/cpu_emu: the SEQ bucket
replay's digit width (plan_bkt, sa_plan.h) over every Slevel and SA_BKT_DB
value, the knob table (parse_knobs, sa_knobs.h) over every SA_* value the
engine reads, the path plan (plan_paths / plan_totals / report_paths) over
every Slevel, Qlevel and front knob, and the two inputs that sit on either side
of the dense AUX sort's 512-model limit (tests/test_gpu_paths.py runs them on
the device).  The two sweeps also run once in an address + undefined-behaviour
sanitizer build of the same stand-alone program."""
import os
import re
import subprocess

import pytest

import synth
from conftest import ROOT


def _build_emu(exe, flags):
    src = os.path.join(ROOT, "tests", "cpu_emu", "emu.cpp")
    subprocess.run(["g++", *flags, "-std=c++17", "-o", str(exe), src,
                    os.path.join(ROOT, "fastqueeze_amd", "csrc", "fastq_host.cpp"),
                    os.path.join(ROOT, "oracle", "fqz_oracle.c"), os.path.join(ROOT, "oracle", "hash_oracle.c"),
                    os.path.join(ROOT, "oracle", "align_oracle.c"), "-lm"], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build_emu(tmp_path_factory.mktemp("emu") / "emu", ["-O2"])


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return _build_emu(tmp_path_factory.mktemp("emu_san") / "emu_san",
                      ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


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


# ---- the knob table (sa_knobs.h) ---------------------------------------------------------------

def _rows(exe, mode, env):
    """emu's `name value ...` lines under exactly `env`, as dicts of ints"""
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=dict(env))
    assert r.returncode == 0 and r.stderr == "", (env, r.stderr[-2000:])
    return [dict(zip(w[0::2], map(int, w[1::2]))) for w in (l.split() for l in r.stdout.splitlines())]


U32, U64 = 1 << 32, 1 << 64
# What sa_engine.hip read before the table existed, and DESIGN.md's knob table: every field with no knob set
KNOB_DEFAULTS = dict(
    aux_dense=1, chain_prio=1, md5_prio=1, prep_fused=0, prep_wave=0, emit_wave=0, l_chunk=32, l_prio=0, seq_unpacked=0,
    front_static=0, wq_chunk_env=0, rv_lanes=0, seq_bucket=1, seq_inv=1, bkt_db_env=0, prep_row=0, bkt_lpt=1, bkt_probe=0,
    wg_per_cu=8, md5_pipe=0, host_waits=1, coder_waves=4, coder_lds=82 * 1024, rv_variant=-1, rv_v6_max=1 << 30,
    rv_wait_ticks=2_000_000_000, test_skip_long=0, rv_short_waves=32, trace=0, rv_probe=0, rb_apply_walk=0,
    rb_fix_serial=0, rb_spec_wg=2, rb_chunk=7904, long_cu_every=4, long_lds=0, rv_cus=0, long_grid_env=0, l_cu_every=0,
    payload_slack=4096, find_runs=0, aln_trace=0, batch_bases=U64 - 1, sort_min_db=7)


def _vals(zero, one, below, above, text):
    return {"0": zero, "1": one, "-5": below, "99": above, "x": text}


def _set_at_all(field):          # true when merely set, "0" included
    return field, _vals(1, 1, 1, 1, 1)


def _on_if_nonzero(field):       # set and not 0; text reads as 0
    return field, _vals(0, 1, 1, 1, 0)


def _off_if_zero(field):         # on unless set and 0; text reads as 0
    return field, _vals(0, 1, 1, 1, 0)


def _raw(field, below=-5):       # atoi as it comes (an unsigned field wraps)
    return field, _vals(0, 1, below, 99, 0)


# knob -> (field, {value: what the field must be}); "-5" is below every range, "99" (or the extra
# entries) above the ranges that have a top, "x" is not a number
KNOBS = {
    "SA_AUX_DENSE": _off_if_zero("aux_dense"),
    "SA_CHAIN_PRIO": _off_if_zero("chain_prio"),
    "SA_MD5_PRIO": _on_if_nonzero("md5_prio"),
    "SA_PREP_FUSED": _set_at_all("prep_fused"),
    "SA_PREP_WAVE": _set_at_all("prep_wave"),
    "SA_EMIT_WAVE": _set_at_all("emit_wave"),
    "SA_TEST_SKIP_LONG": _set_at_all("test_skip_long"),
    "SA_TRACE": _set_at_all("trace"),
    "SA_BKT_PROBE": _set_at_all("bkt_probe"),
    "SA_RV_PROBE": _set_at_all("rv_probe"),
    "SA_FIND_RUNS": _set_at_all("find_runs"),
    "SA_ALN_TRACE": _set_at_all("aln_trace"),
    "SA_L_CHUNK": ("l_chunk", dict(_vals(32, 32, 32, 32, 32), **{"16": 16, "8": 32, "64": 32})),
    "SA_L_PRIO": _on_if_nonzero("l_prio"),
    "SA_SEQ_PACK": ("seq_unpacked", _vals(1, 0, 0, 0, 1)),
    "SA_FRONT_STATIC": _on_if_nonzero("front_static"),
    "SA_WQ_CHUNK": _raw("wq_chunk_env", U32 - 5),
    "SA_RV_LANES": _on_if_nonzero("rv_lanes"),
    "SA_SEQ_BUCKET": _off_if_zero("seq_bucket"),
    "SA_SEQ_INV": _off_if_zero("seq_inv"),
    "SA_BKT_LPT": _off_if_zero("bkt_lpt"),
    "SA_HOST_WAITS": _off_if_zero("host_waits"),
    "SA_BKT_DB": _raw("bkt_db_env"),
    "SA_PREP_ROW": _raw("prep_row"),
    "SA_WAVE_GRID": ("wg_per_cu", _vals(1, 1, 1, 99, 1)),
    "SA_MD5_PIPE": _on_if_nonzero("md5_pipe"),
    "SA_CODER_WAVES": ("coder_waves", dict(_vals(4, 1, 4, 4, 4), **{"2": 2, "3": 4})),
    "SA_CODER_LDS": ("coder_lds", dict(_vals(0, 1, 0, 99, 0), **{"999999": 160 * 1024, "163840": 160 * 1024})),
    "SA_RV_VARIANT": _raw("rv_variant"),
    "SA_RV_V6_MAX": _raw("rv_v6_max"),
    # ms -> ticks of the 100 MHz clock, at least 1 ms, at most 4e9 ticks
    "SA_RV_WAIT_MS": ("rv_wait_ticks", dict(_vals(100_000, 100_000, 100_000, 9_900_000, 100_000),
                                            **{"300": 30_000_000, "1000000000": 4_000_000_000})),
    "SA_RV_SHORT_WAVES": _raw("rv_short_waves", U32 - 5),
    "SA_RB_APPLY": _on_if_nonzero("rb_apply_walk"),
    "SA_RB_FIX_SERIAL": _on_if_nonzero("rb_fix_serial"),
    "SA_RB_SPEC_WG": ("rb_spec_wg", _vals(0, 1, 0, 99, 0)),
    # a multiple of 32 within 32..8192 (RB_CHUNK), otherwise 8192; unset: 7904
    "SA_RB_CHUNK": ("rb_chunk", dict(_vals(8192, 8192, 8192, 8192, 8192),
                                     **{"32": 32, "33": 8192, "4096": 4096, "8192": 8192, "8224": 8192, str(1 << 20): 8192})),
    "SA_LONG_CU_EVERY": ("long_cu_every", _vals(1, 1, 1, 99, 1)),
    "SA_LONG_LDS": _raw("long_lds", U32 - 5),
    "SA_RV_CUS": _raw("rv_cus"),
    "SA_LONG_GRID": ("long_grid_env", _vals(1, 1, 1, 99, 1)),
    "SA_L_CU_EVERY": _raw("l_cu_every"),
    "SA_PAYLOAD_SLACK": ("payload_slack", _vals(0, 1, U64 - 5, 99, 0)),           # (strtoull)
    "SA_BATCH_BASES": ("batch_bases", _vals(U64 - 1, 1, U64 - 5, 99, U64 - 1)),    # (0: no cap)
    "SA_SORT_MIN_DB": ("sort_min_db", dict(_vals(7, 7, 7, 9, 7), **{"8": 8, "9": 9, "10": 9})),
}


def _check_knobs(exe):
    got = _rows(exe, "--knobs", {})
    assert got == [KNOB_DEFAULTS]
    assert sorted(f for f, _ in KNOBS.values()) == sorted(KNOB_DEFAULTS)      # every field has its knob
    for knob, (field, cases) in KNOBS.items():
        assert {"0", "1", "-5", "99", "x"} <= set(cases)
        for value, want in cases.items():
            expect = dict(KNOB_DEFAULTS, **{field: want})
            if knob == "SA_CHAIN_PRIO":
                expect["md5_prio"] = want                                     # (SA_MD5_PRIO unset: follows it)
            assert _rows(exe, "--knobs", {knob: value}) == [expect], (knob, value)
    # SA_MD5_PRIO follows SA_CHAIN_PRIO=0 unless it is set itself
    both = _rows(exe, "--knobs", {"SA_CHAIN_PRIO": "0", "SA_MD5_PRIO": "1"})[0]
    assert (both["chain_prio"], both["md5_prio"]) == (0, 1)
    both = _rows(exe, "--knobs", {"SA_CHAIN_PRIO": "1", "SA_MD5_PRIO": "0"})[0]
    assert (both["chain_prio"], both["md5_prio"]) == (1, 0)


def test_knob_table(emu):
    """parse_knobs / parse_run_knobs on each SA_* knob alone, unset and set to
    "0", "1", a value below its range, one above it and one that is no number
    (and the values the clamps turn on): the field has the value written here
    -- from the engine's parsing before the table existed and DESIGN.md's knob
    table -- and every other field keeps its default."""
    _check_knobs(emu)


# ---- the path plan (sa_plan.h) -----------------------------------------------------------------

PREP = {"row16": 1, "row64": 2, "fused": 3, "wave": 4}
EMIT = {"row16": 1, "wave": 2}
SEQ_REPLAY = {"bucket": 1, "full": 2}
AUX_SORT = {"dense1": 1, "dense2+copy": 2, "raw": 3}
AUX_RUNS = {"runs_dense": 1, "find_runs": 2}
MD5 = {None: 0, "plain": 1, "pipe": 2}
NAMED = dict(prep=PREP, emit=EMIT, seq_replay=SEQ_REPLAY, aux_sort=AUX_SORT, aux_runs=AUX_RUNS, md5=MD5)

# tests/test_gpu_paths.py: DEFAULT (its fields the plan decides), RAW17 / RAW21 and the `expect` of its
# FRONT cases and of seq_unpacked-s3 / -s8, full_sort-s0, bucket-s0-s2 and packed-s7: (env, slevel, qlevel, expect)
DEFAULT = dict(prep="row16", front_counter=1, wg_per_cu=8, emit="row16", seq_packed=1, seq_replay="bucket",
               bkt_inv=1, bkt_lpt=1, bkt_db=8, bkt_sb=12, host_waits=1, md5="plain", rblock=0, front_masked=0)
RAW17 = dict(aux_sort="raw", aux_runs="find_runs", aux_digits=0x89)
RAW21 = dict(aux_sort="raw", aux_runs="find_runs", aux_digits=0x777)
PATH_CASES = [
    ({}, 3, 2, dict(DEFAULT, dege_list=1)),
    ({"SA_PREP_FUSED": "1"}, 3, 2, dict(prep="fused", front_counter=1)),
    ({"SA_PREP_FUSED": "0"}, 3, 2, dict(prep="fused", front_counter=1)),       # (on: it is set)
    ({"SA_PREP_FUSED": "1"}, 3, 3, dict(prep="fused")),
    ({"SA_PREP_WAVE": "1"}, 3, 2, dict(prep="wave", emit="row16", dege_list=0)),
    ({"SA_PREP_ROW": "64"}, 3, 2, dict(prep="row64", emit="row16", front_counter=1)),
    ({"SA_EMIT_WAVE": "1"}, 3, 3, dict(prep="row16", emit="wave", dege_list=0)),
    ({"SA_EMIT_WAVE": "1"}, 1, 2, dict(prep="row16", emit="wave", dege_list=0)),
    ({"SA_EMIT_WAVE": "1", "SA_PREP_WAVE": "1"}, 3, 3, dict(prep="wave", emit="wave", dege_list=0, front_counter=0)),
    ({"SA_EMIT_WAVE": "1", "SA_PREP_WAVE": "1"}, 1, 2, dict(prep="wave", emit="wave", dege_list=0, front_counter=0)),
    ({"SA_SEQ_PACK": "0"}, 3, 2, dict(seq_packed=0, seq_replay="full", seq_digits=0x777)),
    ({"SA_SEQ_PACK": "0"}, 8, 2, dict(seq_packed=0, seq_replay="full", seq_digits=0x7788)),
    ({"SA_WAVE_GRID": "1"}, 3, 2, dict(wg_per_cu=1, front_counter=1, dege_list=1)),
    ({"SA_FRONT_STATIC": "1"}, 3, 2, dict(wg_per_cu=8, front_counter=0, prep="row16", emit="row16")),
    ({"SA_FRONT_STATIC": "1", "SA_WAVE_GRID": "1"}, 3, 2, dict(wg_per_cu=1, front_counter=0, prep="row16", emit="row16")),
    ({"SA_SEQ_BUCKET": "0"}, 0, 2, dict(seq_packed=1, seq_replay="full", seq_digits=0x77)),
    ({}, 0, 2, dict(seq_replay="bucket", bkt_db=8, bkt_sb=6)),
    ({}, 2, 2, dict(seq_replay="bucket", bkt_db=8, bkt_sb=10)),
    ({}, 7, 2, dict(seq_packed=1, seq_replay="full", seq_digits=0x7777)),
    ({"SA_AUX_DENSE": "0"}, 3, 2, RAW17),
    ({"SA_AUX_DENSE": "0"}, 3, 3, RAW21),
    ({}, 3, 3, RAW21),                                                           # (21 model bits: never dense)
    ({"SA_MD5_PIPE": "1"}, 3, 2, dict(md5="pipe")),
    ({"SA_HOST_WAITS": "0"}, 3, 2, dict(host_waits=0)),
]
FRONT_ENVS = [{}, {"SA_PREP_FUSED": "1"}, {"SA_PREP_WAVE": "1"}, {"SA_PREP_ROW": "64"}, {"SA_EMIT_WAVE": "1"},
              {"SA_EMIT_WAVE": "1", "SA_PREP_WAVE": "1"}, {"SA_FRONT_STATIC": "1"}, {"SA_SEQ_PACK": "0"},
              {"SA_SEQ_BUCKET": "0"}, {"SA_RV_VARIANT": "0"}, {"SA_RV_VARIANT": "5"}, {"SA_RV_VARIANT": "6"}]


def _check_path_plan(exe):
    tables = {}

    def table(env):
        key = tuple(sorted(env.items()))
        if key not in tables:
            rows = _rows(exe, "--path-plan", env)
            assert len(rows) == 10 * 2 * 2
            tables[key] = {(p["slevel"], p["qlevel"], p["len"]): p for p in rows}
            assert len(tables[key]) == len(rows)
        return tables[key]

    for env, slevel, qlevel, expect in PATH_CASES:
        p = table(env)[(slevel, qlevel, 150)]
        want = {f: NAMED[f][v] if f in NAMED else v for f, v in expect.items()}
        assert {f: p[f] for f in want} == want, (env, slevel, qlevel)
    for env in FRONT_ENVS:
        packing = env.get("SA_SEQ_PACK") != "0"
        bucket = env.get("SA_SEQ_BUCKET") != "0"
        for (slevel, qlevel, length), p in table(env).items():
            at = (env, slevel, qlevel, length)
            bits = (2 * (slevel + 7)) & 31
            assert p["seq_bits"] == bits and p["aux_bits"] == (21 if qlevel > 2 else 17), at
            # packed keys exactly for contexts of 1..28 bits, when packing is on
            assert (p["seq_sh"] == 2) == (1 <= bits <= 28 and packing), at
            assert p["seq_sh"] in (0, 2) and p["seq_packed"] == p["seq_sh"] // 2, at
            # the bucket replay only over packed keys of 12..22 context bits
            assert p["seq_bkt"] == (1 if bucket and p["seq_sh"] == 2 and 12 <= bits <= 22 else 0), at
            assert p["seq_replay"] == (SEQ_REPLAY["bucket"] if p["seq_bkt"] else SEQ_REPLAY["full"]), at
            if p["seq_bkt"]:
                db = 8 if bits <= 20 else 9
                assert (p["bkt_db"], p["bkt_sb"], p["seq_lo"], p["seq_hi"]) == (db, bits - db, 2, 2 + db), at
                assert p["seq_digits"] == db and p["seq_inv"] == p["bkt_inv"] == 1, at
            else:
                assert (p["seq_lo"], p["seq_hi"]) == (p["seq_sh"], p["seq_sh"] + bits if bits else 0), at
                assert p["bkt_db"] == p["bkt_sb"] == p["bkt_inv"] == 0 and p["seq_max_db"] == 9, at
                # the fewest passes of at most 9 bits, each of at least 7
                dg = [(p["seq_digits"] >> (4 * i)) & 15 for i in range(8) if (p["seq_digits"] >> (4 * i)) & 15]
                assert len(dg) == -(-bits // 9) and all(7 <= d <= 9 for d in dg) and sum(dg) >= bits, at
            # pass R: the override, else 0 for a mean read length above 1000, else 6
            rv = env.get("SA_RV_VARIANT")
            assert p["rv_batch"] == (int(rv) if rv else (0 if length > 1000 else 6)), at
            # reads a take: 64 of 150 bases, a wave's four rows of 2,000; the listed reads from a counter below 64
            assert p["wqc"] == (64 if length == 150 else 4), at
            assert p["dege_counter"] == (1 if p["wqc"] < 64 and "SA_FRONT_STATIC" not in env else 0), at
            # the dense sort for 17 model bits; its buffer sizes carry the 128 elements of slack
            assert p["dense"] == (1 if qlevel == 2 else 0) and p["aux_passes"] == (1 if qlevel == 2 else 3), at
            nreads = 16000 if length == 150 else 400
            seq_total, aux_total = nreads * length, nreads * (length + 40)
            assert (p["stot"], p["atot"]) == (seq_total + 128, aux_total + 128), at
            assert p["max_long"] == aux_total // 512 + 1 and p["max_seq_long"] == seq_total // 243 + 1, at
            assert p["max_short"] == min(aux_total, 3 << p["aux_bits"]), at


def test_path_plan(emu):
    """plan_paths / plan_totals / report_paths for Slevel 0..9 x Qlevel {2, 3} x
    a batch of 150-base and one of 2,000-base reads under each front knob:
    the report equals what tests/test_gpu_paths.py expects of the device for
    the same knobs and levels (values copied from it), keys are packed exactly
    for contexts of 1..28 bits with packing on, the bucket replay runs only
    over packed keys of 12..22 bits, and pass R's variant is 0 for the long
    reads and 6 for the short ones unless SA_RV_VARIANT says otherwise."""
    _check_path_plan(emu)


def test_knobs_and_path_plan_under_sanitizers(emu_san):
    """Both sweeps once more through the stand-alone program built with
    -fsanitize=address,undefined (sa_knobs.h and sa_plan.h compiled in it): the
    same values, and nothing reported (stderr must be empty)."""
    _check_knobs(emu_san)
    _check_path_plan(emu_san)
