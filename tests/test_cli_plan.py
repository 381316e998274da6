"""The command line's knob table (parse_cli_knobs, cli_knobs.h) and batch plan
(plan_batches, cli_plan.h) checked without a GPU through the stand-alone
tests/cpu_emu/cli_emu.cpp, once built with -O2 and once with
-fsanitize=address,undefined; and the two options of -c that run without a
device but had no test, --ramp and --release (under --host-only).

The expected values restate what compress(), SegReader::start, OutPool and main
computed in place before the table and the plan existed (commit 7d78f3a,
seqarc_cli.cpp): _parent_plan below follows that code line by line, and the
named cases carry their numbers written out."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, TEST1, TEST2

from fastqueeze_amd import build

EXE = build.CLI
U64 = 1 << 64
MIB = 1 << 20


def _build_emu(exe, flags):
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpu_emu", "cli_emu.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build_emu(tmp_path_factory.mktemp("cli_emu") / "cli_emu", ["-O2"])


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return _build_emu(tmp_path_factory.mktemp("cli_emu_san") / "cli_emu_san",
                      ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _rows(exe, args, env):
    """cli_emu's `name value ...` lines under exactly `env`, as dicts of ints"""
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=dict(env))
    assert r.returncode == 0 and r.stderr == "", (args, env, r.stderr[-2000:])
    return [dict(zip(w[0::2], map(int, w[1::2]))) for w in (l.split() for l in r.stdout.splitlines())]


# ---- the knob table ----------------------------------------------------------------------------

def _queues(per):   # GPU_MAX_HW_QUEUES for 1, 2, 5 and 8 contexts a device (main: min(32, per * contexts + 4))
    return {f"queues_c{c}": min(32, per * c + 4) for c in (1, 2, 5, 8)}


KNOB_DEFAULTS = dict(windows=0, seg_mib=256, seg_slices=0, ring_segs=0, ahead_batches=1, free_threads=8, ring_free=1,
                     early_read=1, prefill_windows_set=0, prefill_windows=0, stream=0, prefetch=1, out_exact=1,
                     out_pool=1, hwq=0, test_out=0, exit_probe=0, **_queues(4))


def _vals(zero, one, below, above, text):
    return {"0": zero, "1": one, "-5": below, "99": above, "x": text}


def _off_if_zero(field):         # on unless set and atoi gives 0 (text reads as 0)
    return {v: {field: x} for v, x in _vals(0, 1, 1, 1, 0).items()}


def _on_if_nonzero(field):       # set and atoi not 0
    return {v: {field: x} for v, x in _vals(0, 1, 1, 1, 0).items()}


def _at_least(field, floor):     # max(floor, atoi)
    return {v: {field: x} for v, x in _vals(floor, max(floor, 1), floor, 99, floor).items()}


# knob -> {value: the fields that differ from the defaults}; "-5" is below every range, "99" above the
# small ones, "x" is no number.  From the reads as they stood: SegReader::start (SEG_MIB, SEG_SLICES,
# RING_SEGS), SegReader::free_all (FREE_THREADS), OutPool::on, compress() and main (HWQ, STREAM).
KNOBS = {
    "SA_CLI_WINDOWS": {v: {"windows": 1} for v in _vals(0, 0, 0, 0, 0)},          # set at all, "0" included
    "SA_CLI_SEG_MIB": _at_least("seg_mib", 4),
    "SA_CLI_SEG_SLICES": {v: {"seg_slices": x} for v, x in _vals(1, 1, U64 - 5, 99, 1).items()},   # (strtoull)
    "SA_CLI_RING_SEGS": _at_least("ring_segs", 3),
    "SA_CLI_AHEAD_BATCHES": _at_least("ahead_batches", 1),
    "SA_CLI_FREE_THREADS": _at_least("free_threads", 1),
    "SA_CLI_RING_FREE": _off_if_zero("ring_free"),
    "SA_CLI_EARLY_READ": _off_if_zero("early_read"),
    "SA_CLI_PREFILL_WINDOWS": {v: {"prefill_windows_set": 1, "prefill_windows": x}
                               for v, x in _vals(0, 1, U64 - 5, 99, 0).items()},
    # (main: five queues a context with the streamed staging's copy stream)
    "SA_CLI_STREAM": {v: dict({"stream": x}, **_queues(5 if x else 4)) for v, x in _vals(0, 1, 1, 1, 0).items()},
    "SA_CLI_PREFETCH": _off_if_zero("prefetch"),
    "SA_CLI_OUT_EXACT": _off_if_zero("out_exact"),
    "SA_CLI_OUT_POOL": _off_if_zero("out_pool"),
    "SA_CLI_HWQ": {v: dict({"hwq": x}, **_queues(x)) for v, x in _vals(1, 1, 1, 99, 1).items()},
    "SA_CLI_TEST_OUT": {v: {"test_out": x} for v, x in _vals(0, 1, U64 - 5, 99, 0).items()},
    "SA_CLI_EXIT_PROBE": _on_if_nonzero("exit_probe"),
}


def _check_knobs(exe):
    assert _rows(exe, ["--knobs"], {}) == [KNOB_DEFAULTS]
    fields = {f for cases in KNOBS.values() for d in cases.values() for f in d if not f.startswith("queues")}
    assert fields == {f for f in KNOB_DEFAULTS if not f.startswith("queues")}      # every field has its knob
    for knob, cases in KNOBS.items():
        assert {"0", "1", "-5", "99", "x"} <= set(cases)
        for value, diff in cases.items():
            assert _rows(exe, ["--knobs"], {knob: value}) == [dict(KNOB_DEFAULTS, **diff)], (knob, value)
    # SA_CLI_HWQ wins over SA_CLI_STREAM's five
    both = _rows(exe, ["--knobs"], {"SA_CLI_STREAM": "1", "SA_CLI_HWQ": "2"})[0]
    assert {k: both[k] for k in _queues(2)} == _queues(2)


def test_cli_knobs_only_in_the_table():
    """Every SA_CLI_* variable the command line reads is read by parse_cli_knobs:
    seqarc_cli.cpp has no getenv of one, and the table's names are the ones the
    sweep covers."""
    csrc = os.path.join(ROOT, "fastqueeze_amd", "csrc")
    with open(os.path.join(csrc, "seqarc_cli.cpp")) as f:
        assert 'getenv("SA_CLI_' not in f.read()
    with open(os.path.join(csrc, "cli_knobs.h")) as f:
        names = set(re.findall(r'\("(SA_CLI_[A-Z_]+)"\)', f.read()))
    assert names == set(KNOBS)


def test_cli_knob_table(emu):
    """parse_cli_knobs on each SA_CLI_* knob alone, unset and set to "0", "1", a
    value below its range, one above and one that is no number: the field (and
    the hardware queue count main derives) has the value the read it replaces
    gave, every other field its default."""
    _check_knobs(emu)


# ---- the batch plan ----------------------------------------------------------------------------

OPTS = dict(batch=32, contexts=2, devices=1, threads=0, read_threads=16, host_only=0, host_parse=0, ingest_only=0,
            ramp=0, stage_ahead=0, pe=0, bs=50 * MIB, size0=U64 - 1, size1=U64 - 1, gz0=0, gz1=0, reg0=0, reg1=0,
            hw_threads=16)
UNKNOWN = U64 - 1


def _atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def _parent_plan(o, env, nctx=None):
    """compress()'s geometry at 7d78f3a (seqarc_cli.cpp :1998-2050, :2134-2171,
    :2212-2222, :2627) and SegReader::start's (:1083-1102), restated"""
    pe, bs = o["pe"], o["bs"]
    nin = 2 if pe else 1
    gz1, gz2 = bool(o["gz0"]), bool(pe and o["gz1"])
    reg = [bool(o[f"reg{i}"]) and o[f"size{i}"] != UNKNOWN for i in range(nin)]
    size = [o[f"size{i}"] for i in range(nin)]
    p = {}
    dev_parse = not o["host_parse"] and not o["host_only"]
    p["dev_parse"] = int(dev_parse)
    p["nparse"] = 1 if dev_parse else o["threads"] if o["threads"] > 0 else max(1, min(16, o["hw_threads"]))
    win = ((bs & 0xffffffff) >> 1) if pe else bs
    p["cut_window"], p["text_win"], p["tstride"] = win, win + (64 << 10), win + (128 << 10)
    p["texts_pinned"] = int(dev_parse and not o["ingest_only"])
    seg_plain = o["read_threads"] > 0 and not gz1 and not gz2 and "SA_CLI_WINDOWS" not in env and all(reg)
    p["seg_plain"] = int(seg_plain)
    p["early_read"] = int(seg_plain and not ("SA_CLI_EARLY_READ" in env and _atoi(env["SA_CLI_EARLY_READ"]) == 0))
    p["prefill_windows"] = p["prefill_chunks"] = 0
    if p["texts_pinned"] and not seg_plain:
        wins = nin * (2 * max(1, o["batch"]) + 4)
        if all(reg) and not gz1 and not gz2:
            wins = min(wins, nin * (max(size) // win + 3))
        if "SA_CLI_PREFILL_WINDOWS" in env:
            wins = int(env["SA_CLI_PREFILL_WINDOWS"])
        p["prefill_windows"], p["prefill_chunks"] = wins, (wins + 15) // 16
    asked = o["contexts"] * (1 if o["host_only"] else o["devices"])
    p["asked"] = asked
    B, C, ramp = max(1, o["batch"]), asked if nctx is None else nctx, bool(o["ramp"])
    if not o["host_only"] and not o["ingest_only"] and not gz1 and not gz2 and all(reg):
        est = (sum(size) + bs - 1) // bs + 1
        if est <= C * B:
            ramp, B = False, (est + C - 1) // C
    stream = "SA_CLI_STREAM" in env and _atoi(env["SA_CLI_STREAM"]) != 0
    p["stream_opt"] = int(dev_parse and not o["ingest_only"] and not o["stage_ahead"] and stream)
    p["B"], p["C"], p["ramp"] = B, C, int(ramp)
    p["max_inflight"] = B * (C * (2 if p["stream_opt"] else 1) + 2)
    rs = [0]
    for k in range(C if ramp else 0):
        rs.append(rs[-1] + max(1, B * (k + 1) // (C + 1)))
    p["ramp_n"] = len(rs)
    p.update({f"rs{i}": v for i, v in enumerate(rs)})
    r = len(rs) - 1
    p.update({f"bstart{k}": rs[k] if k <= r else rs[-1] + (k - r) * B for k in range(C + 5)})
    p.update(seg_ahead=0, seg_window=0, seg_ahead_bytes=0, seg_bytes=0, ring_segs=0)
    if seg_plain:
        ahead = max(1, _atoi(env["SA_CLI_AHEAD_BATCHES"])) if "SA_CLI_AHEAD_BATCHES" in env else 1
        window, ahead_bytes, slice_ = win + (64 << 10), (ahead * B + 2) * win, 4 * MIB
        smax = (max(4, _atoi(env["SA_CLI_SEG_MIB"])) if "SA_CLI_SEG_MIB" in env else 256) * MIB
        S = max(slice_, min(smax, (max(size) + slice_ - 1) // slice_ * slice_))
        if "SA_CLI_SEG_SLICES" in env:
            S = slice_ * max(1, int(env["SA_CLI_SEG_SLICES"]))
        R = max(3, (ahead_bytes + S - 1) // S + 3)
        if "SA_CLI_RING_SEGS" in env:
            R = max(3, _atoi(env["SA_CLI_RING_SEGS"]))
        R = max(R, (B * window + S - 1) // S + 2)
        p.update(seg_ahead=ahead, seg_window=window, seg_ahead_bytes=ahead_bytes, seg_bytes=S, ring_segs=R)
    return p


def _plans(exe, cases, env):
    """cli_emu --plan for every case (dicts over OPTS, 'nctx' optional) in one run"""
    args = ["--plan"]
    for i, c in enumerate(cases):
        args += (["--"] if i else []) + [f"{k}={v}" for k, v in c.items()]
    rows = _rows(exe, args, env)
    assert len(rows) == len(cases)
    return rows


def _inputs(kind, pe, bs, slots):
    """inputs by kind; slots = C * B.  fits: the largest plain input with est <= C * B
    (est = ceil(bytes / bs) + 1); over: one block more"""
    n = 2 if pe else 1
    d = {}
    for i in range(n):
        if kind == "pipe":
            d.update({f"reg{i}": 0})
        elif kind == "gz":
            d.update({f"reg{i}": 1, f"gz{i}": 1, f"size{i}": 3 * bs})
        else:
            blocks = max(1, slots - 1) + (1 if kind == "over" else 0)      # of the two inputs together
            total = blocks * bs - (0 if kind == "over" else 7)             # fits: inside the last block
            d.update({f"reg{i}": 1, f"size{i}": total // n + (total % n if i == 0 else 0)})
    return d


FLAGS = [{}, {"read_threads": 0}, {"host_only": 1}, {"ingest_only": 1}, {"host_parse": 1, "threads": 3},
         {"host_parse": 1, "hw_threads": 64}, {"ramp": 1}, {"stage_ahead": 1, "ramp": 1}]
PLAN_ENVS = [{}, {"SA_CLI_STREAM": "1"}, {"SA_CLI_AHEAD_BATCHES": "3"}, {"SA_CLI_PREFILL_WINDOWS": "40"},
             {"SA_CLI_WINDOWS": "0"}, {"SA_CLI_EARLY_READ": "0"}, {"SA_CLI_SEG_SLICES": "1", "SA_CLI_RING_SEGS": "3"},
             {"SA_CLI_SEG_MIB": "64"}]


def _sweep_cases():
    cases = []
    for pe in (0, 1):
        for batch in (1, 2, 69):
            for contexts in (1, 3, 5):
                for devices in (1, 8):
                    for kind in ("fits", "over", "pipe", "gz"):
                        for bs in (MIB, 50 * MIB):
                            for flags in FLAGS:
                                o = dict(OPTS, pe=pe, batch=batch, contexts=contexts, devices=devices, bs=bs, **flags)
                                asked = contexts * (1 if o["host_only"] else devices)
                                o.update(_inputs(kind, pe, bs, asked * batch))
                                cases.append(o)
    return cases


def _check_plan(exe, envs):
    cases = _sweep_cases()
    for env in envs:
        for o, got in zip(cases, _plans(exe, cases, env)):
            assert got == _parent_plan(o, env), (env, o)
    # fewer contexts created than asked for: the plan for the created count
    some = [dict(o, nctx=max(1, o["contexts"] * o["devices"] - 1)) for o in cases[::17]]
    for o, got in zip(some, _plans(exe, some, {})):
        want = _parent_plan({k: v for k, v in o.items() if k != "nctx"}, {}, o["nctx"])
        assert got == want and got["C"] == o["nctx"], o


def _named(exe, env=None, **kw):
    o = dict(OPTS, **kw)
    got = _plans(exe, [o], env or {})[0]
    assert got == _parent_plan({k: v for k, v in o.items() if k != "nctx"}, env or {}, o.get("nctx")), o
    return got


def _check_named_plans(exe):
    plain = dict(reg0=1, reg1=1)
    # one round: 2 x 10 MiB at 1 MiB blocks is est = 21 blocks <= C * B = 3 * 8: the ramp off, B = ceil(21 / 3)
    p = _named(exe, pe=1, bs=MIB, batch=8, contexts=3, ramp=1, size0=10 * MIB, size1=10 * MIB, **plain)
    assert (p["ramp"], p["B"], p["C"], p["ramp_n"], p["max_inflight"]) == (0, 7, 3, 1, 7 * 5)
    assert [p[f"bstart{k}"] for k in range(5)] == [0, 7, 14, 21, 28]
    assert (p["seg_plain"], p["early_read"], p["prefill_chunks"]) == (1, 1, 0)
    assert (p["cut_window"], p["text_win"], p["tstride"]) == (MIB // 2, MIB // 2 + 65536, MIB // 2 + 131072)
    assert (p["seg_bytes"], p["seg_ahead_bytes"], p["ring_segs"]) == (12 * MIB, 9 * MIB // 2, 4)
    # one block too big for the round (est = 25 > 24): B and the ramp stay
    p = _named(exe, pe=1, bs=MIB, batch=8, contexts=3, ramp=1, size0=12 * MIB, size1=12 * MIB, **plain)
    assert (p["ramp"], p["B"], p["ramp_n"]) == (1, 8, 4)
    assert [p[f"rs{k}"] for k in range(4)] == [0, 2, 6, 12]                      # 8 (k + 1) / 4
    # a pipe (size unknown): no one-round rule, the window reader, the prefill by the batch
    p = _named(exe, pe=1, bs=MIB, batch=8, contexts=3, ramp=1, reg0=0, reg1=0)
    assert (p["ramp"], p["B"], p["seg_plain"], p["early_read"]) == (1, 8, 0, 0)
    assert (p["prefill_windows"], p["prefill_chunks"]) == (2 * (2 * 8 + 4), 3)
    # gzip: the same, whatever its size
    p = _named(exe, bs=MIB, batch=8, contexts=3, ramp=1, reg0=1, gz0=1, size0=MIB)
    assert (p["ramp"], p["B"], p["seg_plain"], p["prefill_windows"], p["prefill_chunks"]) == (1, 8, 0, 20, 2)
    # --read-threads 0: the window reader over a plain file, the prefill by its size (10 windows + 3)
    p = _named(exe, bs=MIB, batch=8, contexts=3, read_threads=0, reg0=1, size0=10 * MIB)
    assert (p["seg_plain"], p["early_read"], p["prefill_windows"], p["prefill_chunks"], p["B"]) == (0, 0, 13, 1, 4)
    # --host-only / --ingest-only: the one-round rule does not apply; host-only has no devices
    p = _named(exe, bs=MIB, batch=8, contexts=3, devices=8, host_only=1, ramp=1, reg0=1, size0=10 * MIB)
    assert (p["ramp"], p["B"], p["C"], p["dev_parse"], p["nparse"], p["texts_pinned"]) == (1, 8, 3, 0, 16, 0)
    p = _named(exe, bs=MIB, batch=8, contexts=3, devices=8, ingest_only=1, ramp=1, reg0=1, size0=10 * MIB)
    assert (p["ramp"], p["B"], p["C"], p["dev_parse"], p["nparse"], p["texts_pinned"]) == (1, 8, 24, 1, 1, 0)
    # --ramp with C = 5, B = 69 (the input far larger than a round): 69 (k + 1) / 6, entry by entry
    p = _named(exe, pe=1, batch=69, contexts=5, ramp=1, size0=20000 * MIB, size1=20000 * MIB, **plain)
    assert (p["ramp"], p["B"], p["C"], p["ramp_n"]) == (1, 69, 5, 6)
    assert [p[f"rs{k}"] for k in range(6)] == [0, 11, 34, 68, 114, 171]
    bstart = [p[f"bstart{k}"] for k in range(5 + 5)]
    assert bstart[:6] == [0, 11, 34, 68, 114, 171] and all(b > a for a, b in zip(bstart, bstart[1:]))
    assert all(bstart[5 + n] - bstart[5 + n - 1] == 69 for n in range(1, 5))
    assert (p["max_inflight"], p["ring_segs"]) == (69 * 7, 10)     # (71 x 25 MiB ahead / 256 MiB + 3)
    # SA_CLI_STREAM=1 doubles the contexts' share of the in-flight bound (not under --stage-ahead)
    big = dict(pe=1, batch=69, contexts=5, size0=20000 * MIB, size1=20000 * MIB, **plain)
    assert _named(exe, {"SA_CLI_STREAM": "1"}, **big)["max_inflight"] == 69 * 12
    assert _named(exe, {"SA_CLI_STREAM": "0"}, **big)["max_inflight"] == 69 * 7
    assert _named(exe, {"SA_CLI_STREAM": "1"}, stage_ahead=1, **big)["max_inflight"] == 69 * 7
    # SA_CLI_AHEAD_BATCHES: the segment reader's bytes ahead; SA_CLI_PREFILL_WINDOWS: the windows as given
    p = _named(exe, {"SA_CLI_AHEAD_BATCHES": "2"}, **big)
    assert (p["seg_ahead"], p["seg_ahead_bytes"], p["ring_segs"]) == (2, 140 * 25 * MIB, 17)
    p = _named(exe, {"SA_CLI_PREFILL_WINDOWS": "40"}, pe=1, bs=MIB, batch=8, contexts=3, reg0=0, reg1=0)
    assert (p["prefill_windows"], p["prefill_chunks"]) == (40, 3)
    p = _named(exe, {"SA_CLI_PREFILL_WINDOWS": "0"}, pe=1, bs=MIB, batch=8, contexts=3, reg0=0, reg1=0)
    assert (p["prefill_windows"], p["prefill_chunks"]) == (0, 0)
    # fewer contexts created than asked for: the second plan, with the created count
    p = _named(exe, nctx=3, **big)
    assert (p["asked"], p["C"], p["max_inflight"]) == (5, 3, 69 * 5)


def test_cli_plan_sweep(emu):
    """plan_batches over PE and SE x --batch {1, 2, 69} x --contexts {1, 3, 5} x
    --devices {1, 8} x an input that just fits one round, one a block larger, a
    pipe and gzip x 1 and 50 MiB blocks x --read-threads 0, --host-only,
    --ingest-only, --host-parse, --ramp and --stage-ahead, under each knob that
    enters the geometry: every field equals the arithmetic compress() and
    SegReader::start did in place."""
    _check_plan(emu, PLAN_ENVS)


def test_cli_plan_named_cases(emu):
    """The cases with their numbers written out: the one-round rule on either
    side of its threshold, a pipe, gzip, --read-threads 0, --host-only and
    --ingest-only, the ramp's batch starts for C = 5 and B = 69, SA_CLI_STREAM's
    in-flight bound, the SA_CLI_AHEAD_BATCHES and SA_CLI_PREFILL_WINDOWS
    overrides, and a second plan with fewer contexts than asked for."""
    _check_named_plans(emu)


def test_cli_knobs_and_plan_under_sanitizers(emu_san):
    """The knob sweep, the named plans and the plan sweep (default knobs and
    SA_CLI_STREAM) once more through the program built with
    -fsanitize=address,undefined: the same values, nothing reported."""
    _check_knobs(emu_san)
    _check_named_plans(emu_san)
    _check_plan(emu_san, PLAN_ENVS[:2])


# ---- --ramp and --release, without a device ----------------------------------------------------

def _host_only(tmp_path, name, extra):
    r = subprocess.run([EXE, "-c", "-v", "-f", "--host-only", "--block-size", "1", "--contexts", "2", "--batch", "2",
                        "-t", "2", "-1", TEST1, "-2", TEST2, "-o", str(tmp_path / name)] + extra,
                       capture_output=True, text=True, cwd=tmp_path, timeout=120,
                       env=dict(os.environ, SA_CLI_TEST_OUT="50000"))
    assert r.returncode == 0, (name, r.stderr)
    return (tmp_path / (name + ".arc")).read_bytes(), r.stderr


def test_host_only_ramp_and_release(tmp_path, emu):
    """--ramp and --release under --host-only (SA_CLI_TEST_OUT filler, no device),
    the test pair at 1 MiB blocks, two contexts, two-block batches: the archive
    is byte for byte the one without the option and the run ends with status 0;
    --release reports its contexts released, the others leave them to the exit.
    The host path prints no per-batch line, so that the ramp deals first batches
    smaller than B is read off the plan for these very options (one block each,
    then two) -- tests/test_gpu_parity.py reads the same off the device path's
    -v lines."""
    plain, err = _host_only(tmp_path, "plain", [])
    assert "contexts left to the exit" in err
    nblocks = int(re.search(r"seqarc_amd: (\d+) block\(s\)", err).group(1))
    assert nblocks > 3 and plain[16:16 + 50000 * nblocks] == b"\x5a" * (50000 * nblocks)
    ramp, err = _host_only(tmp_path, "ramp", ["--ramp"])
    assert ramp == plain and "contexts left to the exit" in err
    rel, err = _host_only(tmp_path, "rel", ["--release"])
    assert rel == plain and "contexts released" in err and "monotonic clock: main" in err
    both, err = _host_only(tmp_path, "both", ["--ramp", "--release"])
    assert both == plain
    p = _named(emu, pe=1, bs=MIB, batch=2, contexts=2, host_only=1, ramp=1, threads=2, reg0=1, reg1=1,
               size0=os.path.getsize(TEST1), size1=os.path.getsize(TEST2))
    assert (p["ramp"], p["B"], p["C"]) == (1, 2, 2)
    assert [p[f"bstart{k}"] for k in range(5)] == [0, 1, 2, 4, 6]       # batches of 1, 1, 2, 2 blocks
