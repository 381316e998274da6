"""Every kernel path an SA_* knob, a batch shape or the context's own state
selects, against the oracle byte for byte, with the path asserted.

Which kernels a batch runs is decided on the host from the environment (read
when a context is created) and from state a context carries between batches
(the dense AUX sort turns itself off for the context's lifetime).  Each case
here sets its knobs, creates a fresh Encoder, encodes small inputs that still
cross what matters (16- and 64-lane row steps, 4096-key sort tiles, several
blocks of unequal size per batch, the 512 / 65,536 run-length classes,
BASE_MODEL runs past in-run index 242), compares every block with
oracle_py.encode_block, and asserts from Encoder.paths() (sa_last_paths) that
the kernels it meant to run did run: a knob that silently stops selecting its
kernel fails its case."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py
import synth

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_RUN, HUGE_RUN = 512, 65536          # sa_device.h: the AUX replay's run-length classes
RV_LONG_SYMS = 1 << 21                   # sa_engine.hip: a pass-R chain of this many symbols gets a wave


# ---- inputs (made once, never changed) -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _input(name):
    if name in ("S", "S1"):     # 16,000 PE reads: ~10 blocks of unequal size, or one
        a, b = synth.generate(8000, paired=True)
        return fq.blocks_from_fastq(a, b, 600_000) if name == "S" else fq.blocks_from_fastq(a, b)
    if name == "M":             # lengths 0, 1, 2, 16, 17, 63, 64, 65 .. 1000, N / IUPAC, '#' runs, > 512 models
        return fq.blocks_from_fastq(synth.long_read_fastq(5, 510))
    if name == "N":             # the prefix / suffix name set
        return fq.blocks_from_fastq(synth.prefix_suffix_names_fastq(), None, 100_000)
    if name == "LC":            # low-complexity reads: context runs past the first halving
        return fq.blocks_from_fastq(synth.low_complexity_fastq(33, 4000), None, 200_000)
    if name == "Q":             # long reads for -l: noisy qualities, and runs that cross many R-Block chunks
        t1, _ = synth.generate(40, paired=False, seed=12, read_len=20000)
        return (fq.blocks_from_fastq(t1, None, 2 << 20) +
                fq.blocks_from_fastq(synth.rblock_runs_fastq(31, 40, 30000), None, 2 << 20))
    if name == "E":
        return fq.blocks_from_fastq(synth.edge_cases())
    if name == "ONE":           # one block of one read
        return [fq.parse_se(b"@SIMRD1\nACGTNACGT\n+\nFFFF#FF,:\n")]
    if name == "B512":
        return fq.blocks_from_fastq(synth.model_boundary_fastq(synth.MODELS_512_READS))
    if name == "B513":
        return fq.blocks_from_fastq(synth.model_boundary_fastq(synth.MODELS_513_READS))
    raise KeyError(name)


def _cfg(kw):
    return fq.Config(**kw)


@functools.lru_cache(maxsize=None)
def _want(name, cfg_items):
    cfg = _cfg(dict(cfg_items))
    return [oracle_py.encode_block(b, cfg.slevel, cfg.qlevel, cfg.md5, cfg.bin_mode, cfg.lossy) for b in _input(name)]


def _mismatch(got, want):
    """None, or where the first differing block differs."""
    if len(got) != len(want):
        return f"{len(got)} blocks vs the oracle's {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), min(len(g), len(w)))
            return f"block {i}: gpu {len(g)} B vs oracle {len(w)} B, first difference at byte {at}"
    return None


def _path_diff(paths, expect):
    return {k: (paths[k], v) for k, v in expect.items() if paths[k] != v}


def _step(enc, name, cfg_kw, expect):
    """One batch: bytes equal to the oracle, then the reported path."""
    got = enc.encode(_input(name), _cfg(cfg_kw))
    bad = _mismatch(got, _want(name, tuple(sorted(cfg_kw.items()))))
    assert bad is None, f"{name} {cfg_kw}: {bad}"
    diff = _path_diff(enc.paths(), expect)
    assert not diff, f"{name} {cfg_kw}: path (got, expected) {diff}"


def _run(monkeypatch, env, steps):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = fq.Encoder(0)
    try:
        for name, cfg_kw, expect in steps:
            _step(e, name, cfg_kw, expect)
    finally:
        e.close()


# what a fresh context reports for short PE reads at the default config
DEFAULT = dict(prep="row16", front_counter=1, wg_per_cu=8, emit="row16", seq_packed=1, seq_replay="bucket",
               bkt_inv=1, bkt_lpt=1, bkt_db=8, bkt_sb=12, pass_r="rv6", r_waves=4, l_chunk=32, l_stream=0,
               host_waits=1, chain_prio=1, md5="plain", rblock=0, exact_rerun=0, front_masked=0)
DENSE1 = dict(aux_sort="dense1", aux_runs="runs_dense", aux_digits=0x9)
RAW17 = dict(aux_sort="raw", aux_runs="find_runs", aux_digits=0x89)      # 17 model bits: 9 + 8
RAW21 = dict(aux_sort="raw", aux_runs="find_runs", aux_digits=0x777)     # 21 model bits (Qlevel 3)


def test_inputs_cross_what_they_are_meant_to():
    """The shapes the cases rely on, from the inputs themselves (no GPU work):
    S has several blocks of unequal size and more reads than three rounds of a
    one-workgroup-per-CU grid (3 x 4096 rows); S1 is one block whose hottest
    quality context (the oracle's formula, Qlevel 2) holds at least HUGE_RUN
    symbols; M has every length around the 16- and 64-lane steps and more than
    512 quality models; the blocks span several 4096-key sort tiles."""
    S, S1, M = _input("S"), _input("S1"), _input("M")
    assert len(S) >= 8 and len({b.nreads for b in S}) > 1
    assert sum(b.nreads for b in S) == 16000 > 3 * 4096
    assert len(S1) == 1 and S1[0].nreads == 16000 and S1[0].seq.size > 16 * 4096

    def qual_models(b):
        """{quality-context model: symbols coded in it} of a block at Qlevel 2
        (encode_qual: trailing '#' dropped and marked by one symbol 94; the
        context after a symbol from the last two symbols and the summed drops)"""
        lens = b.seq_lens.astype(np.int64)
        nr, L = len(lens), int(lens.max())
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
        idx = np.arange(L)[None, :]
        valid = idx < lens[:, None]
        sym = np.zeros((nr, L + 1), np.int64)
        sym[:, :L][valid] = b.qual[(off[:, None] + idx)[valid]].astype(np.int64) - 33
        nonhash = valid & (sym[:, :L] != ord("#") - 33)
        n = np.where(nonhash.any(1), L - np.argmax(nonhash[:, ::-1], axis=1), 0)
        rows = np.arange(nr)
        sym[rows, n] = np.where(n != lens, 94, sym[rows, n])
        nsym = n + (n != lens)
        q1 = np.zeros(nr, np.int64)
        q2, last, delta = q1.copy(), q1.copy(), q1 + 5
        models = []
        for i in range(L + 1):
            act = i < nsym
            if not act.any():
                break
            models.append(last[act])
            s = sym[:, i]
            ctx = ((np.maximum(q1, q2) << 6) + s) & 0xfff
            ctx += np.where(q1 == q2, 0x1000, 0)
            delta = delta + np.where(q1 > s, q1 - s, 0)
            ctx += (np.minimum(delta, 56) & 0xf8) << 10
            q2, q1, last = q1, s, ctx
        ids, cnt = np.unique(np.concatenate(models), return_counts=True)
        return dict(zip(ids.tolist(), cnt.tolist()))

    hot = qual_models(S1[0])
    assert max(hot.values()) >= HUGE_RUN
    assert len(hot) <= 512                      # (with the other streams' models: the report, below)
    assert max(qual_models(S[0]).values()) > LONG_RUN
    assert len(M) == 1 and {0, 1, 2, 16, 17, 63, 64, 65, 1000} <= set(M[0].seq_lens.tolist())
    assert len(qual_models(M[0])) > 512


# ---- the path matrix ------------------------------------------------------------------------

def _both(names, cfgs, expect):
    return [(n, c, expect) for c in cfgs for n in names]


S33, S12 = dict(slevel=3, qlevel=3), dict(slevel=1, qlevel=2)

FRONT = [
    pytest.param({"SA_PREP_FUSED": "1"}, [("N", dict(bin_mode=0), dict(prep="fused", front_counter=1))], id="prep_fused-N"),
    pytest.param({"SA_PREP_FUSED": "1"}, [("M", S33, dict(prep="fused"))], id="prep_fused-M"),
    # k_prep_sq leaves no maxq: the N / IUPAC symbols come from k_emit's serial path
    pytest.param({"SA_PREP_WAVE": "1"}, _both(["M", "S"], [{}], dict(prep="wave", emit="row16", dege_list=0)),
                 id="prep_wave"),
    pytest.param({"SA_EMIT_WAVE": "1"}, _both(["M", "S"], [S33, S12], dict(prep="row16", emit="wave", dege_list=0)),
                 id="emit_wave"),
    pytest.param({"SA_EMIT_WAVE": "1", "SA_PREP_WAVE": "1"},
                 _both(["M", "S"], [S33, S12], dict(prep="wave", emit="wave", dege_list=0, front_counter=0)),
                 id="emit_wave+prep_wave"),
    pytest.param({"SA_SEQ_PACK": "0"}, _both(["S", "LC"], [dict(slevel=3)], dict(seq_packed=0, seq_replay="full",
                                                                                  seq_digits=0x777)), id="seq_unpacked-s3"),
    pytest.param({"SA_SEQ_PACK": "0"}, [("S", dict(slevel=8), dict(seq_packed=0, seq_replay="full", seq_digits=0x7788))],
                 id="seq_unpacked-s8"),
    # one workgroup per CU: 4,096 rows in flight, so S's 16,000 reads take every grid-stride loop round three times
    pytest.param({"SA_WAVE_GRID": "1"}, _both(["S", "M"], [{}], dict(wg_per_cu=1, front_counter=1, dege_list=1)),
                 id="wave_grid1"),
    pytest.param({"SA_FRONT_STATIC": "1"}, _both(["S", "M"], [{}], dict(wg_per_cu=8, front_counter=0, prep="row16",
                                                                        emit="row16")), id="front_static"),
    pytest.param({"SA_FRONT_STATIC": "1", "SA_WAVE_GRID": "1"},
                 _both(["S", "M"], [{}], dict(wg_per_cu=1, front_counter=0, prep="row16", emit="row16")),
                 id="front_static+wave_grid1"),
]

AUX = [
    pytest.param({}, [("S", {}, dict(DEFAULT, dege_list=1, r_short_shared=1, aux_dense_next=1, **DENSE1)),
                      ("S1", {}, dict(DEFAULT, aux_dense_next=1, **DENSE1))], id="dense_one_pass"),
    pytest.param({"SA_FIND_RUNS": "1"}, [("S", {}, dict(aux_sort="dense1", aux_runs="find_runs")),
                                         ("S1", {}, dict(aux_sort="dense1", aux_runs="find_runs"))], id="find_runs"),
    pytest.param({"SA_AUX_DENSE": "0"}, _both(["S", "S1", "M"], [{}], dict(RAW17, aux_nmod_max=0)), id="raw-q2"),
    pytest.param({"SA_AUX_DENSE": "0"}, _both(["S", "M"], [dict(qlevel=3)], RAW21), id="raw-q3"),
    # more than 512 models in the block: two dense passes and the copy, and the context's flag goes off
    pytest.param({}, [("M", {}, dict(aux_sort="dense2+copy", aux_runs="find_runs", aux_digits=0x89, aux_dense_next=0))],
                 id="dense_two_passes"),
]

SEQ = [
    # 8 digit bits at 22 context bits would need 82,240 B of LDS a wave: plan_bkt falls back to 9
    pytest.param({"SA_BKT_DB": "8"}, [("S", dict(slevel=4), dict(seq_replay="bucket", bkt_db=9, bkt_sb=13))], id="bkt_db8-s4"),
    pytest.param({"SA_BKT_DB": "9"}, _both(["S", "LC"], [dict(slevel=0)], dict(seq_replay="bucket", bkt_db=9, bkt_sb=5)),
                 id="bkt_db9-s0"),
    pytest.param({"SA_BKT_DB": "10"}, _both(["S", "LC"], [dict(slevel=0)], dict(seq_replay="bucket", bkt_db=10, bkt_sb=4,
                                                                               bkt_inv=1)), id="bkt_db10-s0"),
    pytest.param({}, _both(["S", "LC"], [dict(slevel=0)], dict(seq_replay="bucket", bkt_db=8, bkt_sb=6)) +
                 _both(["S", "LC"], [dict(slevel=2)], dict(seq_replay="bucket", bkt_db=8, bkt_sb=10)), id="bucket-s0-s2"),
    # 28 context bits: the largest context whose key still packs ctx << 2 | base (30 bits)
    pytest.param({}, [("S", dict(slevel=7), dict(seq_packed=1, seq_replay="full", seq_digits=0x7777))], id="packed-s7"),
    pytest.param({"SA_SEQ_BUCKET": "0"}, _both(["S", "LC"], [dict(slevel=0)], dict(seq_packed=1, seq_replay="full",
                                                                                  seq_digits=0x77)), id="full_sort-s0"),
]

RBLOCK = [
    pytest.param({"SA_RB_APPLY": "1"}, [("Q", dict(lossy=r), dict(rblock=1, rb_apply_walk=1)) for r in (1.05, 1.15, 1.6)],
                 id="rb_apply"),
] + [
    pytest.param({"SA_RB_CHUNK": str(n)}, [("Q", dict(lossy=1.15), dict(rblock=1, rb_chunk=n, rb_apply_walk=0)),
                                           ("E", dict(lossy=1.15, md5=False), dict(rblock=1, rb_chunk=n, md5=None))],
                 id=f"rb_chunk{n}") for n in (8192, 4096, 1024, 32)
]


@pytest.mark.parametrize("env,steps", FRONT + AUX + SEQ + RBLOCK)
def test_path_matrix(monkeypatch, env, steps):
    _run(monkeypatch, env, steps)


# ---- the bare coder at the shape edges --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_streams():
    """Streams whose lengths sit on the 64-symbol segment edges and the 16 / 32
    record L-pass chunk edges, 40 short ones (more chains than the short
    chains' shared waves), and three around RV_LONG_SYMS, from the three
    generators of oracle_py.squeeze_streams: kind 0 fires the carry-less squeeze
    every few symbols (tot = 2 at probability 1/2) -- in a stream's only or
    last segment (lengths <= 64) and in segments before the last (longer
    ones, which restart) --, kind 1 wide totals up to 0xffe0, kind 2
    BASE_MODEL-sized totals (the three long streams: kinds 1 and 2).  Returns
    (streams, the oracle's bytes)."""
    rng = np.random.default_rng(19)
    edges = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
    lens = edges + [int(x) for x in rng.integers(1, 301, 40)] + [RV_LONG_SYMS - 1, RV_LONG_SYMS, RV_LONG_SYMS + 1]
    # (not the long ones: a restart round moves a stream past one squeezed segment, and the
    # driver gives up after 1000 rounds -- a squeeze per segment over 32,768 segments)
    squeeze = {33, 63, 64, 65, 129, 1025}
    streams = []
    for i, n in enumerate(lens):
        kind = 0 if (n in squeeze or (i >= len(edges) and i % 5 == 0)) else 1 + i % 2
        if kind == 0:
            t = np.full(n, 2, np.uint32); f = np.ones(n, np.uint32); c = np.ones(n, np.uint32)
        elif kind == 1:
            t = rng.integers(2, 0xffe1, n, dtype=np.uint32)
            f = np.maximum(1, (rng.random(n) * t).astype(np.uint32))
            c = (rng.random(n) * (t - f + 1)).astype(np.uint32)
        else:
            t = rng.integers(12, 253, n, dtype=np.uint32)
            f = np.maximum(1, (rng.random(n) * (t - 1)).astype(np.uint32))
            c = (rng.random(n) * (t - f + 1)).astype(np.uint32)
        streams.append((c.astype(np.uint16), f.astype(np.uint16), t.astype(np.uint16)))
    return streams, [oracle_py.rc_encode(*s) for s in streams]


def _check_streams(enc, expect):
    streams, want = _edge_streams()
    got = enc.code_records(streams)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"stream {i} of {len(streams[i][0])} symbols"
    assert enc.coder_restarts() > 0
    diff = _path_diff(enc.paths(), expect)
    assert not diff, f"bare coder: path (got, expected) {diff}"


@pytest.mark.parametrize("env,expect", [
    ({}, dict(r_short_shared=1, l_chunk=32, r_waves=4)),
    ({"SA_RV_SHORT_WAVES": "0"}, dict(r_short_shared=0, l_chunk=32)),
    ({"SA_L_CHUNK": "16"}, dict(r_short_shared=1, l_chunk=16)),
    ({"SA_RV_VARIANT": "0"}, dict(r_short_shared=1, pass_r="rv0")),
    ({"SA_RV_VARIANT": "5"}, dict(r_short_shared=1, pass_r="rv5")),
], ids=["default", "short_waves0", "l_chunk16", "rv0", "rv5"])
def test_coder_shape_edges(monkeypatch, env, expect):
    """sa_code_records against oracle_py.rc_encode on _edge_streams: every stream
    equal, squeezed streams restarted, and the short chains sharing waves
    exactly when SA_RV_SHORT_WAVES lets them."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = fq.Encoder(0)
    try:
        _check_streams(e, expect)
    finally:
        e.close()


# ---- coder variants and placement: S at the default config, then the bare-coder streams -------

CODER = [
    ({"SA_L_CHUNK": "16"}, dict(l_chunk=16), dict(l_chunk=16)),
    ({"SA_RV_SHORT_WAVES": "0"}, dict(r_short_shared=0), dict(r_short_shared=0)),
    ({"SA_RV_SHORT_WAVES": "1"}, dict(r_short_shared=1), dict(r_short_shared=1)),
    ({}, dict(r_short_shared=1, pass_r="rv6"), dict(r_short_shared=1, pass_r="rv6")),
    ({"SA_RV_V6_MAX": "-1"}, dict(pass_r="rv5"), dict(pass_r="rv5")),
    ({"SA_RV_V6_MAX": "0"}, dict(pass_r="rv6"), dict(pass_r="rv6")),
    ({"SA_CODER_WAVES": "1"}, dict(r_waves=1), dict(r_waves=1)),
    ({"SA_CODER_WAVES": "2"}, dict(r_waves=2), dict(r_waves=2)),
    ({"SA_MD5_PIPE": "1"}, dict(md5="pipe"), {}),
    ({"SA_LONG_CU_EVERY": "1", "SA_L_CU_EVERY": "1", "SA_HOST_WAITS": "0", "SA_LONG_GRID": "1", "SA_CHAIN_PRIO": "0",
      "SA_L_PRIO": "1", "SA_MD5_PRIO": "1"},
     dict(l_stream=1, host_waits=0, long_grid=1, chain_prio=0), dict(l_stream=1, chain_prio=0)),
    ({"SA_RV_CUS": "2", "SA_L_CU_EVERY": "4"}, dict(front_masked=1, l_stream=1), dict(l_stream=1)),
]


@pytest.mark.parametrize("env,expect,expect_coder", CODER,
                         ids=["l_chunk16", "short_waves0", "short_waves1", "default", "v6_max-1", "v6_max0",
                              "coder_waves1", "coder_waves2", "md5_pipe", "placement", "rv_cus2+l_cu4"])
def test_coder_and_placement(monkeypatch, env, expect, expect_coder):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = fq.Encoder(0)
    try:
        _step(e, "S", {}, dict(DENSE1, **expect))
        _check_streams(e, expect_coder)
    finally:
        e.close()


# ---- SA_SORT_MIN_DB: read once per process, so in a fresh child ------------------------------

def _child(spec):
    """(in the child process) the steps of `spec` on a fresh context; exits non-zero on a mismatch"""
    e = fq.Encoder(0)
    try:
        for name, cfg_kw, expect in spec:
            got = e.encode(_input(name), _cfg(cfg_kw))
            bad = _mismatch(got, _want(name, tuple(sorted(cfg_kw.items()))))
            diff = _path_diff(e.paths(), expect)
            if bad or diff:
                print(f"{name} {cfg_kw}: {bad or ''} path (got, expected) {diff}")
                sys.exit(1)
    finally:
        e.close()
    print("OK")


@pytest.mark.parametrize("spec", [
    [("S", dict(slevel=3), dict(seq_digits=0x8, aux_digits=0x9)), ("S", dict(slevel=5), dict(seq_digits=0x888))],
    [("M", dict(qlevel=3), dict(aux_sort="raw", aux_digits=0x888))],
], ids=["S-s3-s5", "M-q3"])
def test_sort_min_db8(spec):
    """SA_SORT_MIN_DB=8: no sort pass of fewer than 8 digit bits (the 21-bit AUX
    sort of Qlevel 3 in three passes of 8 instead of 7)."""
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_paths as t; t._child(json.loads(sys.argv[1]))"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(spec)], env=dict(os.environ, SA_SORT_MIN_DB="8"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-2000:])


# ---- state a context carries between batches --------------------------------------------------

def test_dense_flag_sequence(monkeypatch):
    """One context: S sorts its AUX space in one dense pass; M (more than 512
    models) in two and a copy, and turns the dense sort off; S again then
    takes the raw passes.  Each equal to the oracle, each path asserted."""
    _run(monkeypatch, {}, [("S", {}, dict(aux_dense_next=1, **DENSE1)),
                           ("M", {}, dict(aux_sort="dense2+copy", aux_runs="find_runs", aux_dense_next=0)),
                           ("S", {}, dict(RAW17, aux_dense_next=0))])


def test_buffer_reuse_after_largest_batch(monkeypatch):
    """The largest batch, then one block of one read, then S: grown buffers
    reused, and the AUX records zeroed between batches (prs_zero_*)."""
    _run(monkeypatch, {}, [("S1", {}, DENSE1), ("ONE", {}, DENSE1), ("S", {}, DENSE1), ("M", {}, {}), ("ONE", {}, RAW17)])


def test_batch_after_rejected_batch():
    """A batch the device rejects (a quality outside the model) leaves the
    context usable: the next batches are exact."""
    e = fq.Encoder(0)
    try:
        _step(e, "S", {}, DENSE1)
        with pytest.raises(fq.SeqArcError):
            e.encode([fq.parse_se(b"@r\nACGT\n+\nII\x7fI\n")], fq.Config())
        _step(e, "S", {}, DENSE1)
        _step(e, "M", {}, dict(aux_sort="dense2+copy"))
    finally:
        e.close()


def test_config_switches_on_one_context(monkeypatch):
    """-l 1.15, lossless, -l 1.6 (the R tables rebuilt); Slevel 3 (bucket), 8
    (full sort, unpacked keys), 3 again: one context each."""
    _run(monkeypatch, {}, [("S", dict(lossy=1.15), dict(rblock=1)), ("M", {}, dict(rblock=0)),
                           ("S", dict(lossy=1.6), dict(rblock=1)), ("M", dict(lossy=1.15), dict(rblock=1))])
    _run(monkeypatch, {}, [("S", dict(slevel=3), dict(seq_replay="bucket", seq_packed=1)),
                           ("S", dict(slevel=8), dict(seq_replay="full", seq_packed=0)),
                           ("M", dict(slevel=3), dict(seq_replay="bucket", seq_packed=1))])


def test_code_records_between_batches():
    """sa_code_records reuses the SEQ record array and the payload arena of the
    block encodes: interleaved on one context, each exact."""
    streams = oracle_py.squeeze_streams()
    want = [oracle_py.rc_encode(*s) for s in streams]
    e = fq.Encoder(0)
    try:
        for name in ("S", "M", "S"):
            assert e.code_records(streams) == want
            _step(e, name, {}, {})
        assert e.code_records(streams) == want
    finally:
        e.close()


@pytest.mark.parametrize("name,models,expect", [
    ("B512", 512, dict(aux_sort="dense1", aux_runs="runs_dense", aux_dense_next=1)),
    ("B513", 513, dict(aux_sort="dense2+copy", aux_runs="find_runs", aux_dense_next=0)),
])
def test_model_boundary(name, models, expect):
    """The dense AUX sort's limit, dmax > 512: a block of exactly 512 models (as
    the device counts them) sorts in one dense pass with k_runs_dense, one of
    exactly 513 in two.  tests/test_plan.py pins the two inputs on the CPU."""
    # (one name throughout: the ID analysis picks the ID bin, as tests/cpu_emu does -- no name models)
    bin_mode = int(fq.analyze_ids(_input(name)[0], True)[0])
    assert bin_mode == 1
    e = fq.Encoder(0)
    try:
        _step(e, name, dict(bin_mode=bin_mode), dict(expect, aux_nmod_max=models))
    finally:
        e.close()
