"""fastqueeze_amd -- MI355X (gfx950) SeqArc no-reference block encoder.

Thin ctypes binding of libseqarc_amd.so (include/seqarc_amd.h) used by the
tests and bench.py.  The product path is the HIP library; there is no CPU
fallback: if the library or a gfx950 device is missing, the calls raise.

Reference interface mirrored (SeqArc-1.6, cited by address in the binary):
  Encoder.encode()   EncapFqzComp::doFqzEncode@0x42d2d0 for a batch of blocks
  cut_se / cut_pe    SeqArcRead::doReadJob@0x432a80 / doReadPEJob@0x432d10
  parse_se / parse_pe AlignEncodeSEJob::getBlockRead@0x411b60 / getBlockReadPE@0x412920
  analyze_ids        IDProcess::analysisIDBinType@0x4310a0
  Encoder.code_records  the inlined RangeCoder (encode_seq@0x422010-0x422085)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import build as _build

__all__ = ["SeqArcError", "blocks_from_fastq", "Block", "Config", "Encoder", "cut_se", "cut_pe", "parse_se", "parse_pe", "analyze_ids",
           "load_library", "BLOCK_SIZE", "Input", "bgzf_scan", "Inflater", "BGZF_MEMBER", "INFLATE_STATUS",
           "Gunzipper", "GunzipState", "GunzipInfo", "Decoder", "DecodeInfo"]

BLOCK_SIZE = 50 << 20   # SeqArcParam BlockSize(M) = 50 (ctor @0x40776f)

_lib = None


class SeqArcError(RuntimeError):
    pass


class _SaBlock(C.Structure):
    _fields_ = [("names", C.c_void_p), ("name_lens", C.c_void_p), ("seq", C.c_void_p),
                ("seq_lens", C.c_void_p), ("qual", C.c_void_p), ("nreads", C.c_uint32)]


class _SaCfg(C.Structure):
    _fields_ = [("slevel", C.c_int32), ("qlevel", C.c_int32), ("md5", C.c_int32), ("bin_mode", C.c_int32),
                ("lossy", C.c_double)]


class _SaArcBlock(C.Structure):
    _fields_ = [("size", C.c_uint32), ("long_reads", C.c_uint32), ("text1", C.c_uint64), ("text2", C.c_uint64)]


class _SaArcInfo(C.Structure):
    _fields_ = [("file1", C.c_char_p), ("file2", C.c_char_p), ("paired", C.c_int32), ("gz1", C.c_int32),
                ("bare_plus", C.c_int32), ("md5", C.c_int32), ("lossy", C.c_int32), ("id_template", C.c_void_p),
                ("ref_md5", C.c_void_p), ("insert_size", C.c_uint32)]


class _SaDecoded(C.Structure):
    _fields_ = [("names", C.c_void_p), ("name_lens", C.c_void_p), ("seq", C.c_void_p), ("seq_lens", C.c_void_p),
                ("qual", C.c_void_p), ("name_cap", C.c_uint64), ("seq_cap", C.c_uint64), ("max_reads", C.c_uint32),
                ("nreads", C.c_uint32), ("md5_ok", C.c_int32)]


class _SaTextBlock(C.Structure):
    _fields_ = [("text1", C.c_void_p), ("len1", C.c_uint64), ("text2", C.c_void_p), ("len2", C.c_uint64)]


class _SaTextInfo(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("len_long", C.c_uint32), ("name_bytes", C.c_uint64),
                ("seq_bytes", C.c_uint64), ("out_bound", C.c_uint64)]


class _SaAlignCfg(C.Structure):
    _fields_ = [("index", C.c_void_p), ("paired", C.c_int32), ("maxmis", C.c_int32), ("good", C.c_int32),
                ("insert_size", C.c_uint32)]


class _SaRef(C.Structure):
    _fields_ = [("genome", C.c_void_p), ("bases", C.c_uint64), ("paired", C.c_int32), ("maxmis", C.c_int32),
                ("insert_size", C.c_uint32)]


_PATH_FIELDS = ("prep", "front_counter", "wg_per_cu", "emit", "dege_list", "seq_packed", "seq_replay", "bkt_inv",
                "bkt_lpt", "bkt_db", "bkt_sb", "aux_sort", "aux_runs", "aux_nmod_max", "aux_dense_next", "pass_r",
                "r_short_shared", "r_waves", "l_chunk", "l_stream", "host_waits", "long_grid", "chain_prio", "md5",
                "rblock", "rb_spec_counter", "rb_fix_wave", "rb_apply_walk", "rb_chunk", "exact_rerun", "seq_digits",
                "aux_digits", "front_masked")
# the names of sa_paths' enumerated fields (include/seqarc_amd.h, SA_PATH_*)
_PATH_NAMES = {"prep": {0: None, 1: "row16", 2: "row64", 3: "fused", 4: "wave"},
               "emit": {0: None, 1: "row16", 2: "wave"},
               "seq_replay": {0: None, 1: "bucket", 2: "full"},
               "aux_sort": {0: None, 1: "dense1", 2: "dense2+copy", 3: "raw"},
               "aux_runs": {0: None, 1: "runs_dense", 2: "find_runs"},
               "pass_r": {0: None, 1: "rv0", 2: "rv5", 3: "rv6", 4: "lanes"},
               "md5": {0: None, 1: "plain", 2: "pipe", 3: "wave"}}


class _SaPaths(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in _PATH_FIELDS]


class _SaOut(C.Structure):
    _fields_ = [("data", C.c_void_p), ("cap", C.c_uint64), ("size", C.c_uint64)]


def load_library(path: str | None = None):
    """Load libseqarc_amd.so (building it first if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    if path is None and os.environ.get("SA_LIB"):   # (A/B runs: another build of the library)
        path = os.environ["SA_LIB"]
    if path is None:
        path = _build.LIB
        if _build.needs_build():
            if os.environ.get("SA_NO_BUILD"):   # (GPU runs: the library travels prebuilt)
                raise SeqArcError("libseqarc_amd.so is older than its sources and SA_NO_BUILD is set")
            _build.build()
    if not os.path.exists(path):
        raise SeqArcError(f"libseqarc_amd.so not found at {path}")
    lib = C.CDLL(path)
    P, U64, I64, I32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int
    sigs = {
        "sa_create": ([I32], P), "sa_destroy": ([P], None), "sa_last_error": ([P], C.c_char_p),
        "sa_version": ([], C.c_char_p), "sa_output_bound": ([P], U64),
        "sa_encode_blocks": ([P, P, I32, P, P], I32), "sa_stage": ([P, P, I32], I32),
        "sa_run": ([P, P], I32), "sa_fetch": ([P, P, I32], I32), "sa_fetch_sizes": ([P, P, I32], I32),
        "sa_phase_times": ([P, P, P, I32], I32), "sa_set_timing": ([P, I32], None),
        "sa_cut_se": ([P, U64, U64, P, U64], I64), "sa_cut_pe": ([P, U64, P, U64, U64, P, P, U64], I64),
        "sa_parse_se": ([P, U64, P, P, P, P, P], I64), "sa_parse_pe": ([P, U64, P, U64, P, P, P, P, P], I64),
        "sa_analyze_ids": ([P, I32, P], I32),
        "sa_code_records": ([P, I32, P, P, P, P, P, U64, P], I32), "sa_coder_restarts": ([P], C.c_uint32),
        "sa_last_paths": ([P, P], I32),
        "sa_stream_stats": ([P, P, P], None), "sa_device_bytes": ([P], U64), "sa_front_bytes": ([P], U64),
        "sa_create_shared": ([I32, P], P),
        "sa_input_create": ([I32, P, I32], P), "sa_input_destroy": ([P], None), "sa_run_input": ([P, P, P], I32),
        "sa_arc_header": ([U64, P], I32), "sa_arc_trailer": ([P, P, C.c_uint32, P, U64], I64),
        "sa_arc_trailer2": ([P, C.c_int32, P, C.c_uint32, P, U64], I64),
        "sa_decode_block": ([P, U64, P, P, I32, P], I64),
        "sa_host_register": ([P, U64], I32), "sa_host_unregister": ([P], I32),
        "sa_stage_text": ([P, P, I32, P], I32), "sa_host_alloc": ([U64], P), "sa_host_free": ([P], None),
        "sa_text_upload": ([P, P, I32, I32, I32, P, U64], I32), "sa_text_parse": ([P, P, I32, P, I32, U64, P], I32),
        "sa_hash_build": ([P, P, U64, C.c_uint32, C.c_uint32, C.c_uint32], P),
        "sa_hash_file_bytes": ([P], U64), "sa_hash_serialize": ([P, P, P, U64], I32),
        "sa_hash_genome_length": ([P], C.c_uint32), "sa_hash_destroy": ([P], None),
        "sa_hash_align": ([P, P, P, P, P, I64, C.c_int32, C.c_int32, P, P, P, P, P, P], I32),
        "sa_align_chain_create": ([C.c_int32, C.c_int32], P), "sa_align_chain_destroy": ([P], None),
        "sa_run_input_aligned": ([P, P, P, P, P, U64], I32), "sa_run_aligned": ([P, P, P, P, U64], I32),
        "sa_encode_blocks_aligned": ([P, P, I32, P, P, P, P], I32),
        "sa_hash_load": ([P, P, U64], P), "sa_hash_packed": ([P, P, P, U64], I32),
        "sa_hash_align_kernel_ms": ([P], C.c_float),
        "sa_decode_block_ref": ([P, U64, P, P, I32, P, P], I64),
        "sa_bgzf_scan": ([P, U64, P, U64, P, P], I64),
        "sa_inflater_create": ([I32], P), "sa_inflater_destroy": ([P], None),
        "sa_inflate_members": ([P, P, U64, P, C.c_uint32, P, U64, P], I32),
        "sa_inflater_error": ([P], C.c_char_p), "sa_inflater_kernel_ms": ([P], C.c_float),
        "sa_inflater_grid": ([P], C.c_uint32),
        "sa_gunzipper_create": ([I32], P), "sa_gunzipper_destroy": ([P], None),
        "sa_gunzip_run": ([P, P, U64, I32, P, P, U64, P, P, P], I32),
        "sa_gunzipper_error": ([P], C.c_char_p), "sa_gunzipper_kernel_ms": ([P], C.c_float),
        "sa_gunzipper_grid": ([P], C.c_uint32), "sa_gunzipper_chunk": ([P], C.c_uint32),
        "sa_cut_next_se": ([P, U64, I32, U64, P, U64], I64),
        "sa_cut_next_pe": ([P, U64, I32, P, U64, I32, U64, P, U64, P, P], I32),
        "sa_devtext_create": ([I32, U64], P), "sa_devtext_destroy": ([P], None),
        "sa_devtext_error": ([P], C.c_char_p), "sa_devtext_avail": ([P], U64), "sa_devtext_room": ([P], U64),
        "sa_devtext_append": ([P, P, U64], I32), "sa_inflate_members_dev": ([P, P, U64, P, C.c_uint32, P, P], I32),
        "sa_devtext_peek": ([P, U64, P, U64], I32),
        "sa_devtext_cut": ([P, I32, P, I32, U64, P, U64, P, P, U64, P], I64),
        "sa_devtext_take": ([P, U64, P, U64], P), "sa_devblock_release": ([P], None),
        "sa_devblock_lens": ([P, P, P], I32), "sa_devblock_fetch": ([P, P, P], I32),
        "sa_devblock_pool_trim": ([I32], None),
        "sa_text_upload_dev": ([P, P, I32, I32, I32, P, U64], I32), "sa_upload_error": ([P], C.c_char_p),
        "sa_devtext_kernel_ms": ([P, P, P], None), "sa_devtext_count_bytes": ([P], U64),
        "sa_gunzip_run_dev": ([P, P, U64, I32, P, P, U64, P, P, P], I32),
        "sa_decoder_create": ([I32], P), "sa_decoder_destroy": ([P], None), "sa_decoder_error": ([P], C.c_char_p),
        "sa_decode_blocks": ([P, P, P, P, C.c_uint32, P, P, I32, P, P], I32), "sa_decoder_info": ([P, P], None),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


@dataclass
class Block:
    """One parsed block: the SeqArcMemBuf SoA (PE reads interleaved r1, r2)."""
    names: np.ndarray       # uint8, IDs without '@'
    name_lens: np.ndarray   # uint16
    seq: np.ndarray         # uint8
    seq_lens: np.ndarray    # int32
    qual: np.ndarray        # uint8
    text_bytes: int = 0     # FASTQ bytes this block was parsed from
    text1: int = 0          # ... of them in input 1 (ReadBuf+0xc)
    text2: int = 0          # ... in input 2 (ReadBuf+0x10)

    @property
    def nreads(self) -> int:
        return int(self.name_lens.shape[0])

    def _c(self) -> _SaBlock:
        return _SaBlock(_ptr(self.names), _ptr(self.name_lens), _ptr(self.seq), _ptr(self.seq_lens),
                        _ptr(self.qual), self.nreads)


@dataclass
class Config:
    """SeqArcParam fields of the no-ref path (defaults of SeqArcParam::SeqArcParam@0x407490)."""
    slevel: int = 3
    qlevel: int = 2
    md5: bool = True
    bin_mode: int = 0
    lossy: float = 0.0     # -l R (R-Block lossy qualities, rblock@0x426c10); 0 = lossless

    def _c(self) -> _SaCfg:
        return _SaCfg(self.slevel, self.qlevel, 1 if self.md5 else 0, 1 if self.bin_mode else 0, float(self.lossy))


def _as_u8(text) -> np.ndarray:
    if isinstance(text, np.ndarray):
        return text.view(np.uint8).reshape(-1)
    return np.frombuffer(text, dtype=np.uint8)


def cut_se(text, block_size: int = BLOCK_SIZE) -> list[tuple[int, int]]:
    lib = load_library()
    t = _as_u8(text)
    maxb = t.size // 1024 + 16
    ends = np.zeros(maxb, dtype=np.uint64)
    n = lib.sa_cut_se(_ptr(t), t.size, block_size, _ptr(ends), maxb)
    if n < 0:
        raise SeqArcError("block cut failed")
    e = [0] + ends[:n].astype(np.int64).tolist()
    return [(e[i], e[i + 1]) for i in range(n)]


def cut_pe(t1, t2, block_size: int = BLOCK_SIZE):
    lib = load_library()
    a, b = _as_u8(t1), _as_u8(t2)
    maxb = (a.size + b.size) // 1024 + 16
    e1 = np.zeros(maxb, dtype=np.uint64)
    e2 = np.zeros(maxb, dtype=np.uint64)
    n = lib.sa_cut_pe(_ptr(a), a.size, _ptr(b), b.size, block_size, _ptr(e1), _ptr(e2), maxb)
    if n < 0:
        raise SeqArcError("PE block cut failed")
    x = [0] + e1[:n].astype(np.int64).tolist()
    y = [0] + e2[:n].astype(np.int64).tolist()
    return [((x[i], x[i + 1]), (y[i], y[i + 1])) for i in range(n)]


def cut_next_se(win, eof: bool, block_size: int, first) -> int | None:
    """sa_cut_next_se: the next block's bytes in a window, or None (read more / no cut)."""
    lib = load_library()
    w, f = _as_u8(win), _as_u8(first)
    dummy = np.zeros(1, np.uint8)
    r = lib.sa_cut_next_se(_ptr(w) or dummy.ctypes.data, w.size, 1 if eof else 0, block_size, _ptr(f), f.size)
    return None if r < 0 else int(r)


def cut_next_pe(w1, eof1: bool, w2, eof2: bool, block_size: int, first) -> tuple[int, int] | None:
    """sa_cut_next_pe: the next block's bytes of each input, or None (read more / no cut)."""
    lib = load_library()
    a, b, f = _as_u8(w1), _as_u8(w2), _as_u8(first)
    dummy = np.zeros(1, np.uint8)
    e1, e2 = C.c_uint64(0), C.c_uint64(0)
    r = lib.sa_cut_next_pe(_ptr(a) or dummy.ctypes.data, a.size, 1 if eof1 else 0, _ptr(b) or dummy.ctypes.data, b.size,
                           1 if eof2 else 0, block_size, _ptr(f), f.size, C.byref(e1), C.byref(e2))
    return None if r != 0 else (int(e1.value), int(e2.value))


def _alloc(nbytes: int):
    return (np.empty(nbytes + 16, np.uint8), np.empty(nbytes // 4 + 8, np.uint16), np.empty(nbytes + 16, np.uint8),
            np.empty(nbytes // 4 + 8, np.int32), np.empty(nbytes + 16, np.uint8))


def _trim(names, nl, seq, sl, qual, n, text_bytes) -> Block:
    nl = nl[:n].copy()
    sl = sl[:n].copy()
    tn = int(nl.sum(dtype=np.int64))
    ts = int(sl.sum(dtype=np.int64))
    return Block(names[:tn].copy(), nl, seq[:ts].copy(), sl, qual[:ts].copy(), text_bytes)


def parse_se(text) -> Block:
    lib = load_library()
    t = _as_u8(text)
    names, nl, seq, sl, qual = _alloc(t.size)
    n = lib.sa_parse_se(_ptr(t), t.size, _ptr(names), _ptr(nl), _ptr(seq), _ptr(sl), _ptr(qual))
    if n < 0:
        raise SeqArcError("FASTQ parse failed")
    return _trim(names, nl, seq, sl, qual, n, t.size)


def parse_pe(t1, t2) -> Block:
    lib = load_library()
    a, b = _as_u8(t1), _as_u8(t2)
    names, nl, seq, sl, qual = _alloc(a.size + b.size)
    n = lib.sa_parse_pe(_ptr(a), a.size, _ptr(b), b.size, _ptr(names), _ptr(nl), _ptr(seq), _ptr(sl), _ptr(qual))
    if n < 0:
        raise SeqArcError("PE FASTQ parse failed")
    return _trim(names, nl, seq, sl, qual, n, a.size + b.size)


def analyze_ids(first: Block, single_end: bool) -> np.ndarray:
    lib = load_library()
    tmpl = np.zeros(512, dtype=np.uint8)
    cb = first._c()
    if lib.sa_analyze_ids(C.byref(cb), 1 if single_end else 0, _ptr(tmpl)) != 0:
        raise SeqArcError("ID template analysis failed (the reference would throw)")
    return tmpl


def blocks_from_fastq(t1, t2=None, block_size: int = BLOCK_SIZE) -> list[Block]:
    """Cut and parse FASTQ text exactly as the reference's reader does."""
    if t2 is None:
        a = _as_u8(t1)
        return [parse_se(a[s:e]) for s, e in cut_se(a, block_size)]
    a, b = _as_u8(t1), _as_u8(t2)
    out = []
    for (s1, e1), (s2, e2) in cut_pe(a, b, block_size):
        blk = parse_pe(a[s1:e1], b[s2:e2])
        blk.text1, blk.text2 = e1 - s1, e2 - s2
        out.append(blk)
    return out


class Encoder:
    """A gfx950 device context of libseqarc_amd (one per device / host thread)."""

    PHASES = 11

    def __init__(self, device: int = 0, share_with: "Encoder | None" = None):
        """share_with: another Encoder of the same device whose front scratch this
        one shares (sa_create_shared): their fronts then run one at a time."""
        self._lib = load_library()
        self._ctx = (self._lib.sa_create_shared(device, share_with._ctx) if share_with is not None
                     else self._lib.sa_create(device))
        if not self._ctx:
            raise SeqArcError(f"no usable gfx950 device {device} (the HIP path is the only path)")
        self._staged: list[int] | None = []   # output bound of each staged block

    def close(self):
        if self._ctx:
            self._lib.sa_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        msg = self._lib.sa_last_error(self._ctx)
        raise SeqArcError(f"{what}: {msg.decode() if msg else 'unknown error'}")

    def set_timing(self, on: bool = True):
        self._lib.sa_set_timing(self._ctx, 1 if on else 0)

    def stage(self, blocks: list[Block]):
        self._staged = [int(self._lib.sa_output_bound(C.byref(b._c()))) for b in blocks]
        arr = (_SaBlock * max(1, len(blocks)))(*[b._c() for b in blocks])
        if self._lib.sa_stage(self._ctx, arr, len(blocks)) != 0:
            self._err("sa_stage")

    def stage_text(self, texts) -> list[dict]:
        """sa_stage_text: blocks given as FASTQ text, [(text1, text2 or None)]
        as the reader cut them, parsed on the device.  Returns per-block counts."""
        keep = [(_as_u8(a), None if b is None else _as_u8(b)) for a, b in texts]
        dummy = np.zeros(1, np.uint8)   # (an empty PE mate text still needs a non-NULL pointer)
        arr = (_SaTextBlock * max(1, len(keep)))(*[
            _SaTextBlock(_ptr(a) or dummy.ctypes.data, a.size,
                         None if b is None else (_ptr(b) or dummy.ctypes.data), 0 if b is None else b.size)
            for a, b in keep])
        info = (_SaTextInfo * max(1, len(keep)))()
        if self._lib.sa_stage_text(self._ctx, arr, len(keep), info) != 0:
            self._staged = None
            self._err("sa_stage_text")
        self._staged = [int(info[i].out_bound) for i in range(len(keep))]
        return [{"nreads": int(info[i].nreads), "len_long": int(info[i].len_long),
                 "name_bytes": int(info[i].name_bytes), "seq_bytes": int(info[i].seq_bytes)} for i in range(len(keep))]

    def stage_text_streamed(self, texts, slot: int = 0, stride: int | None = None) -> list[dict]:
        """sa_text_upload block by block into text arena `slot`, then
        sa_text_parse: what the command line does as its reader cuts blocks.
        Returns per-block counts as stage_text does."""
        keep = [(_as_u8(a), None if b is None else _as_u8(b)) for a, b in texts]
        if stride is None:
            stride = max([a.size for a, _ in keep] + [0 if b is None else b.size for _, b in keep] + [1])
        dummy = np.zeros(1, np.uint8)
        blks = [_SaTextBlock(_ptr(a) or dummy.ctypes.data, a.size,
                             None if b is None else (_ptr(b) or dummy.ctypes.data), 0 if b is None else b.size)
                for a, b in keep]
        for i, tb in enumerate(blks):
            if self._lib.sa_text_upload(self._ctx, None, slot, i, len(blks), C.byref(tb), stride) != 0:
                self._staged = None
                self._err("sa_text_upload")
        arr = (_SaTextBlock * max(1, len(blks)))(*blks)
        info = (_SaTextInfo * max(1, len(keep)))()
        if self._lib.sa_text_parse(self._ctx, None, slot, arr, len(keep), stride, info) != 0:
            self._staged = None
            self._err("sa_text_parse")
        self._staged = [int(info[i].out_bound) for i in range(len(keep))]
        return [{"nreads": int(info[i].nreads), "len_long": int(info[i].len_long),
                 "name_bytes": int(info[i].name_bytes), "seq_bytes": int(info[i].seq_bytes)} for i in range(len(keep))]

    def stage_devblocks(self, blocks: "list[DevBlock]", slot: int = 0) -> list[dict]:
        """sa_text_upload_dev of each devblock (device to device) into text arena
        `slot`, then sa_text_parse: the blocks staged as stage_text stages their
        texts, which never were on the host.  Returns per-block counts as stage_text does."""
        lens = [b.lens for b in blocks]
        stride = max([max(l1, l2) for l1, l2 in lens] + [1])
        for i, b in enumerate(blocks):
            if self._lib.sa_text_upload_dev(self._ctx, None, slot, i, len(blocks), b._h, stride) != 0:
                self._staged = None
                raise SeqArcError(f"sa_text_upload_dev: {self._lib.sa_upload_error(self._ctx).decode()}")
        dummy = np.zeros(1, np.uint8)   # (text1 / text2 only tell SE from PE)
        arr = (_SaTextBlock * max(1, len(blocks)))(*[
            _SaTextBlock(dummy.ctypes.data, l1, dummy.ctypes.data if b.paired else None, l2)
            for b, (l1, l2) in zip(blocks, lens)])
        info = (_SaTextInfo * max(1, len(blocks)))()
        if self._lib.sa_text_parse(self._ctx, None, slot, arr, len(blocks), stride, info) != 0:
            self._staged = None
            self._err("sa_text_parse")
        self._staged = [int(info[i].out_bound) for i in range(len(blocks))]
        return [{"nreads": int(info[i].nreads), "len_long": int(info[i].len_long),
                 "name_bytes": int(info[i].name_bytes), "seq_bytes": int(info[i].seq_bytes)} for i in range(len(blocks))]

    def run(self, cfg: Config):
        c = cfg._c()
        if self._lib.sa_run(self._ctx, C.byref(c)) != 0:
            self._err("sa_run")

    def fetch_sizes(self) -> list[int]:
        """The encoded size of each block of the last run (sa_fetch_sizes: what
        fetch() will return, known before the copies)."""
        if self._staged is None:
            raise SeqArcError("fetch_sizes(): nothing staged")
        n = len(self._staged)
        sizes = np.zeros(max(1, n), dtype=np.uint64)
        if self._lib.sa_fetch_sizes(self._ctx, _ptr(sizes), n) != 0:
            self._err("sa_fetch_sizes")
        return [int(x) for x in sizes[:n]]

    def fetch(self) -> list[bytes]:
        if self._staged is None:
            raise SeqArcError("fetch(): nothing staged (encode_blocks() fetched its own output; stage() or "
                              "run_input() first)")
        # (the host buffers are kept for the next fetch: freeing memory the
        # device-to-host copies page-locked stalls the GPU's queues while other
        # contexts run -- DESIGN.md, round 5)
        bufs = self.__dict__.setdefault("_fetch_bufs", [])
        outs, keep = [], []
        for i, cap in enumerate(self._staged):
            if i == len(bufs):
                bufs.append(np.empty(0, dtype=np.uint8))
            if bufs[i].size < cap:
                bufs[i] = np.empty(cap + cap // 8, dtype=np.uint8)
            keep.append(bufs[i])
            outs.append(_SaOut(_ptr(bufs[i]), cap, 0))
        arr = (_SaOut * max(1, len(outs)))(*outs)
        if self._lib.sa_fetch(self._ctx, arr, len(outs)) != 0:
            self._err("sa_fetch")
        return [keep[i][: arr[i].size].tobytes() for i in range(len(outs))]

    def encode_blocks(self, blocks: list[Block], cfg: Config) -> list[bytes]:
        """One sa_encode_blocks call (the drop-in for doFqzEncode over a batch;
        the library splits batches larger than its HBM cap into sub-batches)."""
        ins = (_SaBlock * max(1, len(blocks)))(*[b._c() for b in blocks])
        keep, outs = [], []
        for b in blocks:
            cb = b._c()
            cap = int(self._lib.sa_output_bound(C.byref(cb)))
            buf = np.empty(cap, dtype=np.uint8)
            keep.append(buf)
            outs.append(_SaOut(_ptr(buf), cap, 0))
        arr = (_SaOut * max(1, len(outs)))(*outs)
        c = cfg._c()
        if self._lib.sa_encode_blocks(self._ctx, ins, len(blocks), C.byref(c), arr) != 0:
            self._err("sa_encode_blocks")
        self._staged = None   # the context's last output is a sub-batch: nothing to fetch()
        return [keep[i][: arr[i].size].tobytes() for i in range(len(outs))]

    def run_input(self, inp: "Input", cfg: Config):
        """Encode a resident batch (sa_run_input); fetch() then returns its blocks."""
        c = cfg._c()
        if self._lib.sa_run_input(self._ctx, inp._h, C.byref(c)) != 0:
            self._err("sa_run_input")
        self._staged = [int(self._lib.sa_output_bound(C.byref(b._c()))) for b in inp.blocks]

    def run_aligned(self, cfg: Config, index: "HashIndex", paired: bool, chain: "AlignChain",
                    batch: int | None = None, inp: "Input | None" = None, maxmis: int = 7, good: int = 1,
                    insert_size: int = 0):
        """The staged batch (or `inp`) through the reference path
        (sa_run_input_aligned; doAlignEncode@0x42d4c0 per block); fetch() then."""
        c = cfg._c()
        a = _SaAlignCfg(index._h, 1 if paired else 0, maxmis, good, insert_size)
        b = 0xFFFFFFFFFFFFFFFF if batch is None else int(batch)
        if inp is None:
            rc = self._lib.sa_run_aligned(self._ctx, C.byref(c), C.byref(a), chain._h, b)
        else:
            rc = self._lib.sa_run_input_aligned(self._ctx, inp._h, C.byref(c), C.byref(a), chain._h, b)
            self._staged = [int(self._lib.sa_output_bound(C.byref(x._c()))) for x in inp.blocks]
        if rc != 0:
            self._err("sa_run_input_aligned")

    def encode_aligned(self, blocks: list[Block], cfg: Config, index: "HashIndex", paired: bool,
                       chain: "AlignChain | None" = None, **kw) -> list[bytes]:
        """stage + run_aligned + fetch (a fresh chain unless one is given)."""
        own = chain is None
        chain = chain or AlignChain()
        try:
            self.stage(blocks)
            self.run_aligned(cfg, index, paired, chain, **kw)
            return self.fetch()
        finally:
            if own:
                chain.close()

    def device_bytes(self) -> int:
        return int(self._lib.sa_device_bytes(self._ctx))

    def front_bytes(self) -> int:
        return int(self._lib.sa_front_bytes(self._ctx))

    def encode(self, blocks: list[Block], cfg: Config) -> list[bytes]:
        self.stage(blocks)
        self.run(cfg)
        return self.fetch()

    def code_records(self, streams) -> list[bytes]:
        """Range-code pre-modelled streams [(cum, freq, tot) uint16 arrays] on the GPU."""
        lens = np.array([len(c) for c, _, _ in streams], dtype=np.uint32)
        cat = [np.ascontiguousarray(np.concatenate([s[k] for s in streams]) if streams else np.zeros(0), dtype=np.uint16)
               for k in range(3)]
        cap = int(2 * lens.sum() + 64 * len(streams) + 16)
        out = np.empty(cap, dtype=np.uint8)
        ol = np.zeros(max(1, len(streams)), dtype=np.uint64)
        if self._lib.sa_code_records(self._ctx, len(streams), _ptr(lens), _ptr(cat[0]), _ptr(cat[1]), _ptr(cat[2]),
                                     _ptr(out), cap, _ptr(ol)) != 0:
            self._err("sa_code_records")
        res, o = [], 0
        for i in range(len(streams)):
            res.append(out[o:o + int(ol[i])].tobytes())
            o += int(ol[i])
        return res

    def coder_restarts(self) -> int:
        return int(self._lib.sa_coder_restarts(self._ctx))

    def paths(self) -> dict:
        """What the host chose for the last run / code_records (sa_last_paths):
        the fields of sa_paths, the enumerated ones by name (prep: row16 / row64
        / fused / wave; emit: row16 / wave; seq_replay: bucket / full; aux_sort:
        dense1 / dense2+copy / raw; aux_runs: runs_dense / find_runs; pass_r:
        rv0 / rv5 / rv6 / lanes; md5: plain (a message per lane) / pipe / wave; None: the stage did not
        run), the others as integers (seq_digits / aux_digits: a sort's digit
        widths, four bits a pass, the first pass lowest)."""
        p = _SaPaths()
        if self._lib.sa_last_paths(self._ctx, C.byref(p)) != 0:
            self._err("sa_last_paths")
        out = {f: int(getattr(p, f)) for f in _PATH_FIELDS}
        for f, names in _PATH_NAMES.items():
            out[f] = names[out[f]]
        return out

    def stream_stats(self) -> tuple[int, int]:
        """(symbols of the longest coder stream, symbols of all streams) of the last run."""
        mx, tot = C.c_uint64(0), C.c_uint64(0)
        self._lib.sa_stream_stats(self._ctx, C.byref(mx), C.byref(tot))
        return int(mx.value), int(tot.value)

    def phase_times(self) -> dict[str, float]:
        names = (C.c_char_p * self.PHASES)()
        ms = (C.c_float * self.PHASES)()
        n = self._lib.sa_phase_times(self._ctx, names, ms, self.PHASES)
        return {names[i].decode(): float(ms[i]) for i in range(n)}


class HostBuffer:
    """Page-locked host memory (sa_host_alloc: portable across devices, so a copy
    from it is a DMA) seen as a numpy uint8 array: where sa_stage_text wants the
    reader's text windows."""

    def __init__(self, nbytes: int):
        self._lib = load_library()
        self._p = self._lib.sa_host_alloc(max(1, nbytes))
        if not self._p:
            raise SeqArcError(f"sa_host_alloc({nbytes}) failed")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(self._p))[:nbytes]

    def close(self):
        if self._p:
            self.array = None
            self._lib.sa_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# sa_bgzf_member (include/seqarc_amd.h): a member's deflate bytes in the input and its place in the output
BGZF_MEMBER = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("out_off", "<u8"), ("isize", "<u4"), ("crc", "<u4")],
                       align=True)
INFLATE_STATUS = {0: "ok", 1: "input overrun", 2: "bad block type or stored length", 3: "bad code lengths",
                  4: "distance too far", 5: "output size is not ISIZE", 6: "CRC mismatch", 7: "not a gzip member header"}


def bgzf_scan(data, max_members: int | None = None):
    """sa_bgzf_scan: the whole BGZF members of `data` as a BGZF_MEMBER array, the
    bytes they take and the bytes they inflate to.  A member cut by the end of
    `data` is left out (consumed < len(data)); raises on anything that is not BGZF."""
    lib = load_library()
    a = _as_u8(data)
    cap = max_members if max_members is not None else a.size // 26 + 1
    ms = np.zeros(max(1, cap), BGZF_MEMBER)
    consumed, out_bytes = C.c_uint64(0), C.c_uint64(0)
    n = lib.sa_bgzf_scan(_ptr(a), a.size, ms.ctypes.data, cap, C.byref(consumed), C.byref(out_bytes))
    if n < 0:
        raise SeqArcError({-1: "not BGZF (malformed member header)", -2: "a BGZF member larger than 64 KiB",
                           -3: f"more than {cap} BGZF members"}.get(n, f"sa_bgzf_scan: {n}"))
    return ms[:n], consumed.value, out_bytes.value


class Inflater:
    """BGZF members inflated on the device (sa_inflater_*): one wave per member,
    CRC-32 checked there.  Its device slabs grow on demand and are kept."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = self._lib.sa_inflater_create(device)
        if not self._h:
            raise SeqArcError(f"sa_inflater_create failed: no usable gfx950 device {device}")

    def close(self):
        if self._h:
            self._lib.sa_inflater_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def last_kernel_ms(self) -> float:
        return float(self._lib.sa_inflater_kernel_ms(self._h))

    @property
    def grid(self) -> int:
        """(tests and diagnostics) Workgroups (waves) a launch uses at most (SA_INFL_GRID)."""
        return int(self._lib.sa_inflater_grid(self._h))

    def inflate_into(self, data, members: np.ndarray, out: np.ndarray) -> tuple[int, np.ndarray]:
        """sa_inflate_members into the uint8 array `out`; (return value, status)."""
        a = _as_u8(data)
        ms = np.ascontiguousarray(members, BGZF_MEMBER)
        status = np.zeros(max(1, ms.size), np.uint32)
        rc = self._lib.sa_inflate_members(self._h, _ptr(a), a.size, ms.ctypes.data, ms.size, _ptr(out), out.size,
                                          status.ctypes.data)
        if rc < 0:
            raise SeqArcError(f"sa_inflate_members ({rc}): {self._lib.sa_inflater_error(self._h).decode()}")
        return rc, status[:ms.size]

    def inflate_to(self, devtext: "DevText", data, members: np.ndarray) -> tuple[int, np.ndarray]:
        """sa_inflate_members_dev: the members' text appended to the devtext, never
        on the host; (return value, status).  -3: more text than devtext.room (nothing done)."""
        a = _as_u8(data)
        ms = np.ascontiguousarray(members, BGZF_MEMBER)
        status = np.zeros(max(1, ms.size), np.uint32)
        rc = self._lib.sa_inflate_members_dev(self._h, _ptr(a), a.size, ms.ctypes.data, ms.size, devtext._h,
                                              status.ctypes.data)
        if rc < 0 and rc != -3:
            raise SeqArcError(f"sa_inflate_members_dev ({rc}): {self._lib.sa_inflater_error(self._h).decode()}")
        return rc, status[:ms.size]

    def inflate_members(self, data, members: np.ndarray) -> tuple[bytes, np.ndarray]:
        """The members' output (a buffer that ends with the last member's bytes;
        a failed member's range is undefined) and the per-member status."""
        ms = np.ascontiguousarray(members, BGZF_MEMBER)
        size = int((ms["out_off"] + ms["isize"]).max()) if ms.size else 0
        out = np.zeros(size, np.uint8)
        _, status = self.inflate_into(data, ms, out)
        return out.tobytes(), status

    def inflate_bgzf(self, data) -> bytes:
        """A whole BGZF file's text."""
        a = _as_u8(data)
        ms, consumed, _ = bgzf_scan(a)
        if consumed != a.size:
            raise SeqArcError(f"BGZF input ends inside a member (at byte {consumed} of {a.size})")
        out, status = self.inflate_members(a, ms)
        bad = np.flatnonzero(status)
        if bad.size:
            i = int(bad[0])
            raise SeqArcError(f"BGZF member {i} failed to inflate: status {int(status[i])} "
                              f"({INFLATE_STATUS.get(int(status[i]), '?')})")
        return out


CUT_MORE, CUT_DONE, CUT_FULL, CUT_NONE = 1, 2, 3, 4   # SA_CUT_*: why DevText.cut stopped


class DevBlock:
    """One block's text in device memory (sa_devblock), as DevText.take cut it."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = handle
        l1, l2 = C.c_uint64(0), C.c_uint64(0)
        self.paired = bool(self._lib.sa_devblock_lens(handle, C.byref(l1), C.byref(l2)))
        self.lens = (int(l1.value), int(l2.value))

    def fetch(self) -> tuple[bytes, bytes | None]:
        """The block's texts copied to the host."""
        a = np.empty(self.lens[0], np.uint8)
        b = np.empty(self.lens[1], np.uint8)
        dummy = np.zeros(1, np.uint8)
        if self._lib.sa_devblock_fetch(self._h, _ptr(a) or dummy.ctypes.data, _ptr(b) or dummy.ctypes.data) != 0:
            raise SeqArcError("sa_devblock_fetch failed")
        return a.tobytes(), (b.tobytes() if self.paired else None)

    def close(self):
        if self._h:
            self._lib.sa_devblock_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevText:
    """One input's FASTQ text as a stream in device memory (sa_devtext): appended
    from the host or inflated into by Inflater.inflate_to, cut on the device."""

    def __init__(self, capacity: int, device: int = 0):
        self._lib = load_library()
        self._h = self._lib.sa_devtext_create(device, capacity)
        if not self._h:
            raise SeqArcError(f"sa_devtext_create failed: no usable gfx950 device {device}, or no memory")

    def close(self):
        if self._h:
            self._lib.sa_devtext_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise SeqArcError(f"{what}: {self._lib.sa_devtext_error(self._h).decode()}")

    @property
    def avail(self) -> int:
        return int(self._lib.sa_devtext_avail(self._h))

    @property
    def room(self) -> int:
        return int(self._lib.sa_devtext_room(self._h))

    @property
    def kernel_ms(self) -> tuple[float, float]:
        """Device time of the last newline count and the last cut."""
        a, b = C.c_float(0), C.c_float(0)
        self._lib.sa_devtext_kernel_ms(self._h, C.byref(a), C.byref(b))
        return float(a.value), float(b.value)

    @property
    def count_bytes(self) -> int:
        return int(self._lib.sa_devtext_count_bytes(self._h))

    def append(self, data):
        a = _as_u8(data)
        if self._lib.sa_devtext_append(self._h, _ptr(a), a.size) != 0:
            self._err("sa_devtext_append")

    def peek(self, off: int, n: int) -> bytes:
        out = np.empty(n, np.uint8)
        if self._lib.sa_devtext_peek(self._h, off, _ptr(out), n) != 0:
            self._err("sa_devtext_peek")
        return out.tobytes()

    def cut(self, block_size: int, first, eof: bool = True, mate: "DevText | None" = None, mate_eof: bool | None = None,
            max_blocks: int = 4096) -> tuple[list[tuple[int, int]], int]:
        """sa_devtext_cut: ([(len1, len2)] of the blocks the unread text holds, CUT_*)."""
        f = _as_u8(first)
        l1 = np.zeros(max_blocks, np.uint64)
        l2 = np.zeros(max_blocks, np.uint64)
        end = C.c_int32(0)
        e2 = eof if mate_eof is None else mate_eof
        n = self._lib.sa_devtext_cut(self._h, 1 if eof else 0, mate._h if mate is not None else None, 1 if e2 else 0,
                                     block_size, _ptr(f), f.size, _ptr(l1), _ptr(l2), max_blocks, C.byref(end))
        if n < 0:
            self._err("sa_devtext_cut")
        return list(zip(l1[:n].astype(np.int64).tolist(), l2[:n].astype(np.int64).tolist())), int(end.value)

    def take(self, len1: int, mate: "DevText | None" = None, len2: int = 0) -> DevBlock:
        h = self._lib.sa_devtext_take(self._h, len1, mate._h if mate is not None else None, len2)
        if not h:
            self._err("sa_devtext_take")
        return DevBlock(h)


class GunzipState(C.Structure):
    """sa_gunzip_state: where a gzip stream stands between two sa_gunzip_run calls (zeros: a file's start)."""
    _fields_ = [("in_stream", C.c_uint32), ("bit", C.c_uint32), ("win_len", C.c_uint32), ("crc", C.c_uint32),
                ("len", C.c_uint64), ("ended", C.c_uint32), ("reserved", C.c_uint32), ("window", C.c_uint8 * 32768)]


class GunzipInfo(C.Structure):
    """sa_gunzip_info: what one sa_gunzip_run call did."""
    _fields_ = [("chunks", C.c_uint32), ("candidates", C.c_uint32), ("waves_confirmed", C.c_uint32),
                ("false_skipped", C.c_uint32), ("members_ended", C.c_uint32), ("end_wave", C.c_uint32),
                ("end_why", C.c_uint32), ("status", C.c_uint32), ("find_ms", C.c_float), ("spec_ms", C.c_float),
                ("chain_ms", C.c_float), ("resolve_ms", C.c_float), ("crc_ms", C.c_float)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class Gunzipper:
    """Ordinary gzip (gzip, pigz, concatenated members) inflated on the device by
    speculation (sa_gunzipper_*): a wave per chunk of compressed bytes, the
    members' CRC-32 and ISIZE checked.  Its device slabs grow on demand and are kept."""

    SLAB = 32 << 20   # compressed bytes fed per call

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = self._lib.sa_gunzipper_create(device)
        if not self._h:
            raise SeqArcError(f"sa_gunzipper_create failed: no usable gfx950 device {device}")
        self.last_info: dict = {}
        self.calls: list[dict] = []   # the info of every call of the last gunzip()

    def close(self):
        if self._h:
            self._lib.sa_gunzipper_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def last_kernel_ms(self) -> float:
        return float(self._lib.sa_gunzipper_kernel_ms(self._h))

    @property
    def grid(self) -> int:
        """(tests and diagnostics) Workgroups a launch uses at most (SA_GUNZIP_GRID)."""
        return int(self._lib.sa_gunzipper_grid(self._h))

    @property
    def chunk(self) -> int:
        """Compressed bytes per chunk (SA_GUNZIP_CHUNK)."""
        return int(self._lib.sa_gunzipper_chunk(self._h))

    def run(self, data, state: GunzipState, out: np.ndarray, eof: bool = True, out_cap: int | None = None):
        """One sa_gunzip_run into the uint8 array `out`: (return value, out_bytes, in_used);
        `state` is updated and .last_info set.  A negative return value raises."""
        a = _as_u8(data)
        ob, used, info = C.c_uint64(0), C.c_uint64(0), GunzipInfo()
        rc = self._lib.sa_gunzip_run(self._h, _ptr(a), a.size, int(eof), C.byref(state), _ptr(out),
                                     out.size if out_cap is None else out_cap, C.byref(ob), C.byref(used), C.byref(info))
        self.last_info = info.as_dict()
        if rc < 0:
            raise SeqArcError(f"sa_gunzip_run ({rc}): {self._lib.sa_gunzipper_error(self._h).decode()}")
        return rc, ob.value, used.value

    def gunzip(self, data, slab: int | None = None, out_cap: int | None = None) -> bytes:
        """A whole gzip file's text: sa_gunzip_run over slabs of `slab` compressed
        bytes, what a call leaves unconsumed carried into the next.  Raises on a
        corrupt stream, and where the device path would hand the stream to the
        host (a call of two chunks or more that confirms less than one)."""
        a = _as_u8(data)
        slab = slab or self.SLAB
        cap = out_cap or max(64 << 20, 16 * slab)
        out = np.empty(cap, np.uint8)
        state = GunzipState()
        parts, at, carry = [], 0, np.zeros(0, np.uint8)
        self.calls = []
        while True:
            take = min(slab, a.size - at)
            buf = np.concatenate([carry, a[at:at + take]]) if carry.size else a[at:at + take]
            at += take
            eof = at == a.size
            rc, ob, used = self.run(buf, state, out, eof)
            self.calls.append(self.last_info)
            parts.append(out[:ob].tobytes())
            if rc > 0:
                raise SeqArcError(f"gzip stream is corrupt: status {rc} ({INFLATE_STATUS.get(rc, '?')}) after "
                                  f"{sum(map(len, parts))} text bytes")
            carry = buf[used:]
            if state.ended or (eof and carry.size == 0):
                break
            if (self.last_info["chunks"] >= 2 and used < self.chunk) or (eof and not used and not ob):
                raise SeqArcError(f"the device path makes too little progress (end_why {self.last_info['end_why']}): "
                                  "inflate this stream on the host")
        return b"".join(parts)

    def run_to(self, devtext: "DevText", data, state: GunzipState, eof: bool = True, out_cap: int | None = None):
        """One sa_gunzip_run_dev: the confirmed prefix's text appended to the devtext,
        never on the host; (return value, text_bytes, in_used).  out_cap (default: the
        devtext's room) is the most text the call may append; -3: it exceeds devtext.room
        (nothing done).  Any other negative return value raises."""
        a = _as_u8(data)
        tb, used, info = C.c_uint64(0), C.c_uint64(0), GunzipInfo()
        rc = self._lib.sa_gunzip_run_dev(self._h, _ptr(a), a.size, int(eof), C.byref(state), devtext._h,
                                         devtext.room if out_cap is None else out_cap, C.byref(tb), C.byref(used),
                                         C.byref(info))
        self.last_info = info.as_dict()
        if rc < 0 and rc != -3:
            raise SeqArcError(f"sa_gunzip_run_dev ({rc}): {self._lib.sa_gunzipper_error(self._h).decode()}")
        return rc, tb.value, used.value

    def gunzip_to(self, devtext: "DevText", data, slab: int | None = None, out_cap: int | None = None) -> int:
        """A whole gzip file's text appended to the devtext: gunzip()'s loop over
        sa_gunzip_run_dev, each call with the devtext's room (at most out_cap) for its
        text.  Returns the text bytes appended; raises where gunzip() raises, and when
        the devtext has no room left."""
        a = _as_u8(data)
        slab = slab or self.SLAB
        state = GunzipState()
        total, at, carry = 0, 0, np.zeros(0, np.uint8)
        self.calls = []
        while True:
            take = min(slab, a.size - at)
            buf = np.concatenate([carry, a[at:at + take]]) if carry.size else a[at:at + take]
            at += take
            eof = at == a.size
            rc, tb, used = self.run_to(devtext, buf, state, eof, min(out_cap or devtext.room, devtext.room))
            self.calls.append(self.last_info)
            total += tb
            if rc > 0:
                raise SeqArcError(f"gzip stream is corrupt: status {rc} ({INFLATE_STATUS.get(rc, '?')}) after "
                                  f"{total} text bytes")
            carry = buf[used:]
            if state.ended or (eof and carry.size == 0):
                break
            if (self.last_info["chunks"] >= 2 and used < self.chunk) or (eof and not used and not tb):
                raise SeqArcError(f"the device path makes too little progress (end_why {self.last_info['end_why']}): "
                                  "inflate this stream on the host")
        return total


class Input:
    """A batch of blocks resident in HBM (sa_input_create): uploaded once, encoded
    by any Encoder of the same device, concurrently from several host threads."""

    def __init__(self, blocks: list[Block], device: int = 0):
        self._lib = load_library()
        self.blocks = list(blocks)
        arr = (_SaBlock * max(1, len(blocks)))(*[b._c() for b in blocks])
        self._h = self._lib.sa_input_create(device, arr, len(blocks))
        if not self._h:
            raise SeqArcError(f"sa_input_create failed on device {device}")
        self.text_bytes = sum(b.text_bytes for b in blocks)

    def close(self):
        if self._h:
            self._lib.sa_input_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bare_plus(text) -> int:
    """1 if the first record's '+' line carries no ID (getFirstLine@0x431eb0)."""
    t = _as_u8(text)
    nl = np.flatnonzero(t[: 1 << 16] == 10)[:3]
    if nl.size < 3:
        return 1
    return 0 if int(nl[2]) - int(nl[1]) > 2 else 1


def arc_archive(encaps: list[bytes], blocks: list[Block], file1: str, file2: str | None = None,
                template: np.ndarray | None = None, cfg: Config | None = None, gz1: bool = False,
                plus_bare: int = 1, ref_md5: bytes | None = None, insert_size: int = 0, maxmis: int = 7) -> bytes:
    """The .arc file around encoded blocks (header, blocks in input order, trailer):
    SeqArcFile::writeFileInfo@0x4171b0 / writeParam@0x416450 / writeBlockLenArry (arc_file.cpp)."""
    lib = load_library()
    cfg = cfg or Config()
    recs = (_SaArcBlock * max(1, len(encaps)))()
    for i, (e, b) in enumerate(zip(encaps, blocks)):
        lng = 1 if b.nreads and int(b.seq_lens.max()) > 0xffff else 0
        recs[i] = _SaArcBlock(len(e), lng, b.text1 or b.text_bytes, b.text2)
    tmpl = np.zeros(512, np.uint8) if template is None else np.ascontiguousarray(template, dtype=np.uint8)
    rm = None if ref_md5 is None else np.frombuffer(ref_md5, np.uint8)
    info = _SaArcInfo(file1.encode(), (file2 or "").encode(), 1 if file2 else 0, 1 if gz1 else 0, int(plus_bare),
                      1 if cfg.md5 else 0, 1 if cfg.lossy > 0 else 0, _ptr(tmpl), None if rm is None else _ptr(rm),
                      int(insert_size))
    cap = 4096 + 40 * len(encaps)
    tr = np.empty(cap, np.uint8)
    n = lib.sa_arc_trailer2(C.byref(info), int(maxmis), recs, len(encaps), _ptr(tr), cap)
    if n < 0:
        raise SeqArcError("sa_arc_trailer failed")
    hdr = np.zeros(16, np.uint8)
    lib.sa_arc_header(sum(map(len, encaps)), _ptr(hdr))
    return hdr.tobytes() + b"".join(encaps) + tr[:n].tobytes()


def hash_file_genome(hash_file: bytes) -> tuple[np.ndarray, int]:
    """(packed genome words, bases) of a `.hash` file (HashRefIndex32 layout:
    K, bases, words, positions, then the words)."""
    K, bases, nwords, npos = np.frombuffer(hash_file[:16], np.uint32)
    return np.frombuffer(hash_file, np.uint32, count=int(nwords), offset=16).copy(), int(bases)


def decode_block(data: bytes, text_bytes: int, cfg: Config | None = None, template: np.ndarray | None = None,
                 long_reads: bool = False, ref: tuple | None = None) -> tuple[Block, bool]:
    """Host decode of one encoded block (sa_decode_block; doFqzDecode@0x42c680):
    (the block's reads, stored MD5s match).  text_bytes bounds the arrays
    (the block's FASTQ size, from the archive's block table).  ref = (genome
    words, bases, paired, maxmis[, insert_size]): a block of the reference path."""
    lib = load_library()
    cfg = cfg or Config()
    cap = int(text_bytes) + 64
    names, seq, qual = (np.empty(cap, np.uint8) for _ in range(3))
    mr = cap // 4 + 8
    nl, sl = np.empty(mr, np.uint16), np.empty(mr, np.int32)
    d = _SaDecoded(_ptr(names), _ptr(nl), _ptr(seq), _ptr(sl), _ptr(qual), cap, cap, mr, 0, 0)
    src = np.frombuffer(data, np.uint8)
    tmpl = np.zeros(512, np.uint8) if template is None else np.ascontiguousarray(template, dtype=np.uint8)
    c = cfg._c()
    if ref is None:
        n = lib.sa_decode_block(_ptr(src), src.size, C.byref(c), _ptr(tmpl), 1 if long_reads else 0, C.byref(d))
    else:
        words = np.ascontiguousarray(ref[0], dtype=np.uint32)
        r = _SaRef(_ptr(words), int(ref[1]), 1 if ref[2] else 0, int(ref[3]), int(ref[4]) if len(ref) > 4 else 0)
        n = lib.sa_decode_block_ref(_ptr(src), src.size, C.byref(c), _ptr(tmpl), 1 if long_reads else 0, C.byref(r),
                                    C.byref(d))
    if n < 0:
        raise SeqArcError("sa_decode_block: malformed block")
    n = int(n)
    ln, ls = int(nl[:n].astype(np.int64).sum()), int(sl[:n].astype(np.int64).sum())
    return Block(names[:ln].copy(), nl[:n].copy(), seq[:ls].copy(), sl[:n].copy(), qual[:ls].copy(), text_bytes), \
        bool(d.md5_ok)


class DecodeInfo(C.Structure):
    """sa_decode_info: what the last sa_decode_blocks call did."""
    _fields_ = [("groups", C.c_uint32), ("inflight", C.c_uint32), ("slice", C.c_uint32), ("qual_launches", C.c_uint32),
                ("seq_launches", C.c_uint32), ("unsupported", C.c_uint32), ("init_ms", C.c_float), ("qual_ms", C.c_float),
                ("place_ms", C.c_float), ("seq_ms", C.c_float), ("h2d_ms", C.c_float), ("d2h_ms", C.c_float)]


# why a block's decode ended (SA_DEC_* of include/seqarc_amd.h)
DEC_OK, DEC_LAYOUT, DEC_INPUT, DEC_SLOT, DEC_RANGE, DEC_PLACE, DEC_UNSUPPORTED, DEC_STUCK = range(8)


class Decoder:
    """Blocks of a no-reference, lossless archive decoded on the device
    (sa_decoder_*): a wave per block and chain, in a number of launches fixed
    from the blocks' symbol counts.  SA_DEC_SLICE and SA_DEC_INFLIGHT are read
    when the Decoder is made.  Its device and page-locked buffers are kept."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = self._lib.sa_decoder_create(device)
        if not self._h:
            raise SeqArcError(f"sa_decoder_create failed: no usable gfx950 device {device}")

    def close(self):
        if self._h:
            self._lib.sa_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = DecodeInfo()
        self._lib.sa_decoder_info(self._h, C.byref(i))
        return {n: getattr(i, n) for n, _ in i._fields_}

    def decode(self, blocks, caps, cfg: Config | None = None, template: np.ndarray | None = None, long_reads=None,
               threads: int = 4) -> list[tuple]:
        """One sa_decode_blocks over the encoded blocks (bytes); caps[i] bounds block i's
        arrays as decode_block's text_bytes does.  Per block (Block | None, md5_ok, status):
        the Block is None where the status (DEC_*) is not 0."""
        n = len(blocks)
        cfg = cfg or Config()
        tmpl = np.zeros(512, np.uint8) if template is None else np.ascontiguousarray(template, dtype=np.uint8)
        srcs = [np.frombuffer(b, np.uint8) for b in blocks]
        ins = (C.c_void_p * max(1, n))(*[_ptr(s) for s in srcs])
        lens = np.array([s.size for s in srcs], np.uint64)
        lng = np.array([1 if (long_reads is not None and long_reads[i]) else 0 for i in range(n)], np.int32)
        outs = (_SaDecoded * max(1, n))()
        keep = []
        for i in range(n):
            cap = int(caps[i]) + 64
            mr = cap // 4 + 8
            a = (np.empty(cap, np.uint8), np.empty(mr, np.uint16), np.empty(cap, np.uint8), np.empty(mr, np.int32),
                 np.empty(cap, np.uint8))
            keep.append(a)
            outs[i] = _SaDecoded(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(a[4]), cap, cap, mr, 0, 0)
        status = np.zeros(max(1, n), np.uint32)
        c = cfg._c()
        rc = self._lib.sa_decode_blocks(self._h, ins, _ptr(lens), _ptr(lng), n, C.byref(c), _ptr(tmpl), int(threads), outs,
                                        _ptr(status))
        if rc < 0:
            raise SeqArcError(f"sa_decode_blocks ({rc}): {self._lib.sa_decoder_error(self._h).decode()}")
        res = []
        for i in range(n):
            st = int(status[i])
            if st:
                res.append((None, False, st))
                continue
            names, nl, seq, sl, qual = keep[i]
            k = int(outs[i].nreads)
            ln, ls = int(nl[:k].astype(np.int64).sum()), int(sl[:k].astype(np.int64).sum())
            res.append((Block(names[:ln].copy(), nl[:k].copy(), seq[:ls].copy(), sl[:k].copy(), qual[:ls].copy(), int(caps[i])),
                        bool(outs[i].md5_ok), 0))
        return res


class AlignChain:
    """The align_info state an encode thread carries from read to read and block
    to block on the reference path (sa_align_chain): one per input, batches
    pass through it in order.  nmis: the states before the first read (0 for
    a fresh encode thread's AlignParam)."""

    def __init__(self, nmis_mate1: int = 0, nmis_mate2: int = 0):
        self._lib = load_library()
        self._h = self._lib.sa_align_chain_create(nmis_mate1, nmis_mate2)

    def close(self):
        if self._h:
            self._lib.sa_align_chain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HashIndex:
    """The HASH reference index of a FASTA (`SeqArc -i ref.fa`,
    buildRefIndex@0x410190), built and kept on an Encoder's device
    (sa_hash_build), and the gapless seed alignment of reads against it
    (sa_hash_align, getHashAlignInfo@0x4113c0)."""

    K, STEP, MAXCOUNT, MAXMIS, GOOD = 14, 2, 1 << 16, 7, 1   # SeqArcParam ctor @0x407490

    def __init__(self, enc: "Encoder", fasta: bytes | None, k: int = K, step: int = STEP, maxcount: int = MAXCOUNT,
                 hash_file: bytes | None = None):
        """From the FASTA (built on the device) or from its `.hash` file (hash_file)."""
        self._enc, self._lib = enc, enc._lib
        if hash_file is not None:
            f = np.frombuffer(hash_file, np.uint8)
            self._h = self._lib.sa_hash_load(enc._ctx, _ptr(f), f.size)
            if not self._h:
                enc._err("sa_hash_load")
            return
        if isinstance(fasta, np.ndarray):   # (a genome-scale FASTA as a uint8 array: no bytes copy)
            self._h = self._lib.sa_hash_build(enc._ctx, _ptr(fasta), fasta.size, k, step, maxcount)
        else:
            self._h = self._lib.sa_hash_build(enc._ctx, fasta, len(fasta), k, step, maxcount)
        if not self._h:
            enc._err("sa_hash_build")

    def close(self):
        if self._h:
            self._lib.sa_hash_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def genome_length(self) -> int:
        return int(self._lib.sa_hash_genome_length(self._h))

    def file_bytes(self) -> bytes:
        """The `<ref.fa>.hash` file (HashRefIndex32::writeIndexFile@0x41ed00)."""
        return self.file_array().tobytes()

    def file_array(self) -> np.ndarray:
        """file_bytes() as a uint8 array."""
        n = int(self._lib.sa_hash_file_bytes(self._h))
        out = np.empty(n, dtype=np.uint8)
        if self._lib.sa_hash_serialize(self._enc._ctx, self._h, _ptr(out), n) != 0:
            self._enc._err("sa_hash_serialize")
        return out

    def packed(self) -> tuple[np.ndarray, int]:
        """(the genome's packed words, bases): what the aligned-read decoder
        reads (sa_hash_packed; HashAlignment::doGetSeq@0x40ff90)."""
        n = self.genome_length
        words = np.empty(max(1, (n + 15) // 16), np.uint32)
        if self._lib.sa_hash_packed(self._enc._ctx, self._h, _ptr(words), words.size) != 0:
            self._enc._err("sa_hash_packed")
        return words, n

    def align(self, reads: list[bytes], maxmis: int = MAXMIS, good: int = GOOD, ai_nmis: int = 0):
        """The reads in order, one align_info state carried across them
        (ai_nmis: before the first read; 0 = a zero-filled AlignParam).  Per
        read: ret (mismatches or -1), rev, pos (1-based), mispos and mistype
        ([n, maxmis + 1], -1 past the read's mismatches)."""
        n = len(reads)
        seq = np.frombuffer(b"".join(reads) or b"\0", dtype=np.uint8)
        lens = np.array([len(r) for r in reads] or [0], dtype=np.int32)
        off = np.zeros(max(n, 1), dtype=np.uint64)
        if n > 1:
            off[1:n] = np.cumsum(lens[:n - 1])
        return self.align_arrays(seq, off, lens, n, maxmis, good, ai_nmis)

    def align_arrays(self, seq: np.ndarray, off: np.ndarray, lens: np.ndarray, n: int, maxmis: int = MAXMIS,
                     good: int = GOOD, ai_nmis: int = 0):
        """align() over reads given as one uint8 array with uint64 offsets and
        int32 lengths (no per-read Python objects)."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        ret = np.zeros(max(n, 1), dtype=np.int32)
        rev = np.zeros(max(n, 1), dtype=np.uint8)
        pos = np.zeros(max(n, 1), dtype=np.uint64)
        mp = np.zeros((max(n, 1), maxmis + 1), dtype=np.int32)
        mt = np.zeros((max(n, 1), maxmis + 1), dtype=np.int32)
        st = np.array([ai_nmis], dtype=np.int32)
        if self._lib.sa_hash_align(self._enc._ctx, self._h, _ptr(seq), _ptr(off), _ptr(lens), n, maxmis, good,
                                   _ptr(st), _ptr(ret), _ptr(rev), _ptr(pos), _ptr(mp), _ptr(mt)) != 0:
            self._enc._err("sa_hash_align")
        self.last_kernel_ms = float(self._lib.sa_hash_align_kernel_ms(self._enc._ctx))
        return ret[:n], rev[:n], pos[:n], mp[:n], mt[:n]
