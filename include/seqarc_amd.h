/*
 * seqarc_amd.h -- C-ABI of the MI355X SeqArc block encoder (libseqarc_amd.so).
 *
 * Plain pointers and sizes only.  The reference (SeqArc-1.6) is one monolithic
 * executable with no plugin API; the seam this library replaces is the per-block
 * encoder call inside the encode thread:
 *
 *   int EncapFqzComp::doFqzEncode(SeqArcMemBuf*, DebugInfo*)   SeqArc-1.6@0x42d2d0
 *     called from ISeqArcEncodeThread::doTask                   SeqArc-1.6@0x433dd0
 *     after SeqArcMemBuf::calcBlockMd5@0x414d90 and DegeInfoProcess@0x433a10
 *
 * sa_encode_blocks() takes a batch of parsed blocks (the SeqArcMemBuf SoA:
 * IDs + u16 lengths, bases + i32 lengths, qualities; PE reads interleaved
 * r1,r2) and returns, per block, exactly the bytes doFqzEncode writes
 * ("81 <size4> ..." : count, len, ID, qual, dege streams, seq).
 *
 * Errors: a non-zero return and sa_last_error(); the reference abort()s on a
 * coder invariant violation -- here the batch fails and no output is produced.
 * Thread-safety: one sa_ctx per host thread / device; contexts are independent.
 */
#ifndef SEQARC_AMD_H
#define SEQARC_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_ctx sa_ctx;

/* One parsed block (SeqArcMemBuf fields +0x80/+0xc0, +0x88/+0xd0, +0x90, +0x4). */
typedef struct {
    const uint8_t *names;       /* concatenated IDs without '@'            */
    const uint16_t *name_lens;  /* nreads entries                           */
    const uint8_t *seq;         /* concatenated bases                       */
    const int32_t *seq_lens;    /* nreads entries                           */
    const uint8_t *qual;        /* concatenated quals (same lengths)        */
    uint32_t nreads;
} sa_block;

/* Encoder parameters (SeqArcParam fields of the no-reference path). */
typedef struct {
    int32_t slevel;    /* param+0x1b54 (default 3): seq order k = slevel + 7      */
    int32_t qlevel;    /* param+0x1b58 (default 2)                                */
    int32_t md5;       /* param+0x1880 (default 1): per-block MD5 of ID/seq/qual  */
    int32_t bin_mode;  /* param+0x18a4 (ID template byte 0, see sa_analyze_ids)   */
    double lossy;      /* -l R (param+0x1878; param+0x1870 set iff R > 0): R-Block
                          quality pre-pass rblock@0x426c10, no quality MD5; 0 = off */
} sa_cfg;

typedef struct {
    uint8_t *data;     /* caller-allocated, >= sa_output_bound() bytes  */
    uint64_t cap;
    uint64_t size;     /* written                                     */
} sa_out;

/* ---- lifecycle ------------------------------------------------------- */
sa_ctx *sa_create(int device);               /* NULL if no usable gfx950 device */
/* A context of the same device sharing `peer`'s front scratch: the contexts'
 * throughput-bound fronts (symbol extraction, sorts, short model runs) run one
 * at a time on it while each one's latency-bound range coder chains overlap the
 * next front (the pipeline of encoder lanes on one GPU). */
sa_ctx *sa_create_shared(int device, sa_ctx *peer);
void sa_destroy(sa_ctx *ctx);
const char *sa_last_error(const sa_ctx *ctx);
const char *sa_version(void);

/* ---- one-shot batch: replaces doFqzEncode@0x42d2d0 per block ---------- */
uint64_t sa_output_bound(const sa_block *blk);
/* page-locks host memory the caller hands to the encoder (block SoA buffers)
 * so that staging is a DMA instead of a pageable copy through the runtime's
 * bounce buffer (4.9 vs 56 GB/s H2D on MI355X); unregister before freeing it.
 * 0 on success.  (The reader/parser buffers of seqarc_amd -c.) */
int sa_host_register(void *p, uint64_t bytes);
int sa_host_unregister(void *p);
/* Batches above 3 Gi bases (env SA_BATCH_BASES lowers the cap) are encoded as
 * consecutive sub-batches; outputs keep the input order. */
int sa_encode_blocks(sa_ctx *ctx, const sa_block *in, int n, const sa_cfg *cfg, sa_out *out);

/* ---- staged API (inputs resident in HBM; used by bench.py) ------------ */
/* the batch size (blocks) the context's buffers are sized for from its first
 * batch on, when its first batches are smaller (a re-allocation synchronises
 * the device); 0: as each batch needs */
void sa_set_reserve(sa_ctx *ctx, uint32_t blocks);
/* device buffer re-allocations in this process so far (each one's hipFree
 * synchronises the device) and the host time spent allocating, in ms */
void sa_alloc_stats(uint32_t *grows, double *alloc_ms);
int sa_stage(sa_ctx *ctx, const sa_block *in, int n);     /* H2D copy of a batch   */
/* FASTQ text of one block as the reader cut it (doReadPEJob@0x432d10 /
 * cultPEbuf@0x432180 hand these to getBlockRead[PE]): file 1 and, for PE,
 * file 2 (text2 = NULL: single-end). */
typedef struct sa_text_block {
    const uint8_t *text1;
    uint64_t len1;
    const uint8_t *text2;
    uint64_t len2;
} sa_text_block;
typedef struct sa_text_info {   /* per block, written by sa_stage_text */
    uint32_t nreads;
    uint32_t len_long;          /* a read > 65535 bp (SeqArcMemBuf+0x2)     */
    uint64_t name_bytes;
    uint64_t seq_bytes;
    uint64_t out_bound;         /* sa_output_bound of the parsed block      */
} sa_text_info;
/* Stages a batch given as FASTQ text: the texts are copied to HBM (a DMA when
 * they are in sa_host_alloc memory) and parsed there into the batch sa_stage
 * would upload -- getBlockRead@0x411b60 (SE) / getBlockReadPE@0x412920 (PE),
 * byte for byte the blocks sa_parse_se / sa_parse_pe give.  info (optional, n
 * entries) gets each block's counts.  Then sa_run / sa_fetch.  -1 and
 * sa_last_error where sa_parse_* fail.  The texts may be reused on return. */
int sa_stage_text(sa_ctx *ctx, const sa_text_block *in, int n, sa_text_info *info);
/* page-locked host memory for the reader's text windows (2 MiB-aligned, huge pages
 * asked for, registered portable with the runtime); free with sa_host_free */
void *sa_host_alloc(uint64_t bytes);
void sa_host_free(void *p);
int sa_run(sa_ctx *ctx, const sa_cfg *cfg);                /* encode the staged batch */
int sa_fetch(sa_ctx *ctx, sa_out *out, int n);             /* D2H of the encaps     */
/* the encoded size of each of the last run's n blocks (what sa_fetch will
 * copy), so a caller can size its output buffers before the fetch instead of
 * reserving sa_output_bound for every block; -1 on a count mismatch */
int sa_fetch_sizes(const sa_ctx *ctx, uint64_t *sizes, int n);
/* per-phase device time (ms) of the last sa_run, measured with HIP events on
 * the stream each phase runs on; returns the number of phases written */
int sa_phase_times(const sa_ctx *ctx, const char **names, float *ms, int max);
void sa_set_timing(sa_ctx *ctx, int on);
/* HBM bytes the context's work buffers hold (they grow to the largest batch) */
uint64_t sa_device_bytes(const sa_ctx *ctx);
/* HBM bytes of the (possibly shared) front scratch */
uint64_t sa_front_bytes(const sa_ctx *ctx);

/* ---- resident inputs: a batch uploaded once, encoded by any context ----
 * The reference keeps a pool of parsed blocks between its reader and its
 * encode threads (ReadBufPool::getEmptybuf/getFullbuf@0x4341e0/0x4343d0); an
 * sa_input is such a batch resident in HBM.  Several contexts of one device
 * (one host thread each) encode their batches concurrently: one batch's
 * throughput-bound front overlaps another's latency-bound range coder. */
typedef struct sa_input sa_input;
sa_input *sa_input_create(int device, const sa_block *in, int n);   /* NULL on error */
void sa_input_destroy(sa_input *in);
int sa_run_input(sa_ctx *ctx, const sa_input *in, const sa_cfg *cfg);   /* then sa_fetch */
/* an empty input of a device, filled by sa_stage_text_input: FASTQ text staged
 * and parsed on the device with ctx's stream (ctx may be another context than
 * the one that later runs the input: the command line stages a context's next
 * batch while the context encodes the current one) */
sa_input *sa_input_empty(int device);
int sa_stage_text_input(sa_ctx *ctx, sa_input *in, const sa_text_block *blocks, int n, sa_text_info *info);
/* Streaming form of sa_stage_text (round 6): the reader hands each block's text
 * over as it cuts it (doReadPEJob@0x432d10 / ReadBufPool::addFullbuf@0x434900),
 * and its bytes go to the device at once, so the reader's buffer is free again
 * before the rest of the batch is cut.  in = NULL: the context's own input.
 * Each input has two text arenas (slot 0 / 1): a thread of its own may fill one
 * while the context encodes the batch parsed from the other.  Block `index` of
 * a batch of at most nmax blocks lands at 2 x index x stride (file 1) and
 * (2 x index + 1) x stride (file 2); stride >= every text length (the reader's
 * window).  Block 0 of a batch first.  Returns once the copy is done. */
int sa_text_upload(sa_ctx *ctx, sa_input *in, int slot, int index, int nmax, const sa_text_block *blk,
                   uint64_t stride);
/* Parses the n blocks uploaded into arena `slot` (lens: their lengths; text2
 * non-NULL for PE) into the input, byte for byte what sa_stage_text gives.
 * The input must not be in use (its previous sa_run* returned). */
int sa_text_parse(sa_ctx *ctx, sa_input *in, int slot, const sa_text_block *lens, int n, uint64_t stride,
                  sa_text_info *info);

/* ---- range coder over pre-modelled symbols ---------------------------- */
/* The carry-less range coder inlined in every EncapFqzComp::encode_* (e.g.
 * encode_seq@0x422010-0x422085, finish @0x424a1c), applied to nstreams streams
 * of (cum, freq, tot) triples laid out back to back (stream s has lens[s]
 * symbols).  Writes the streams' coded bytes back to back into out and their
 * lengths into out_lens.  Rejects cum + freq > tot (the reference abort()s). */
int sa_code_records(sa_ctx *ctx, int nstreams, const uint32_t *lens, const uint16_t *cum,
                    const uint16_t *freq, const uint16_t *tot, uint8_t *out, uint64_t out_cap,
                    uint64_t *out_lens);
/* streams restarted after a carry-less squeeze in the last sa_run / sa_code_records */
uint32_t sa_coder_restarts(const sa_ctx *ctx);
/* symbols of the longest coder stream and of all streams in the last sa_run
 * (the serial range chain of the longest stream bounds the batch) */
void sa_stream_stats(const sa_ctx *ctx, uint64_t *max_symbols, uint64_t *total_symbols);

/* ---- path report ------------------------------------------------------ */
/* Which kernels the host chose for the context's last sa_run / sa_run_input /
 * sa_encode_blocks (its last sub-batch) / sa_code_records: filled where the
 * launches are chosen, read-only, no device work.  The tests assert from it
 * that an SA_* knob or a batch shape selected the path they mean to check.
 * Fields of a stage that did not run are 0. */
typedef struct {
    uint32_t prep;            /* SA_PATH_PREP_*                                        */
    uint32_t front_counter;   /* 1: front reads taken from a counter, 0: static stride */
    uint32_t wg_per_cu;       /* workgroups per CU of the grid-stride front kernels    */
    uint32_t emit;            /* SA_PATH_EMIT_*                                        */
    uint32_t dege_list;       /* 1: k_dege_list + the listed k_emit_sq ran             */
    uint32_t seq_packed;      /* 1: SEQ keys ctx << 2 | base, implicit values          */
    uint32_t seq_replay;      /* SA_PATH_SEQ_*                                         */
    uint32_t bkt_inv;         /* bucket: 1 inverse permutation, 0 scattered stores     */
    uint32_t bkt_lpt;         /* bucket: 1 largest digits first, 0 digit order         */
    uint32_t bkt_db;          /* bucket: the digit bits used                           */
    uint32_t bkt_sb;          /* bucket: the context bits a wave holds in LDS          */
    uint32_t aux_sort;        /* SA_PATH_AUX_*                                         */
    uint32_t aux_runs;        /* SA_PATH_RUNS_*                                        */
    uint32_t aux_nmod_max;    /* dense: the largest per-block model count read back    */
    uint32_t aux_dense_next;  /* the context's dense flag after the batch              */
    uint32_t pass_r;          /* SA_PATH_R_*                                           */
    uint32_t r_short_shared;  /* 1: the short chains shared waves                      */
    uint32_t r_waves;         /* pass-R waves per workgroup                            */
    uint32_t l_chunk;         /* records per L-pass chunk: 16 or 32                    */
    uint32_t l_stream;        /* 1: the L passes on a stream of their own              */
    uint32_t host_waits;      /* 1: host-side waits between the context's streams      */
    uint32_t long_grid;       /* k_replay_aux_long workgroups                          */
    uint32_t chain_prio;      /* 1: the chain kernels raise their issue priority       */
    uint32_t md5;             /* 0: none, 1: k_md5_lanes, 2: k_md5<true>, 3: k_md5<false> */
    uint32_t rblock;          /* 1: the R-Block pre-pass ran                           */
    uint32_t rb_spec_counter; /* 1: k_rb_spec's chunks from a counter, 0: one grid     */
    uint32_t rb_fix_wave;     /* 1: k_rb_fix_w, 0: k_rb_fix                            */
    uint32_t rb_apply_walk;   /* 1: k_rb_apply, 0: k_rb_true + k_rb_fill               */
    uint32_t rb_chunk;        /* the R-Block chunk length                              */
    uint32_t exact_rerun;     /* 1: the exact-payload fallback re-ran the batch        */
    uint32_t seq_digits;      /* the SEQ sort's digit widths, 4 bits a pass, first low */
    uint32_t aux_digits;      /* the AUX sort's, likewise                              */
    uint32_t front_masked;    /* 1: the front's stream CU-masked (SA_RV_CUS)           */
} sa_paths;
enum { SA_PATH_PREP_ROW16 = 1, SA_PATH_PREP_ROW64 = 2, SA_PATH_PREP_FUSED = 3, SA_PATH_PREP_WAVE = 4 };
enum { SA_PATH_EMIT_ROW16 = 1, SA_PATH_EMIT_WAVE = 2 };
enum { SA_PATH_SEQ_BUCKET = 1, SA_PATH_SEQ_FULL = 2 };
enum { SA_PATH_AUX_DENSE1 = 1, SA_PATH_AUX_DENSE2_COPY = 2, SA_PATH_AUX_RAW = 3 };
enum { SA_PATH_RUNS_DENSE = 1, SA_PATH_RUNS_FIND = 2 };
enum { SA_PATH_R_V0 = 1, SA_PATH_R_V5 = 2, SA_PATH_R_V6 = 3, SA_PATH_R_LANES = 4 };
/* copies the report into *out; -1 without a context or out */
int sa_last_paths(const sa_ctx *ctx, sa_paths *out);

/* ---- host-side mirrors of the reference's block plumbing -------------- */
/* Block cut: SeqArcRead::doReadJob@0x432a80 / cultbuf@0x432530 / getEndPos@0x4320c0
 * (SE) and doReadPEJob@0x432d10 / cultPEbuf@0x432180 (PE).  Returns #blocks. */
int64_t sa_cut_se(const uint8_t *text, uint64_t len, uint64_t block_size,
                  uint64_t *ends, uint64_t max_blocks);
int64_t sa_cut_pe(const uint8_t *t1, uint64_t len1, const uint8_t *t2, uint64_t len2,
                  uint64_t block_size, uint64_t *ends1, uint64_t *ends2, uint64_t max_blocks);
/* Streaming forms (the reader thread's view, doReadJob / doReadPEJob): the end of
 * the next block in a window of the input that starts at a block boundary.
 * first/flen: the input's first line, '\n' included (getFirstLine@0x431eb0);
 * eof: the window holds the rest of that input.  SE: returns the block's
 * bytes, or -1 when the window is too short (read more) or no cut exists.  PE:
 * 0 and the block's bytes of each file in end1/end2, or -1 likewise. */
int64_t sa_cut_next_se(const uint8_t *win, uint64_t avail, int eof, uint64_t block_size,
                       const uint8_t *first, uint64_t flen);
int sa_cut_next_pe(const uint8_t *w1, uint64_t avail1, int eof1, const uint8_t *w2, uint64_t avail2, int eof2,
                   uint64_t block_size, const uint8_t *first, uint64_t flen, uint64_t *end1, uint64_t *end2);
/* sa_cut_next_pe with the newline counts of both windows given: k1 / k2 =
 * newlines in the first min(avail, block_size / 2) bytes of each window (the
 * command line's reader threads count them as they read the input). */
int sa_cut_next_pe_nl(const uint8_t *w1, uint64_t avail1, int eof1, uint64_t k1, const uint8_t *w2,
                      uint64_t avail2, int eof2, uint64_t k2, uint64_t block_size, const uint8_t *first,
                      uint64_t flen, uint64_t *end1, uint64_t *end2);
/* Block parse: getBlockRead@0x411b60 (SE) / getBlockReadPE@0x412920 (PE).
 * Output arrays sized >= text bytes (names/seq/qual) and text/4+1 (lens). */
int64_t sa_parse_se(const uint8_t *text, uint64_t len, uint8_t *names, uint16_t *name_lens,
                    uint8_t *seq, int32_t *seq_lens, uint8_t *qual);
int64_t sa_parse_pe(const uint8_t *t1, uint64_t len1, const uint8_t *t2, uint64_t len2,
                    uint8_t *names, uint16_t *name_lens, uint8_t *seq, int32_t *seq_lens,
                    uint8_t *qual);
/* ID template ("adaptive binning") detection on the first block:
 * IDProcess::analysisIDBinType@0x4310a0.  tmpl = the 512-byte param+0x18a4
 * area, caller zero-initialised; tmpl[0] is sa_cfg.bin_mode. */
int sa_analyze_ids(const sa_block *first, int single_end, uint8_t tmpl[512]);

/* ---- .arc container (SeqArcFile, host) ---------------------------------- */
/* Archive = 16-byte header + the encoded blocks back to back (input order,
 * the reference's -t 1 order) + trailer.  Restated from
 * SeqArcFile::writeFileInfo@0x4171b0, writeParam@0x416450 and
 * writeBlockLenArry{SE,PE}@0x416d60/0x416e90 (fastqueeze_amd/csrc/arc_file.cpp). */
typedef struct {
    uint32_t size;         /* encoded block bytes (sa_out.size of the block)           */
    uint32_t long_reads;   /* a read > 65535 bp (SeqArcMemBuf+0x2; compressLen_long)   */
    uint64_t text1;        /* FASTQ text bytes of the block in input 1 (ReadBuf+0xc)   */
    uint64_t text2;        /* ... in input 2 (ReadBuf+0x10; 0 for single-end)          */
} sa_arc_block;

typedef struct {
    const char *file1;             /* input paths as given (basename stored, ".gz" cut) */
    const char *file2;             /* NULL / "" for single-end                          */
    int32_t paired;
    int32_t gz1;                   /* param+0x6: input 1 is gzip (getFileType@0x40d9f0)  */
    int32_t bare_plus;             /* '+' lines carry no ID (getFirstLine@0x431eb0)      */
    int32_t md5;                   /* param+0x1880                                       */
    int32_t lossy;                 /* param+0x1870 (-l)                                  */
    const uint8_t *id_template;    /* 512 B, param+0x18a4 (sa_analyze_ids)               */
    /* reference path (-c ref.fa): param+0x3 clear, -I in field 10, and the
     * index MD5 encap writeMd5@0x416b10 (ID 8: the 16 bytes of "<ref.fa>.md5",
     * the MD5 of the FASTA file, getMd5@0x416810) */
    const uint8_t *ref_md5;        /* NULL: no reference                                 */
    uint32_t insert_size;          /* param+0x28 (-I)                                    */
} sa_arc_info;   /* (layout unchanged since round 1: maxmis is sa_arc_trailer2's argument) */

/* ---- block decoder (SeqArc -d; host) ------------------------------------ */
/* The inverse of sa_encode_blocks for one block: EncapFqzComp::doFqzDecode@0x42c680
 * and, in ID-bin mode, IDProcess::decodeIDS@0x430610 (fastqueeze_amd/csrc/arc_decode.cpp).
 * Caller-owned arrays; PE reads come back interleaved r1, r2. */
typedef struct {
    uint8_t *names;        /* >= name_cap bytes     */
    uint16_t *name_lens;   /* >= max_reads entries  */
    uint8_t *seq;          /* >= seq_cap bytes      */
    int32_t *seq_lens;     /* >= max_reads entries  */
    uint8_t *qual;         /* >= seq_cap bytes      */
    uint64_t name_cap, seq_cap;
    uint32_t max_reads;
    uint32_t nreads;       /* out */
    int32_t md5_ok;        /* out: stored digests match (blockMd5Verify@0x414e00), 1 if MD5 off */
} sa_decoded;
/* Returns nreads, or -1 on a malformed block / too small arrays.  tmpl: the
 * archive's 512-byte ID template (trailer field 15); long_reads: the block
 * record's flag bit (compressLen_long). */
int64_t sa_decode_block(const uint8_t *in, uint64_t len, const sa_cfg *cfg, const uint8_t tmpl[512],
                        int32_t long_reads, sa_decoded *out);

/* The reference path's blocks (doAlignEncode@0x42d4c0 layout): aligned reads are
 * rebuilt from the genome (EncapFqzComp::decompressSeq@0x42e390 ->
 * getRealPos@0x42de30, AlignInfoToSeq@0x42e020). */
typedef struct {
    const uint32_t *genome;   /* packed bases: sa_hash_packed / the .hash file's words */
    uint64_t bases;           /* genome length (param+0x1868)                          */
    int32_t paired;           /* the archive is PE (the mate relation streams)         */
    int32_t maxmis;           /* param+0x1b60 the archive was made with (Mis model)    */
    uint32_t insert_size;     /* -I (trailer field 10): the mate distances' bits when  */
                              /* the block's insert-bits count is 0 (the reference's   */
                              /* own decoder reads 0 bits there)                       */
} sa_ref;
int64_t sa_decode_block_ref(const uint8_t *in, uint64_t len, const sa_cfg *cfg, const uint8_t tmpl[512],
                            int32_t long_reads, const sa_ref *ref, sa_decoded *out);

/* ---- block decoder on the device (no-reference, lossless archives) --------- */
/* Why a block's decode ended (fastqueeze_amd/csrc/sa_decode_logic.h, sa_decoder.h). */
enum {
    SA_DEC_OK = 0,
    SA_DEC_LAYOUT = 1,       /* the encap walk or one of the small streams failed, or the arrays are too small */
    SA_DEC_INPUT = 2,        /* a chain read past its payload */
    SA_DEC_SLOT = 3,         /* the coder's slot is not below the model's total */
    SA_DEC_RANGE = 4,        /* range 0 after a carry-less squeeze (the renormalisation is bounded) */
    SA_DEC_PLACE = 5,        /* the side streams disagree with each other or with the qualities */
    SA_DEC_UNSUPPORTED = 6,  /* not decoded on the device: -l blocks, a block beyond the memory budget */
    SA_DEC_STUCK = 7         /* a chain had not ended after the launches its symbol count allows */
};
/* Many blocks at once, a wave per block and chain (sa_decode.hip): the QUAL and SEQ chains run
 * in launches of SA_DEC_SLICE symbols (default 2^18), a number of launches fixed before the first
 * one from the blocks' symbol counts; at most SA_DEC_INFLIGHT blocks (default: what 7/8 of the
 * device's free memory holds) are on the device at a time.  Both are read at sa_decoder_create. */
typedef struct sa_decoder sa_decoder;
sa_decoder *sa_decoder_create(int device);      /* own stream; no sa_ctx needed */
void sa_decoder_destroy(sa_decoder *);
const char *sa_decoder_error(const sa_decoder *);
/* n blocks of one no-reference archive: in[i]/len[i]/long_reads[i] as for sa_decode_block, out[i] caller-owned
 * as for sa_decode_block.  status[i]: SA_DEC_*.  threads: host threads for the pre-pass and MD5.
 * Returns the number of blocks whose status != 0, or <0 for a call error.  A block with a status has
 * undefined out[i] contents; the caller may hand it to sa_decode_block. */
int sa_decode_blocks(sa_decoder *, const uint8_t *const *in, const uint64_t *len, const int32_t *long_reads,
                     uint32_t n, const sa_cfg *cfg, const uint8_t tmpl[512], int threads,
                     sa_decoded *out, uint32_t *status);
typedef struct { uint32_t groups, inflight, slice, qual_launches, seq_launches, unsupported;
                 float init_ms, qual_ms, place_ms, seq_ms, h2d_ms, d2h_ms; } sa_decode_info;
void sa_decoder_info(const sa_decoder *, sa_decode_info *);   /* the last call */

/* RFC 1321 MD5 (MD5File@0x405950 of the reference FASTA, the block digests) */
void sa_md5(const uint8_t *data, uint64_t len, uint8_t digest[16]);

/* 16-byte header; block_bytes = sum of the blocks' sizes. Returns 0. */
int sa_arc_header(uint64_t block_bytes, uint8_t out[16]);
/* Trailer bytes written to out (written at offset 16 + block_bytes), or -1
 * (writeParam@0x416450 + writeMd5@0x416b10 + writeBlockLenArry{SE,PE}@0x416d60/0x416e90). */
int64_t sa_arc_trailer(const sa_arc_info *info, const sa_arc_block *blocks, uint32_t nblocks,
                       uint8_t *out, uint64_t cap);
/* The same with the reference path's maxmis (param+0x1b60, 0..8).  SeqArc reads it
 * from ./seqarc.config and stores none; a value other than its default 7 is
 * written as params field 19 so that -d rebuilds the same Mis model.
 * sa_arc_trailer(...) == sa_arc_trailer2(info, 7, ...). */
int64_t sa_arc_trailer2(const sa_arc_info *info, int32_t maxmis, const sa_arc_block *blocks, uint32_t nblocks,
                        uint8_t *out, uint64_t cap);

/* ---- HASH reference index and gapless seed alignment ----
 * The index `SeqArc -i ref.fa` builds (HashAlignment::buildRefIndex@0x410190
 * with HashRefIndex32: FASTA < 5 GiB), built on ctx's device and kept there;
 * K / step / maxcount = param+0x1b64 / +0x1b70 / 2^(+0x1b6c) (14, 2, 65536).
 * NULL on error (sa_last_error(ctx)). */
typedef struct sa_hash_index sa_hash_index;
sa_hash_index *sa_hash_build(sa_ctx *ctx, const char *fasta, uint64_t bytes, uint32_t K, uint32_t step,
                             uint32_t maxcount);
/* the "<ref.fa>.hash" file (HashRefIndex32::writeIndexFile@0x41ed00): K, bases,
 * words, positions (u32), packed bases, per-K-mer counts, starts, positions */
uint64_t sa_hash_file_bytes(const sa_hash_index *ix);
int sa_hash_serialize(sa_ctx *ctx, const sa_hash_index *ix, uint8_t *out, uint64_t cap);
uint32_t sa_hash_genome_length(const sa_hash_index *ix);
void sa_hash_destroy(sa_hash_index *ix);
/* getHashAlignInfo@0x4113c0 for n reads in order (HashAlignment::doSEAlign@
 * 0x4117b0; doPEAlign@0x4117d0 aligns each mate the same way): per read the
 * mismatch count or -1 (unaligned), strand (1: reverse complement), 1-based
 * reference position, and maxmis + 1 slots of mismatch offsets and types (-1
 * past the read's mismatches).  maxmis = param+0x1b60 (7), good = +0x1b74 (1).
 * *ai_nmis is the align_info state the reference carries from read to read
 * (AlignParam+0xc, never reset by doAlign@0x411910): in, before the first
 * read; out, after the last. */
int sa_hash_align(sa_ctx *ctx, const sa_hash_index *ix, const char *seq, const uint64_t *off, const int32_t *lens,
                  int64_t n, int32_t maxmis, int32_t good, int32_t *ai_nmis, int32_t *ret, uint8_t *rev,
                  uint64_t *pos, int32_t *mispos, int32_t *mistype);

/* ---- reference path: the block encoder with a HASH index ---------------
 * Replaces, per block, EncapFqzComp::doAlignEncode@0x42d4c0 together with the
 * per-block alignment driver ISeqArcEncodeThread::doTask@0x433ed8 runs before
 * it (AlignEncodeSEJob::doAlign@0x411910 / AlignEncodePEJob::doAlign@0x413580):
 * every read aligned (getHashAlignInfo@0x4113c0), aligned reads coded as order /
 * position / mismatch / strand streams (and the PE mate relation), the rest
 * through the SEQ stream.  The encode thread carries one align_info per mate
 * from read to read and from block to block; an sa_align_chain is that state,
 * and batches of one input pass it on in order. */
typedef struct {
    const sa_hash_index *index;   /* on the encoding context's device              */
    int32_t paired;               /* PE, reads interleaved r1, r2 (-2 given)       */
    int32_t maxmis;               /* param+0x1b60 (7), 0..8 (the Mis model's range) */
    int32_t good;                 /* param+0x1b74 (1)                              */
    uint32_t insert_size;         /* -I (param+0x28); 0: estimated per block       */
} sa_align_cfg;
typedef struct sa_align_chain sa_align_chain;
/* the align_info mismatch counts before the first batch (AlignParam+0xc / +0x54;
 * 0 for a fresh encode thread) */
sa_align_chain *sa_align_chain_create(int32_t nmis_mate1, int32_t nmis_mate2);
void sa_align_chain_destroy(sa_align_chain *ch);
/* marks the chain failed: every call waiting on it (and every later one)
 * returns an error.  For a caller whose batch cannot reach the chain (e.g. its
 * staging failed), so that the batches after it do not wait forever. */
void sa_align_chain_fail(sa_align_chain *ch);
/* encodes the resident batch in the doAlignEncode layout; batch = its place in
 * the chain (0, 1, 2, ...: a call waits until the previous batch has passed
 * its alignment), or UINT64_MAX for the chain's next.  Then sa_fetch. */
int sa_run_input_aligned(sa_ctx *ctx, const sa_input *in, const sa_cfg *cfg, const sa_align_cfg *acfg,
                         sa_align_chain *chain, uint64_t batch);
int sa_run_aligned(sa_ctx *ctx, const sa_cfg *cfg, const sa_align_cfg *acfg, sa_align_chain *chain, uint64_t batch);
/* one-shot form of the above (sub-batches in order through the chain) */
int sa_encode_blocks_aligned(sa_ctx *ctx, const sa_block *in, int n, const sa_cfg *cfg, const sa_align_cfg *acfg,
                             sa_align_chain *chain, sa_out *out);
/* device time (ms, HIP events) of sa_hash_align's aligner kernel over all the
 * reads of the last call (the first pass: the carried state "not aligned") */
float sa_hash_align_kernel_ms(const sa_ctx *ctx);
/* the ".hash" file back onto ctx's device (HashRefIndex32::readIndexFile) */
sa_hash_index *sa_hash_load(sa_ctx *ctx, const uint8_t *file, uint64_t bytes);
/* the genome's packed bases (16 a word, 2 bits, first base in the top bits,
 * N as A): what decoding an aligned read reads (HashAlignment::doGetSeq@0x40ff90);
 * out has room for (bases + 15) / 16 words */
int sa_hash_packed(sa_ctx *ctx, const sa_hash_index *ix, uint32_t *out, uint64_t words);

/* ---- BGZF inflate on the device ------------------------------------------
 * bgzip's BGZF is a series of gzip members of at most 64 KiB of text each, every
 * one an independent raw-DEFLATE stream whose compressed size is in its 'BC'
 * extra field and whose CRC-32 and ISIZE are in its trailer.  sa_bgzf_scan walks
 * the members of a buffer on the host; sa_inflate_members inflates them on the
 * device, one wave per member (k_inflate_bgzf), and checks each one's CRC. */
typedef struct { uint64_t in_off; uint32_t in_len; uint64_t out_off; uint32_t isize; uint32_t crc; } sa_bgzf_member;
/* per-member status of sa_inflate_members */
enum {
    SA_INFL_OK = 0,
    SA_INFL_INPUT = 1,   /* the deflate stream runs past the member's compressed bytes */
    SA_INFL_BLOCK = 2,   /* block type 3, or a stored block's LEN != ~NLEN              */
    SA_INFL_CODES = 3,   /* code lengths zlib rejects, or a code that stands for nothing */
    SA_INFL_DIST = 4,    /* a match reaches back past the member's first byte           */
    SA_INFL_SIZE = 5,    /* the stream's output is not ISIZE bytes                      */
    SA_INFL_CRC = 6      /* the output's CRC-32 is not the trailer's                    */
};
/* host: walk whole members in buf[0..have); *consumed = bytes of whole members, *out_bytes = sum of ISIZE.
 * ms[i].in_off / in_len: the member's deflate bytes in buf; out_off: the sum of the ISIZEs before it.
 * Returns the number of members (a member cut by the end of buf is left: *consumed < have), or
 * <0: not BGZF / malformed header (-1), member larger than the format allows (-2), more than
 * max_members (-3) */
int64_t sa_bgzf_scan(const uint8_t *buf, uint64_t have, sa_bgzf_member *ms, uint64_t max_members,
                     uint64_t *consumed, uint64_t *out_bytes);
typedef struct sa_inflater sa_inflater;
sa_inflater *sa_inflater_create(int device);          /* own stream and device slabs; no sa_ctx needed */
void sa_inflater_destroy(sa_inflater *);
/* H2D of in[0..in_bytes), kernel, D2H into out[0..out_bytes); status may be NULL.
 * Every member is checked on the host first (in_off + in_len <= in_bytes, out_off + isize <=
 * out_bytes, isize <= 65536): a bad descriptor is a call error and nothing is launched.  A
 * member of isize 0 (the end-of-file marker) is ok when its crc is 0.  The copies are DMAs
 * when in / out are sa_host_alloc memory and work from pageable memory too.
 * All of out[0..out_bytes) is overwritten: the ranges of failed members, and any gaps the
 * caller leaves between the members' ranges, with undefined bytes (the device slab is not
 * cleared between calls).
 * 0: every member ok; >0: number of failed members (status[i] says why); <0: call error */
int sa_inflate_members(sa_inflater *, const uint8_t *in, uint64_t in_bytes, const sa_bgzf_member *ms,
                       uint32_t n, uint8_t *out, uint64_t out_bytes, uint32_t *status);
const char *sa_inflater_error(const sa_inflater *);
float sa_inflater_kernel_ms(const sa_inflater *);      /* HIP events around the last kernel */
/* (tests and diagnostics only) workgroups (one wave each) a launch uses at most: two per CU, or
 * env SA_INFL_GRID (a small value makes every wave take many members), read at
 * sa_inflater_create; lets a test assert that the knob took effect */
uint32_t sa_inflater_grid(const sa_inflater *);

/* ---- ordinary gzip inflated on the device -----------------------------------
 * A gzip member (gzip, pigz, members concatenated) carries no sizes and no restart points.
 * sa_gunzip_run inflates it by speculation: the compressed bytes are cut into chunks
 * (env SA_GUNZIP_CHUNK, bytes), k_gz_find looks in each for the first bit position at which
 * a dynamic block can start, k_gz_spec decodes one wave per start into 16-bit symbols in
 * which references to the unknown 32 KiB before the start are markers, k_gz_chain confirms
 * the starts a predecessor's decode ended at exactly and derives every confirmed wave's true
 * window, k_gz_resolve replaces the markers and k_gz_crc sums the text; the host compares
 * each member's CRC-32 and ISIZE with its trailer.  No kernel waits for another wave. */
enum {
    SA_INFL_HEADER = 7,  /* the stream does not begin with a gzip member header            */
    /* why the confirmed prefix of a call ended (sa_gunzip_info.end_why), besides SA_INFL_* */
    SA_GZ_MET = 16,      /* (a wave's stop: a block boundary at the next start)             */
    SA_GZ_FULL = 17,     /* the wave's symbol range is full (env SA_GUNZIP_RATIO)           */
    SA_GZ_END = 18,      /* the input ends after a member's trailer, or no member follows   */
    SA_GZ_BREAKS = 19,   /* the wave ended eight members                                    */
    SA_GZ_OUTCAP = 20    /* the next wave's text does not fit out_cap                       */
};
/* Where a stream stands between calls.  All zeros: the start of a file. */
typedef struct {
    uint32_t in_stream;      /* 0: a member header is next; 1: inside a deflate stream, at a block start */
    uint32_t bit;            /* in_stream: bits of the next call's first byte that are consumed (0..7)   */
    uint32_t win_len;        /* in_stream: text bytes of this member before the position, at most 32768  */
    uint32_t crc;            /* CRC-32 of the current member's text so far                               */
    uint64_t len;            /* ... and its length                                                       */
    uint32_t ended;          /* 1: the stream is over (bytes that are no gzip member follow the last)    */
    uint32_t reserved;
    uint8_t window[32768];   /* the last win_len text bytes, at the END of the array (a dictionary)      */
} sa_gunzip_state;
typedef struct {
    uint32_t chunks;            /* chunks of the call's input                                */
    uint32_t candidates;        /* block starts the finder returned                          */
    uint32_t waves_confirmed;   /* waves whose text is in the output                         */
    uint32_t false_skipped;     /* candidates the confirmed waves decoded past               */
    uint32_t members_ended;     /* trailers checked                                          */
    uint32_t end_wave;          /* the wave that ended the confirmed prefix ...              */
    uint32_t end_why;           /* ... and why: SA_GZ_* or SA_INFL_*                         */
    uint32_t status;            /* the return value when it is > 0                           */
    float find_ms, spec_ms, chain_ms, resolve_ms, crc_ms;   /* HIP events around each kernel */
} sa_gunzip_info;
typedef struct sa_gunzipper sa_gunzipper;
sa_gunzipper *sa_gunzipper_create(int device);        /* own stream and device slabs; no sa_ctx needed */
void sa_gunzipper_destroy(sa_gunzipper *);
/* Inflates in[0..in_bytes) (at most 256 MiB), which continues the stream at *state, as far as
 * the confirmed prefix reaches and its text fits out_cap (cut at a wave's boundary), into
 * out[0..*out_bytes); *in_used: the whole input bytes consumed -- the caller carries
 * in[*in_used..) into the next call, in front of new input; *state is updated.  eof: no input
 * follows in[0..in_bytes).  info may be NULL.  The copies are DMAs when in / out are
 * sa_host_alloc memory and work from pageable memory too.
 * 0: progress, a clean end of the stream (state->ended, or eof with *in_used == in_bytes and
 * no member open), or no progress because the input ends inside the first block (more input
 * decides) or the first wave's symbols do not fit (info->end_why == SA_GZ_FULL: the caller
 * continues on the host from *state); >0: the stream is corrupt, an SA_INFL_* code (the text
 * before the error is delivered); <0: call error (-2: out_cap is too small for the first wave) */
int sa_gunzip_run(sa_gunzipper *, const uint8_t *in, uint64_t in_bytes, int eof, sa_gunzip_state *state,
                  uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint64_t *in_used, sa_gunzip_info *info);
const char *sa_gunzipper_error(const sa_gunzipper *);
float sa_gunzipper_kernel_ms(const sa_gunzipper *);    /* the last call's kernels together */
/* (tests and diagnostics) workgroups a launch uses at most: two per CU, or env SA_GUNZIP_GRID,
 * read at sa_gunzipper_create like SA_GUNZIP_CHUNK and SA_GUNZIP_RATIO */
uint32_t sa_gunzipper_grid(const sa_gunzipper *);
uint32_t sa_gunzipper_chunk(const sa_gunzipper *);     /* bytes per chunk in effect */

/* ---- text resident on the device: sa_devtext --------------------------------
 * One input's FASTQ text as a stream in device memory: a linear buffer with a read and a
 * write position and a stream of its own; no sa_ctx needed.  Text arrives by sa_devtext_append
 * (from the host), sa_inflate_members_dev (BGZF members inflated straight into it) or
 * sa_gunzip_run_dev (ordinary gzip, by speculation, straight into it), the block
 * cut of sa_cut_next_se / sa_cut_next_pe runs on the device (sa_devtext_cut, k_dt_cut), a block
 * leaves as a sa_devblock, made by sa_devtext_take, and reaches an encoder's text arena by
 * sa_text_upload_dev; sa_text_parse then works as after sa_text_upload.  The text never
 * crosses to the host: per block only its lengths do.
 * Threads: one thread at a time drives a devtext (append, inflate, cut, take, peek).  A
 * devblock is a copy and belongs to whoever holds it: another thread may upload or fetch it
 * while the devtext goes on.  Every call returns with its device work done. */
typedef struct sa_devtext sa_devtext;
typedef struct sa_devblock sa_devblock;
/* why sa_devtext_cut stopped */
enum {
    SA_CUT_MORE = 1,   /* the next block needs more text (the host cut's "read more")        */
    SA_CUT_DONE = 2,   /* every input is at eof and empty                                   */
    SA_CUT_FULL = 3,   /* max_blocks blocks were cut                                        */
    SA_CUT_NONE = 4    /* a full window without a cut (the host cut's -1: mates out of step) */
};
sa_devtext *sa_devtext_create(int device, uint64_t capacity);   /* NULL: no gfx950 device, or no memory */
void sa_devtext_destroy(sa_devtext *);
const char *sa_devtext_error(const sa_devtext *);
uint64_t sa_devtext_avail(const sa_devtext *);   /* bytes between the read and the write position */
/* bytes an append can take now: capacity - avail.  When the room behind the write position
 * is too small, the append first moves the unread bytes to the front of the buffer (device
 * to device, in pieces that never overlap their source) and counts their newlines again. */
uint64_t sa_devtext_room(const sa_devtext *);
/* host bytes to the write position; -3 (nothing done) when n > room, -1: call / device error */
int sa_devtext_append(sa_devtext *, const uint8_t *bytes, uint64_t n);
/* sa_inflate_members without the copy of the text to the host: the members' text lands at the
 * devtext's write position back to back in list order (ms[i].out_off is not read, so any
 * part of a scanned member list can be passed as it is).  The same host checks of in_off,
 * in_len and isize, the same status array and return value as sa_inflate_members, and -3
 * (nothing done) when the sum of the ISIZEs exceeds sa_devtext_room: pass fewer members.
 * If any member fails or the call does, the write position does not move
 * (unread text may have been moved to the front, which sa_devtext_peek / _cut do not see). */
int sa_inflate_members_dev(sa_inflater *, const uint8_t *in, uint64_t in_bytes, const sa_bgzf_member *ms,
                           uint32_t n, sa_devtext *dt, uint32_t *status);
/* sa_gunzip_run without the copy of the text to the host: the confirmed prefix's text lands at
 * the devtext's write position (the devtext must be on the gunzipper's device).  out_cap is the
 * most text the call may deliver: -3 (nothing done) when it exceeds sa_devtext_room; otherwise
 * room for out_cap bytes is made behind the write position first, as an append does (unread
 * text may move to the front).  0: *text_bytes bytes were appended and counted, and *in_used,
 * *state and *info are sa_gunzip_run's.  Any other return value -- > 0: the stream is corrupt
 * (SA_INFL_*), < 0: a call error (-2: out_cap is too small for the first wave) -- leaves the
 * write position where it was and *text_bytes = 0; no byte below the write position is written,
 * the bytes behind it are scratch.  Unlike sa_gunzip_run this call does not deliver the text
 * before an error, and *state after a positive return is not one to continue from: the input
 * has failed.  The 256 MiB input limit and sa_gunzipper_kernel_ms are sa_gunzip_run's;
 * sa_gunzipper_error carries the devtext's error text when the devtext failed. */
int sa_gunzip_run_dev(sa_gunzipper *, const uint8_t *in, uint64_t in_bytes, int eof, sa_gunzip_state *state,
                      sa_devtext *dt, uint64_t out_cap, uint64_t *text_bytes, uint64_t *in_used,
                      sa_gunzip_info *info);
/* n bytes at read position + off to the host (the first line, the bare-'+' test) */
int sa_devtext_peek(sa_devtext *, uint64_t off, uint8_t *out, uint64_t n);
/* Cuts as many blocks as the unread text holds, at most max_blocks: block 0 starts at the
 * read positions, each further one where the last ended; nothing is consumed.  t2 = NULL:
 * single-end (len2 may be NULL).  eof: the devtext holds the rest of its input.  first / flen:
 * input 1's first line, '\n' included (host memory).  The lengths are, block for block, what
 * repeated sa_cut_next_se / sa_cut_next_pe return on the same bytes with the same avail and
 * eof.  Returns the block count and in *end an SA_CUT_* value, or -1 for a call error. */
int64_t sa_devtext_cut(sa_devtext *t1, int eof1, sa_devtext *t2, int eof2, uint64_t block_size,
                       const uint8_t *first, uint64_t flen, uint64_t *len1, uint64_t *len2,
                       uint64_t max_blocks, int32_t *end);
/* One block's text copied device to device into an allocation of its own (from a pool of
 * the device that sa_devblock_release gives it back to), the read positions advanced.
 * t2 = NULL: single-end.  NULL on error (sa_devtext_error(t1)). */
sa_devblock *sa_devtext_take(sa_devtext *t1, uint64_t len1, sa_devtext *t2, uint64_t len2);
void sa_devblock_release(sa_devblock *);
/* the block's text lengths; returns 1 for a paired block, 0 for single-end */
int sa_devblock_lens(const sa_devblock *, uint64_t *len1, uint64_t *len2);
/* the block's text to the host (out2 may be NULL); the command line needs it for block 0 only */
int sa_devblock_fetch(const sa_devblock *, uint8_t *out1, uint8_t *out2);
/* frees the device's pooled allocations that no devblock holds */
void sa_devblock_pool_trim(int device);
/* sa_text_upload with a device source: the devblock's text to block `index` of arena `slot`,
 * device to device on the context's copy stream, done on return.  Then sa_text_parse.  A
 * helper thread may call this while the context runs a batch, so its error text is kept apart
 * from sa_last_error's, under the upload lock: sa_upload_error(ctx) after a non-zero return.
 * (sa_text_upload is unchanged and still reports through sa_last_error.) */
int sa_text_upload_dev(sa_ctx *ctx, sa_input *in, int slot, int index, int nmax, const sa_devblock *blk,
                       uint64_t stride);
const char *sa_upload_error(sa_ctx *ctx);   /* valid until the context's next sa_text_upload_dev */
/* device time (ms, HIP events) of the devtext's last newline count and last cut (the cut is
 * timed on the devtext passed as t1); either pointer may be NULL */
void sa_devtext_kernel_ms(const sa_devtext *, float *count_ms, float *cut_ms);
/* bytes the last newline count covered (with count_ms: the count's rate) */
uint64_t sa_devtext_count_bytes(const sa_devtext *);

#ifdef __cplusplus
}
#endif
#endif
