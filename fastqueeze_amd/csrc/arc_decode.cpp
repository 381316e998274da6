// arc_decode.cpp -- host decoder of one encoded block (SeqArc -d path).
//
// The inverse of the block layout doFqzEncode@0x42d2d0 writes; the reference's
// decoder is EncapFqzComp::doFqzDecode@0x42c680 (decode_seq@0x4296b0,
// decode_qual@0x42a750, decode_name@0x428380, the Dege decoders) and, in ID-bin
// mode, IDProcess::decodeIDS@0x430610 + assembleNameS@0x4300a0.  Adaptive
// decoding is a serial chain per stream (each symbol updates the model the next
// one is read with), so blocks are decoded on host threads, one block each.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "arc_decode_host.h"

namespace {

using namespace sadh;

int64_t decode_block(const uint8_t* in, uint64_t in_len, const sa_cfg* cfg, const uint8_t tmpl[512],
                     int32_t long_reads, const sa_ref* ref, sa_decoded* o)
{
    if (!in || !cfg || !o) return -1;
    Cursor c{in, in + in_len};
    o->md5_ok = 1;
    uint32_t n = 0;
    if (!dec_open(c, n)) return -1;
    if (n > o->max_reads) return -1;
    o->nreads = n;
    std::vector<uint32_t> len(n);
    const bool md5_q = cfg->md5 && !(cfg->lossy > 0.0);
    uint8_t dg_id[16], dg_q[16], dg_s[16];

    if (!dec_lengths(c, long_reads, n, len)) return -1;
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; r++) { o->seq_lens[r] = (int32_t)len[r]; total += len[r]; }
    if (total > o->seq_cap) return -1;
    // reference path: order count and bytes (doAlignEncode@0x42d4c0)
    uint32_t norder = 0;
    std::vector<uint8_t> order;
    if (ref) {
        if (!count_encap(c, 0x1b, norder) || norder > n || !sm_stream(c, 8, 5, norder, order)) return -1;
    }

    uint64_t name_total = 0;
    if (!dec_names(c, cfg, tmpl, o, n, dg_id, name_total)) return -1;

    {   // qualities: compressQual@0x426e80 / encode_qual@0x422180
        if (!c.id(7)) return -1;
        const uint32_t sz = c.size4();
        if (c.bad) return -1;
        const uint8_t* q = c.p;
        if (md5_q) { memcpy(dg_q, q, 16); q += 16; }
        const uint32_t nm = cfg->qlevel > 2 ? 0x100000u : 0x10000u;
        std::unique_ptr<SModel[]> qm(new SModel[nm]);
        for (uint32_t i = 0; i < nm; i++) qm[i].reset(95);
        RangeIn rc(q, c.p + sz);
        uint8_t* Q = o->qual;
        for (uint32_t r = 0; r < n && !rc.bad; r++) {
            uint32_t last = 0;
            int q1 = 0, q2 = 0, delta = 5;
            for (uint32_t i = 0; i < len[r]; i++) {
                const int s = qm[last].decode(rc);
                if (s == 94) { memset(Q + i, '#', len[r] - i); break; }   // the stripped trailing '#' run
                Q[i] = (uint8_t)(s + 33);
                uint32_t ctx = ((uint32_t)((q1 > q2 ? q1 : q2) << 6) + (uint32_t)s) & 0xfffu;
                if (cfg->qlevel > 1) {
                    ctx += q1 == q2 ? 0x1000u : 0u;
                    delta += q1 > s ? q1 - s : 0;
                    ctx += (uint32_t)(((delta <= 56 ? delta : 56) & 0xf8) << 10);
                    if (cfg->qlevel > 2) ctx += i <= 0x6f ? (uint32_t)(((i + 15) & 0x78) << 13) : 0xf0000u;
                }
                q2 = q1;
                q1 = s;
                last = ctx;
            }
            Q += len[r];
        }
        if (rc.bad) return -1;
        c.p += sz;
    }

    // reference path: the alignment streams (counts, PE relation, position bits,
    // mismatch counts, strands, mismatch offset bits and types)
    uint32_t nalign = 0, npos = 0, ncigl = 0, ncigv = 0, ibits = 0, nperel = 0;
    std::vector<uint8_t> perel, posb, mis, rev, cigl, cigv;
    if (ref) {
        if (!count_encap(c, 0x11, nalign) || !count_encap(c, 0x12, npos) || !count_encap(c, 0x13, ncigl) ||
            !count_encap(c, 0x14, ncigv))
            return -1;
        if (ref->paired && (!count_encap(c, 0x15, ibits) || !count_encap(c, 0x16, nperel) ||
                            !sm_stream(c, 9, 4, nperel, perel)))
            return -1;
        const int mis_nsym = ref->maxmis >= 1 && ref->maxmis <= 7 ? 8 : ref->maxmis == 8 ? 9 : 0;
        if (!sm_stream(c, 0xb, 2, npos, posb) || !sm_stream(c, 0xf, mis_nsym, nalign, mis) ||
            !sm_stream(c, 0xa, 2, nalign, rev) || !sm_stream(c, 0xc, 2, ncigl, cigl) ||
            !sm_stream(c, 0xd, 4, ncigv, cigv))
            return -1;
    }

    // N / IUPAC side streams (DegeInfoProcess@0x433a10): 23 tip, 14 chars,
    // 24 max quality, 25 exception counts, 26 gaps (25 and 26 share one kModel)
    DecSide side;
    std::vector<uint8_t> isn(total, 0);
    {
        if (!dec_side(c, n, side)) return -1;
        const std::vector<uint8_t>&tip = side.tip, &chs = side.chs, &maxq = side.maxq;
        const std::vector<uint64_t>&exc = side.exc, &gaps = side.gaps;
        // a tip-1 read's candidate positions (quality <= its max) read
        // N^g1 B N^g2 B ... N^gE B N...: gaps g, E = exception count.  With -l
        // the candidates were chosen on the original qualities, which the
        // archive no longer holds (the reference's decoder fails there, SURVEY
        // section 5 ii): placement stops at the first inconsistency and the
        // sequence MD5 reports it.
        const bool lenient = cfg->lossy > 0.0;
        size_t it = 0, ig = 0, ic = 0;
        uint64_t at = 0;
        const uint8_t* Q = o->qual;
        for (uint32_t r = 0; r < n; r++) {
            if (tip[r]) {
                const int mq = (int)maxq[it] + 33;
                const uint64_t E = exc[it++];
                uint64_t e = 0;
                uint64_t rem = ~0ull;
                bool stop = false;
                if (E) {
                    if (ig >= gaps.size()) { if (!lenient) return -1; stop = true; }
                    else rem = gaps[ig];
                }
                for (uint32_t i = 0; i < len[r] && !stop; i++) {
                    if ((int)(int8_t)Q[i] > mq) continue;
                    if (e < E && rem == 0) {
                        e++;
                        ig++;
                        rem = ~0ull;
                        if (e < E) {
                            if (ig >= gaps.size()) { if (!lenient) return -1; stop = true; }
                            else rem = gaps[ig];
                        }
                    } else {
                        if (ic >= chs.size()) { if (!lenient) return -1; stop = true; break; }
                        const uint8_t sc = chs[ic++];
                        isn[at + i] = (uint8_t)kIupac[sc < 11 ? sc : 0];
                        rem--;
                    }
                }
            }
            Q += len[r];
            at += len[r];
        }
        if (ic != chs.size() && !lenient) return -1;
    }

    {   // bases: compressSeq@0x4248a0 / encode_seq@0x421f30 (BASE_MODEL, order k)
        if (!c.id(6)) return -1;
        const uint32_t sz = c.size4();
        if (c.bad) return -1;
        const uint8_t* q = c.p;
        if (cfg->md5) { memcpy(dg_s, q, 16); q += 16; }
        const int k = cfg->slevel + 7;
        const uint32_t ns = 1u << ((2 * k) & 31), mask = ns - 1;
        std::vector<uint8_t> tab((size_t)ns * 4, 3);
        RangeIn rc(q, c.p + sz);
        uint8_t* S = o->seq;
        uint64_t at = 0;
        // with -l a misplaced N shifts the base stream (see above): the rest of
        // the block decodes as 'N' and the sequence MD5 reports it
        const bool lenient = cfg->lossy > 0.0;
        // reference path: decompressSeq@0x42e390 rebuilds the reads with an order
        // byte from the genome (getRealPos@0x42de30: the position from the order
        // byte and low bits, or for a PE mate 2 after an aligned mate 1 from the
        // relation; AlignInfoToSeq@0x42e020: the segment, its mismatches, the
        // strand), the N / IUPAC bases then from the side streams
        size_t ip = 0, ia = 0, il = 0, iv = 0, ir = 0;
        if (ref && !ibits && ref->insert_size)   // -I: the encoder used bits(I), the block says 0
            for (uint32_t v = ref->insert_size; v; v >>= 1) ibits++;
        uint64_t last_pos = 0;
        const uint32_t shift = ref && ref->bases ? (uint32_t)(64 - __builtin_clzll(ref->bases)) - 2 : 0;
        auto take_bits = [&](uint32_t nb, const std::vector<uint8_t>& v, size_t& at, bool& ok) {
            uint64_t x = 0;
            for (uint32_t k = 0; k < nb; k++) {
                if (at >= v.size()) { ok = false; return x; }
                x |= (uint64_t)v[at++] << k;
            }
            return x;
        };
        auto nbits = [](uint64_t v) { uint32_t k = 0; while (v) { k++; v >>= 1; } return k; };
        for (uint32_t r = 0; r < n && (!rc.bad || lenient); r++) {
            if (ref && r < norder && order[r]) {
                bool ok = true;
                uint64_t pos;
                if (ref->paired && (r & 1) && order[r - 1]) {
                    const uint8_t rl = ir < perel.size() ? perel[ir++] : 0xff;
                    if (rl == 1) pos = last_pos + take_bits(ibits, posb, ip, ok);
                    else if (rl == 0) pos = last_pos - take_bits(ibits, posb, ip, ok);
                    else if (rl == 2) pos = take_bits(nbits(last_pos), posb, ip, ok);
                    else if (rl == 3) pos = last_pos + take_bits(nbits(ref->bases - last_pos), posb, ip, ok);
                    else return -1;
                } else {
                    pos = ((uint64_t)(order[r] - 1) << shift) + take_bits(shift, posb, ip, ok);
                }
                last_pos = pos;
                if (ia >= mis.size() || ia >= rev.size()) return -1;
                const uint32_t nm = mis[ia], rv = rev[ia];
                ia++;
                const uint32_t L = len[r];
                if (!ok || pos == 0 || pos - 1 + L > ref->bases) return -1;
                std::vector<uint8_t> seg(L);
                for (uint32_t i = 0; i < L; i++) {   // doGetSeq@0x40ff90: 2-bit codes (N read as A)
                    const uint64_t q = pos - 1 + i;
                    seg[i] = (uint8_t)((ref->genome[q >> 4] >> (30 - 2 * (q & 15))) & 3u);
                }
                uint32_t prev = 0;
                for (uint32_t k = 0; k < nm; k++) {
                    const uint32_t at2 = prev + (uint32_t)take_bits(nbits(L - prev), cigl, il, ok);
                    if (!ok || at2 >= L || iv >= cigv.size()) return -1;
                    seg[at2] = (uint8_t)var2base(seg[at2], cigv[iv++]);
                    prev = at2;
                }
                for (uint32_t i = 0; i < L; i++) {   // getch@0x40dc50
                    uint32_t b = seg[rv ? L - 1 - i : i];
                    if (b < 4 && rv) b = 3 - b;
                    S[i] = isn[at + i] ? isn[at + i] : (uint8_t)(b < 4 ? "ACGT"[b] : 'N');
                }
                S += L;
                at += L;
                continue;
            }
            uint32_t ctx = 0x7616c7u & mask;
            for (uint32_t i = 0; i < len[r]; i++) {
                if (isn[at + i]) { S[i] = isn[at + i]; continue; }
                if (rc.bad) { S[i] = 'N'; continue; }
                uint8_t* m = &tab[(size_t)ctx * 4];
                uint32_t tot = (uint32_t)m[0] + m[1] + m[2] + m[3];
                if (tot > 253) {
                    for (int j = 0; j < 4; j++) m[j] = (uint8_t)(m[j] - (m[j] >> 1));
                    tot = (uint32_t)m[0] + m[1] + m[2] + m[3];
                }
                uint32_t scale;
                const uint32_t v = rc.slot(tot, scale);
                uint32_t cum = 0, b = 0;
                while (b < 3 && cum + m[b] <= v) cum += m[b++];
                rc.consume(scale, cum, m[b]);
                m[b]++;
                S[i] = (uint8_t)"ACGT"[b];
                ctx = ((ctx << 2) + b) & mask;
            }
            S += len[r];
            at += len[r];
        }
        if (rc.bad && !lenient) return -1;
        if (rc.bad) o->md5_ok = 0;
        c.p += sz;
    }
    if (c.p != c.end) return -1;
    if (cfg->md5 && !dec_md5_verify(o, name_total, total, md5_q, dg_id, dg_q, dg_s)) o->md5_ok = 0;
    return (int64_t)n;
}

}  // namespace

extern "C" void sa_md5(const uint8_t* data, uint64_t len, uint8_t digest[16]) { md5(data, (size_t)len, digest); }

extern "C" int64_t sa_decode_block(const uint8_t* in, uint64_t in_len, const sa_cfg* cfg, const uint8_t tmpl[512],
                                   int32_t long_reads, sa_decoded* o)
{
    return decode_block(in, in_len, cfg, tmpl, long_reads, nullptr, o);
}

extern "C" int64_t sa_decode_block_ref(const uint8_t* in, uint64_t in_len, const sa_cfg* cfg, const uint8_t tmpl[512],
                                       int32_t long_reads, const sa_ref* ref, sa_decoded* o)
{
    if (!ref || !ref->genome || ref->bases < 4) return -1;
    return decode_block(in, in_len, cfg, tmpl, long_reads, ref, o);
}
