// arc_decode_host.h -- the host pieces of the block decoder that more than one
// path uses: the range decoder, SIMPLE_MODEL / kModel, MD5, the encap cursor,
// the name decoders and the pre-pass over the small streams (count, lengths,
// names, the five N / IUPAC side streams).  sa_decode_block (arc_decode.cpp)
// decodes a whole block with them; the host emulation of the many-blocks-at-once
// decoder (tests/cpu_emu/decode_emu.cpp) runs the pre-pass and leaves the QUAL
// and SEQ chains to sa_decode_logic.h.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/seqarc_amd.h"

namespace sadh {

// ---- carry-less range decoder (Subbotin; the coder of encode_seq@0x422010) ----
class RangeIn {
public:
    RangeIn(const uint8_t* p, const uint8_t* end) : p_(p), end_(end)
    {
        for (int i = 0; i < 8; i++) code_ = (code_ << 8) | byte();
    }
    // slot of the next symbol in [0, tot) and the scale range / tot
    uint32_t slot(uint32_t tot, uint32_t& scale)
    {
        scale = range_ / tot;
        const uint64_t v = (code_ - low_) / scale;
        if (v >= tot) { bad = true; return tot - 1; }
        return (uint32_t)v;
    }
    void consume(uint32_t scale, uint32_t cum, uint32_t freq)
    {
        low_ += (uint32_t)(cum * scale);
        range_ = scale * freq;
        while (range_ < (1u << 24)) {
            if ((low_ ^ (low_ + range_)) >> 56) range_ = ((uint32_t)low_ | 0xffffffu) - (uint32_t)low_;
            code_ = (code_ << 8) | byte();
            range_ <<= 8;
            low_ <<= 8;
        }
    }
    bool bad = false;

private:
    uint8_t byte()
    {
        if (p_ < end_) return *p_++;
        bad = true;
        return 0;
    }
    const uint8_t *p_, *end_;
    uint64_t low_ = 0, code_ = 0;
    uint32_t range_ = 0xffffffffu;
};

// ---- SIMPLE_MODEL<N> (kModelEncode@0x42ccb0 layout): symbol list ordered by
//      bubble swaps every 16th update, +8 per hit, halving above 0xffe0 ----
class SModel {
public:
    void reset(int n)
    {
        n_ = n;
        tot_ = (uint32_t)n;
        bub_ = 0;
        for (int i = 0; i < n; i++) { sym_[i] = (uint16_t)i; freq_[i] = 1; }
    }
    int decode(RangeIn& rc)
    {
        uint32_t scale;
        const uint32_t v = rc.slot(tot_, scale);
        uint32_t acc = 0;
        int i = 0;
        while (i < n_ && acc + freq_[i] <= v) acc += freq_[i++];
        if (i >= n_) { rc.bad = true; return 0; }
        const int s = sym_[i];
        rc.consume(scale, acc, freq_[i]);
        freq_[i] += 8;
        tot_ += 8;
        if (tot_ > 0xffe0) {
            tot_ = 0;
            for (int k = 0; k < n_; k++) { freq_[k] -= freq_[k] >> 1; tot_ += freq_[k]; }
        }
        if ((++bub_ & 15) == 0 && i > 0 && freq_[i] > freq_[i - 1]) {
            std::swap(freq_[i], freq_[i - 1]);
            std::swap(sym_[i], sym_[i - 1]);
        }
        return s;
    }

private:
    int n_ = 0;
    uint32_t tot_ = 0, bub_ = 0;
    uint16_t sym_[256], freq_[256];
};

// kModel (kModelInit@0x42cbe0 / kModelEncode@0x42ccb0): bit count, then bits LSB first
struct KModel {
    SModel nbits, bits[64];
    void reset()
    {
        nbits.reset(64);
        for (auto& b : bits) b.reset(2);
    }
    uint64_t decode(RangeIn& rc)
    {
        const int nb = nbits.decode(rc);
        uint64_t v = 0;
        for (int i = 0; i < nb && i < 64; i++) v |= (uint64_t)bits[i].decode(rc) << i;
        return v;
    }
};

// ---- RFC 1321 MD5 (the block digests, calcBlockMd5@0x414d90) ----
inline void md5(const uint8_t* data, size_t len, uint8_t out[16])
{
    static const uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
        0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
        0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
        0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
        0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
        0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
        0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
        0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    static const uint8_t S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};
    uint32_t h[4] = {0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476};
    auto block = [&](const uint8_t* p) {
        uint32_t M[16];
        for (int i = 0; i < 16; i++) M[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
        for (int i = 0; i < 64; i++) {
            uint32_t f;
            int g;
            const int r = i >> 4;
            if (r == 0) { f = (b & c) | (~b & d); g = i; }
            else if (r == 1) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
            else if (r == 2) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
            else { f = c ^ (b | ~d); g = (7 * i) & 15; }
            const uint32_t x = a + f + K[i] + M[g];
            const int s = S[r][i & 3];
            a = d; d = c; c = b;
            b = b + ((x << s) | (x >> (32 - s)));
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d;
    };
    size_t i = 0;
    for (; i + 64 <= len; i += 64) block(data + i);
    uint8_t tail[128] = {0};
    const size_t r = len - i;
    memcpy(tail, data + i, r);
    tail[r] = 0x80;
    const size_t tl = r < 56 ? 64 : 128;
    const uint64_t bits = (uint64_t)len * 8;
    for (int k = 0; k < 8; k++) tail[tl - 8 + k] = (uint8_t)(bits >> (8 * k));
    block(tail);
    if (tl == 128) block(tail + 64);
    for (int k = 0; k < 16; k++) out[k] = (uint8_t)(h[k >> 2] >> (8 * (k & 3)));
}

// ---- encap walking (the one-byte IDs and 4-byte sizes of this layout) ----
struct Cursor {
    const uint8_t *p, *end;
    bool bad = false;
    bool id(int v)
    {
        if (p < end && *p == (uint8_t)(0x80 | v)) { p++; return true; }
        return false;
    }
    uint32_t size4()
    {
        if (end - p < 4) { bad = true; return 0; }
        const uint32_t v = ((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]) & 0x0fffffffu;
        p += 4;
        if ((uint64_t)(end - p) < v) bad = true;
        return v;
    }
};

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

inline bool is_delim(uint8_t c) { return c == ' ' || (c >= '!' && c <= '/') || (c >= ':' && c <= '@') || (c >= '[' && c <= '`') || (c >= '{' && c <= '~'); }

// encode_name@0x421070 inverse: prefix / suffix / length models keyed by the
// previous name, middle characters keyed by the aligned previous-name byte.
class NameDecoder {
public:
    NameDecoder() : m_(new SModel[768 + 8192])
    {
        for (int i = 0; i < 768; i++) m_[i].reset(256);
        for (int i = 0; i < 8192; i++) m_[768 + i].reset(128);
        buf_[0] = 0;   // the byte before the buffer (an alignment step can reach index -1)
        memset(last_, ' ', 1024 + 1);
    }
    int decode(RangeIn& rc, uint8_t* name, int cap)
    {
        const int p = m_[last_p_].decode(rc), s = m_[256 + last_s_].decode(rc), len = m_[512 + last_len_].decode(rc);
        if (rc.bad || len > cap || p + s > len || p > last_len_ || s > last_len_) return -1;
        last_p_ = p;
        last_s_ = s;
        memcpy(name, last_, (size_t)p);
        const int body = len - s;
        int lc = p != 0, k = 0, j = p;
        for (int i = p; i < body; i++) {
            if (j > 1023) return -1;
            const int ctx = (k * 64 + lc + 2 * ((int)(int8_t)last_[j] - 32)) % 8192;
            if (ctx < 0) return -1;
            const uint8_t c = (uint8_t)m_[768 + ctx].decode(rc);
            name[i] = c;
            bool reset = false;
            if (c == ' ') {
                if (last_[j] != ' ' && last_[j + 1] != ':') j++;
                k = (k + 3) & ~3;
                reset = j < 0;
            } else {
                uint8_t d = last_[j];
                if (d == ' ') d = last_[--j];
                if (c == ':') {
                    j += d != ':';
                    k = (k + 3) & ~3;
                } else {
                    j -= d == ':';
                }
                reset = j < 0;
            }
            if (reset) { j = 0; lc = 0; k++; }
            else { lc = c == last_[j]; j++; k++; }
        }
        memcpy(name + body, last_ + last_len_ - s, (size_t)s);
        memcpy(last_, name, (size_t)len);
        last_len_ = len;
        return rc.bad ? -1 : len;
    }

private:
    std::unique_ptr<SModel[]> m_;
    uint8_t buf_[1 + 1024 + 2];
    uint8_t* const last_ = buf_ + 1;
    int last_len_ = 0, last_p_ = 0, last_s_ = 0;
};

// ID-bin names: decodeIDS@0x430610 / assembleNameS@0x4300a0.  The block keeps
// its first ID; token k of name i is template type T[k+2]: 0 the first ID's
// token, 1 its number + i (+ i/2 for pairs), 3 the read length; mates per the
// PE type T[1]: 1 the same name, 2 the last character '2', 3 the name up to
// its last delimiter + the mate's length.
inline bool bin_names(const uint8_t* first, int flen, const uint8_t T[512], const int32_t* lens, uint32_t n,
               uint8_t* names, uint64_t cap, uint16_t* nl, uint64_t& used)
{
    std::vector<std::string> tok;
    std::string delim;
    int i = 0;
    while (i < flen && is_delim(first[i])) i++;
    while (i < flen) {
        int j = i;
        while (j < flen && !is_delim(first[j])) j++;
        tok.emplace_back((const char*)first + i, (size_t)(j - i));
        if (j < flen) delim.push_back((char)first[j]);
        while (j < flen && is_delim(first[j])) j++;
        i = j;
    }
    std::vector<uint64_t> val(tok.size(), 0);
    for (size_t k = 0; k < tok.size(); k++)
        if (k + 2 < 512 && T[k + 2] == 1) val[k] = strtoull(tok[k].c_str(), nullptr, 10);
    const int pet = T[1];
    used = 0;
    auto put = [&](const std::string& s, uint32_t r) {
        if (used + s.size() > cap || s.size() > 0xffff) return false;
        memcpy(names + used, s.data(), s.size());
        used += s.size();
        nl[r] = (uint16_t)s.size();
        return true;
    };
    auto assemble = [&](uint32_t idx) {
        std::string s;
        for (size_t k = 0; k < tok.size(); k++) {
            const int ty = k + 2 < 512 ? T[k + 2] : 0;
            if (ty == 1) s += std::to_string(val[k] + (pet ? idx / 2 : idx));
            else if (ty == 3) s += std::to_string(lens[idx]);
            else if (ty == 0) s += tok[k];
            if (k + 1 < tok.size() && k < delim.size()) s += delim[k];
        }
        return s;
    };
    if (!pet) {
        for (uint32_t r = 0; r < n; r++)
            if (!put(assemble(r), r)) return false;
        return true;
    }
    for (uint32_t r = 0; r < n; r += 2) {
        const std::string a = assemble(r);
        if (!put(a, r)) return false;
        if (r + 1 >= n) break;
        std::string b = a;
        if (pet == 2 && !b.empty()) b.back() = '2';
        else if (pet == 3) {
            const char last = delim.empty() ? ' ' : delim.back();
            const size_t at = a.rfind(last);
            b = a.substr(0, at == std::string::npos ? 0 : at + 1) + std::to_string(lens[r + 1]);
        }
        if (!put(b, r + 1)) return false;
    }
    return true;
}

const char kIupac[] = "NMRYKSWHBVD";   // base codes 4..14 (seq_val_table@0x44b800)

// one SIMPLE_MODEL<nsym> stream of `n` symbols (compressOrder@0x424b70 and
// the compressAlignInfo_* family): setID(id), size4, the coded bytes
inline bool sm_stream(Cursor& c, int id, int nsym, uint32_t n, std::vector<uint8_t>& out)
{
    if (!c.id(id)) return false;
    const uint32_t sz = c.size4();
    if (c.bad) return false;
    out.assign(n, 0);
    if (nsym > 0) {
        SModel m;
        m.reset(nsym);
        RangeIn rc(c.p, c.p + sz);
        for (uint32_t i = 0; i < n; i++) out[i] = (uint8_t)m.decode(rc);
        if (rc.bad) return false;
    }
    c.p += sz;
    return true;
}

inline bool count_encap(Cursor& c, int id, uint32_t& v)   // compressCount@0x422a00
{
    if (!c.id(id) || c.end - c.p < 5 || c.p[0] != 0x84) return false;
    v = le32(c.p + 1);
    c.p += 5;
    return true;
}

// the read type the encoder wrote for a substitution (@0x44a0c0, [ref * 4 + read])
const uint8_t kMisType[16] = {3, 1, 0, 2, 1, 3, 0, 2, 1, 0, 3, 2, 2, 1, 0, 3};

// mapvar2base@0x40db20: the read base of mismatch type t over reference base b
// (type 3: an N / IUPAC base, restored from the side streams)
inline uint32_t var2base(uint32_t b, uint32_t t)
{
    if (t >= 3) return 4;
    for (uint32_t x = 0; x < 4; x++)
        if (x != b && kMisType[b * 4 + x] == t) return x;
    return 4;
}

// ---- the parts of a block that are small per-read or per-N work: both
//      sa_decode_block and dec_prepass call these ----

// the block's opening encap and its read count (compressCount@0x422a00); c.end becomes the block's end
inline bool dec_open(Cursor& c, uint32_t& n)
{
    if (!c.id(1)) return false;
    const uint32_t bsize = c.size4();
    if (c.bad) return false;
    c.end = c.p + bsize;
    if (!c.id(1) || c.end - c.p < 5 || c.p[0] != 0x84) return false;
    n = le32(c.p + 1);
    c.p += 5;
    return true;
}

// lengths: compressLen_short@0x423f50 / compressLen_long@0x423710
inline bool dec_lengths(Cursor& c, int32_t long_reads, uint32_t n, std::vector<uint32_t>& len)
{
    if (!c.id(4)) return false;
    const uint32_t sz = c.size4();
    if (c.bad) return false;
    SModel same, by[4];
    same.reset(2);
    for (auto& m : by) m.reset(256);
    RangeIn rc(c.p, c.p + sz);
    const int nbytes = long_reads ? 4 : 2;
    for (uint32_t r = 0; r < n; r++) {
        if (same.decode(rc)) { len[r] = 0; continue; }
        uint32_t v = 0;
        for (int k = 0; k < nbytes; k++) v |= (uint32_t)by[k].decode(rc) << (8 * k);
        len[r] = v;
    }
    if (rc.bad) return false;
    c.p += sz;
    return true;
}

// IDs: compressID@0x4247c0 (o->seq_lens must hold the lengths: ID-bin names quote them)
inline bool dec_names(Cursor& c, const sa_cfg* cfg, const uint8_t tmpl[512], sa_decoded* o, uint32_t n, uint8_t dg_id[16],
                      uint64_t& name_total)
{
    name_total = 0;
    if (!c.id(5)) return false;
    const uint32_t sz = c.size4();
    if (c.bad) return false;
    const uint8_t* q = c.p;
    const uint8_t* qe = c.p + sz;
    if (cfg->md5) { if (qe - q < 16) return false; memcpy(dg_id, q, 16); q += 16; }
    if (cfg->bin_mode) {
        if (qe - q < 2) return false;
        const int fl = q[0] | q[1] << 8;
        if (qe - q < 2 + fl) return false;
        if (!bin_names(q + 2, fl, tmpl, o->seq_lens, n, o->names, o->name_cap, o->name_lens, name_total)) return false;
    } else {
        NameDecoder nd;
        RangeIn rc(q, qe);
        for (uint32_t r = 0; r < n; r++) {
            const uint64_t room = o->name_cap - name_total;
            const int l = nd.decode(rc, o->names + name_total, room > 255 ? 255 : (int)room);
            if (l < 0) return false;
            o->name_lens[r] = (uint16_t)l;
            name_total += (uint64_t)l;
        }
        if (rc.bad) return false;
    }
    c.p += sz;
    return true;
}

// N / IUPAC side streams (DegeInfoProcess@0x433a10): 23 tip, 14 chars,
// 24 max quality, 25 exception counts, 26 gaps (25 and 26 share one kModel)
struct DecSide {
    std::vector<uint8_t> tip, chs, maxq;
    std::vector<uint64_t> exc, gaps;
};
inline bool dec_side(Cursor& c, uint32_t n, DecSide& s)
{
    s.tip.assign(n, 0);
    KModel km;
    km.reset();
    uint32_t ntip = 0;
    const int ids[5] = {23, 14, 24, 25, 26};
    for (int k = 0; k < 5; k++) {
        if (!c.id(ids[k])) continue;   // omitted when empty
        const uint32_t sz = c.size4();
        if (c.bad || sz < 4) return false;
        const uint32_t cnt = le32(c.p);
        RangeIn rc(c.p + 4, c.p + sz);
        if (ids[k] == 23) {
            SModel m;
            m.reset(2);
            for (uint32_t i = 0; i < cnt && i < n; i++) ntip += s.tip[i] = (uint8_t)m.decode(rc);
        } else if (ids[k] == 14 || ids[k] == 24) {
            SModel m;
            m.reset(ids[k] == 14 ? 11 : 95);
            std::vector<uint8_t>& v = ids[k] == 14 ? s.chs : s.maxq;
            v.resize(cnt);
            for (uint32_t i = 0; i < cnt; i++) v[i] = (uint8_t)m.decode(rc);
        } else {
            std::vector<uint64_t>& v = ids[k] == 25 ? s.exc : s.gaps;
            v.resize(cnt);
            for (uint32_t i = 0; i < cnt; i++) v[i] = km.decode(rc);
        }
        if (rc.bad) return false;
        c.p += sz;
    }
    return s.maxq.size() == ntip && s.exc.size() == ntip;
}

// blockMd5Verify@0x414e00: 1 when the stored digests match the decoded streams
inline int32_t dec_md5_verify(const sa_decoded* o, uint64_t name_total, uint64_t total, bool md5_q, const uint8_t dg_id[16],
                              const uint8_t dg_q[16], const uint8_t dg_s[16])
{
    int32_t ok = 1;
    uint8_t dg[16];
    md5(o->names, name_total, dg);
    if (memcmp(dg, dg_id, 16)) ok = 0;
    if (md5_q) {
        md5(o->qual, total, dg);
        if (memcmp(dg, dg_q, 16)) ok = 0;
    }
    md5(o->seq, total, dg);
    if (memcmp(dg, dg_s, 16)) ok = 0;
    return ok;
}

// ---- the pre-pass of a chain-per-block decoder: everything of a no-reference block but
//      the QUAL and SEQ chains, whose payloads are only located ----
struct DecPre {
    uint32_t n = 0;
    uint64_t total = 0, name_total = 0;
    std::vector<uint32_t> len;
    uint8_t dg_id[16], dg_q[16], dg_s[16];
    const uint8_t *qual = nullptr, *seq = nullptr;   // the coded bytes (after the digest)
    uint32_t qual_len = 0, seq_len = 0;
    DecSide side;
    // the tip reads, in order: offset of the read in the block's bases, its length
    std::vector<uint64_t> tip_off;
    std::vector<uint32_t> tip_len;
};

// one coder payload: id, size4, [digest], bytes
inline bool dec_locate(Cursor& c, int id, bool digest, uint8_t dg[16], const uint8_t*& p, uint32_t& len)
{
    if (!c.id(id)) return false;
    const uint32_t sz = c.size4();
    if (c.bad || (digest && sz < 16)) return false;
    if (digest) memcpy(dg, c.p, 16);
    p = c.p + (digest ? 16 : 0);
    len = sz - (digest ? 16u : 0u);
    c.p += sz;
    return true;
}

// false: the encap walk or one of the small streams failed (sa_decode_block returns -1 there too)
inline bool dec_prepass(const uint8_t* in, uint64_t in_len, const sa_cfg* cfg, const uint8_t tmpl[512], int32_t long_reads,
                        sa_decoded* o, DecPre& pre)
{
    Cursor c{in, in + in_len};
    if (!dec_open(c, pre.n) || pre.n > o->max_reads) return false;
    const uint32_t n = pre.n;
    o->nreads = n;
    pre.len.assign(n, 0);
    if (!dec_lengths(c, long_reads, n, pre.len)) return false;
    pre.total = 0;
    for (uint32_t r = 0; r < n; r++) { o->seq_lens[r] = (int32_t)pre.len[r]; pre.total += pre.len[r]; }
    if (pre.total > o->seq_cap) return false;
    if (!dec_names(c, cfg, tmpl, o, n, pre.dg_id, pre.name_total)) return false;
    const bool md5_q = cfg->md5 && !(cfg->lossy > 0.0);
    if (!dec_locate(c, 7, md5_q, pre.dg_q, pre.qual, pre.qual_len)) return false;
    if (!dec_side(c, n, pre.side)) return false;
    if (!dec_locate(c, 6, cfg->md5 != 0, pre.dg_s, pre.seq, pre.seq_len)) return false;
    if (c.p != c.end) return false;
    pre.tip_off.clear();
    pre.tip_len.clear();
    uint64_t at = 0;
    for (uint32_t r = 0; r < n; r++) {
        if (pre.side.tip[r]) { pre.tip_off.push_back(at); pre.tip_len.push_back(pre.len[r]); }
        at += pre.len[r];
    }
    return true;
}

}  // namespace sadh
