"""A DEFLATE writer for tests: streams that Python's zlib (the only encoder behind
the other fixtures) never emits, built symbol by symbol and checked by zlib's
inflate before anything of ours is asked.  Used by tests/test_deflate_forge.py
(the host emulations) and tests/test_gpu_deflate_forge.py (the kernels).

A stream is a list of blocks; a block is a type (stored, fixed, dynamic), a
token list and a final flag.  A token is a literal byte (an int) or a match
(length, distance), or (length, distance, length symbol) where the symbol is
not the canonical one (258 as symbol 284 with all extra bits set).  Stream
renders the tokens into the text as it writes them, so a fixture's expected
bytes come from its tokens and zlib only has to agree.

The three corpora: valid(), invalid() and seeded(); gz_streams() and gz_invalid()
for the gzip path.  Each list asserts, while it is built, that zlib accepts or
rejects every stream as intended and that the property a fixture is named for
can be read back from its bytes."""
import bisect
import functools
import heapq
import zlib

import numpy as np

import test_inflate as ti
from test_inflate import E_CODES, E_INPUT, E_SIZE, BitWriter, dynamic_code_lengths

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_XB = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_XB = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in range(2))
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EOB = 256
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
_LEN_SYM = [0] * 259
for _s in range(28):
    for _l in range(LEN_BASE[_s], LEN_BASE[_s] + (1 << LEN_XB[_s])):
        if _l <= 258:
            _LEN_SYM[_l] = 257 + _s
_LEN_SYM[258] = 285


def len_sym(length):
    return _LEN_SYM[length]


def dist_sym(dist):
    return bisect.bisect_right(DIST_BASE, dist) - 1


def len_max(sym):
    """The longest length symbol `sym` writes (all its extra bits set)."""
    return LEN_BASE[sym - 257] + (1 << LEN_XB[sym - 257]) - 1


def dist_max(ds):
    return DIST_BASE[ds] + (1 << DIST_XB[ds]) - 1


# ---- codes -------------------------------------------------------------------
def kraft(lens):
    """The set's Kraft sum in units of 2^-15: 32768 is a complete set."""
    return sum(1 << (15 - l) for l in lens if l)


def canon(lens):
    """{symbol: (the canonical code's bits reversed, for BitWriter.bits, its length)} (RFC 1951, 3.2.2)."""
    out, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[s] = (int(format(code, f"0{ln}b")[::-1], 2), ln)
                code += 1
        code <<= 1
    return out


def limited_lengths(freq, limit):
    """Huffman code lengths of the symbols with a frequency, no code longer than
    `limit`: Huffman's lengths cut at the limit, then the longest codes below the
    limit are lengthened until the set fits and the cheapest shortened until it
    is complete.  One symbol gets one 1-bit code (an incomplete set)."""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) <= 2:
        for s in used:
            lens[s] = 1
        return lens
    assert len(used) <= 1 << limit
    heap = [(freq[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    for s in used:
        lens[s] = min(lens[s], limit)
    full = 1 << limit
    k = sum(1 << (limit - lens[s]) for s in used)
    while k > full:
        s = max((s for s in used if lens[s] < limit), key=lambda s: (lens[s], -freq[s]))
        k -= 1 << (limit - lens[s] - 1)
        lens[s] += 1
    while k < full:
        s = max((s for s in used if (1 << (limit - lens[s])) <= full - k), key=lambda s: (lens[s], freq[s]))
        k += 1 << (limit - lens[s])
        lens[s] -= 1
    return lens


def skew_lengths(freq, chosen, limit):
    """A complete set in which the symbols `chosen` (one or two) own codes of
    `limit` bits, the longest of the set.  The longest codes of a complete set
    come in pairs: one chosen symbol gets the rarest other one as its partner.
    The other symbols share what is left, 1 - 2^-(limit-1) = 2^-1 + ... +
    2^-(limit-1): one code of each of those lengths, the shortest split in two
    until there is one for each symbol, the frequent symbols first.  Symbols
    that do not occur are given codes where the alphabet in use is too small."""
    n = len(freq)
    chosen = list(chosen)
    rest = [s for s in range(n) if freq[s] and s not in chosen]
    spare = [s for s in range(n) if not freq[s] and s not in chosen]
    if len(chosen) == 1:
        if len(rest) >= limit:
            partner = min(rest, key=lambda s: (freq[s], s))
            rest.remove(partner)
        else:
            partner = spare.pop(0)
        chosen.append(partner)
    while len(rest) < limit - 1:
        rest.append(spare.pop(0))
    have = list(range(1, limit))
    while len(have) < len(rest):
        have.sort()
        k = have.pop(0)
        assert k < limit
        have += [k + 1, k + 1]
    have.sort()
    lens = [0] * n
    for s, l in zip(sorted(rest, key=lambda s: (-freq[s], s)), have):
        lens[s] = l
    for s in chosen:
        lens[s] = limit
    assert kraft(lens) == 32768 and max(lens) == limit
    return lens


def chain_lengths(n, start):
    """n >= 2 lengths start, start + 1, ..., whose Kraft sum is 2^-(start - 1)."""
    return [start + i for i in range(n - 1)] + [start + n - 2]


# ---- the code-length encoding of a dynamic header ------------------------------
def cl_items(seq, rle=True):
    """The literal/length and distance lengths, one run, as code-length symbols:
    [(symbol, extra value, index of the first length it writes, how many)].
    rle: the repeats 16 / 17 / 18 used greedily (the longest first), over the
    boundary between the alphabets too; otherwise every length on its own."""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        run = 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if not rle:
            out.append((v, 0, i, 1))
            i += 1
            continue
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11, i, take) if take >= 11 else (17, take - 3, i, take))
            i += take
            continue
        out.append((v, 0, i, 1))
        i += 1
        run -= 1
        while v and run >= 3:
            take = min(run, 6)
            out.append((16, take - 3, i, take))
            i += take
            run -= take
    return out


def min_hclen(cl_lens):
    return max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))


class Stream:
    """One raw-deflate stream being written: .w the bits, .data the text so far,
    .dyn the bit offset of every dynamic block, .hdr what the last dynamic header used."""

    def __init__(self, history: bytes = b""):
        self.w = BitWriter()
        self.data = bytearray()
        self.dyn = []
        self.hdr = None
        if history:
            for i in range(0, len(history), 0xffff):
                self.stored(history[i:i + 0xffff])

    def bitlen(self):
        return len(self.w.out) * 8 + self.w.n

    def done(self):
        return self.w.done(), bytes(self.data)

    def render(self, tokens):
        d = self.data
        for t in tokens:
            if isinstance(t, int):
                d.append(t)
                continue
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= min(32768, len(d)), t
            if dist >= length:
                d += d[len(d) - dist:len(d) - dist + length]
            else:
                for _ in range(length):
                    d.append(d[-dist])

    def emit(self, tokens, lc, dc):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.bits(*lc[t])
                continue
            length, dist = t[0], t[1]
            ls = t[2] if len(t) > 2 else _LEN_SYM[length]
            w.bits(*lc[ls])
            if LEN_XB[ls - 257]:
                assert 0 <= length - LEN_BASE[ls - 257] < 1 << LEN_XB[ls - 257]
                w.bits(length - LEN_BASE[ls - 257], LEN_XB[ls - 257])
            ds = dist_sym(dist)
            w.bits(*dc[ds])
            if DIST_XB[ds]:
                w.bits(dist - DIST_BASE[ds], DIST_XB[ds])
        w.bits(*lc[EOB])

    def stored(self, payload: bytes, final=False):
        assert len(payload) <= 0xffff
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(payload), 16)
        self.w.bits(len(payload) ^ 0xffff, 16)
        self.w.out += payload
        self.data += payload
        return self

    def fixed(self, tokens, final=False):
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        self.emit(tokens, _FIXED_LC, _FIXED_DC)
        self.render(tokens)
        return self

    def raw_header(self, final, hlit_field, hdist_field, cl_lens, hclen, items):
        """A dynamic block's header from its field values as they are: HLIT and
        HDIST fields of any value, any code-length code, any item sequence."""
        w = self.w
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(hlit_field, 5)
        w.bits(hdist_field, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canon(cl_lens)
        for it in items:
            w.bits(*cc[it[0]])
            if it[0] >= 16:
                w.bits(it[1], (2, 3, 7)[it[0] - 16])

    def dynamic(self, tokens, final=False, ll=None, dl=None, limit=15, skew_l=None, skew_d=None, hlit=None, hdist=None,
                hclen=None, rle=True, cl_skew=False):
        """A dynamic block.  ll / dl: explicit code lengths (by symbol; shorter
        lists are padded); otherwise from the tokens' frequencies, no code longer
        than `limit`, with skew_l / skew_d: those symbols own `limit`-bit codes.
        hlit / hdist: how many lengths the header carries (default: up to the
        last code).  hclen: default the minimum.  cl_skew: the code-length code
        has a 7-bit code."""
        lf, df = [0] * 286, [0] * 30
        lf[EOB] = 1
        for t in tokens:
            if isinstance(t, int):
                lf[t] += 1
            else:
                lf[t[2] if len(t) > 2 else _LEN_SYM[t[0]]] += 1
                df[dist_sym(t[1])] += 1
        if ll is None:
            lim = max(limit, (sum(1 for f in lf if f) - 1).bit_length())
            ll = skew_lengths(lf, skew_l, limit) if skew_l else limited_lengths(lf, lim)
        if dl is None:
            dl = skew_lengths(df, skew_d, limit) if skew_d else limited_lengths(df, max(limit, 5)) if any(df) else [0]
        ll = list(ll) + [0] * (286 - len(ll))
        dl = list(dl) + [0] * (30 - len(dl))
        hlit = hlit or max(257, max(i + 1 for i in range(286) if ll[i]))
        hdist = hdist or max(1, max([i + 1 for i in range(30) if dl[i]], default=1))
        assert not any(ll[hlit:]) and not any(dl[hdist:])
        ll, dl = ll[:hlit], dl[:hdist]
        items = cl_items(ll + dl, rle)
        cf = [0] * 19
        for it in items:
            cf[it[0]] += 1
        if cl_skew:
            cl_lens = skew_lengths(cf, [min((s for s in range(19) if cf[s]), key=lambda s: (cf[s], s))], 7)
        else:
            cl_lens = limited_lengths(cf, 7)
            if sum(1 for l in cl_lens if l) == 1:   # (the code-length code must be complete: a second, unused code)
                cl_lens[[s for s in (0, 8) if not cl_lens[s]][0]] = 1
        hclen = hclen or min_hclen(cl_lens)
        assert min_hclen(cl_lens) <= hclen <= 19
        self.dyn.append(self.bitlen())
        self.hdr = dict(hlit=hlit, hdist=hdist, hclen=hclen, items=items, cl_lens=cl_lens, ll=ll, dl=dl)
        self.raw_header(final, hlit - 257, hdist - 1, cl_lens, hclen, items)
        self.emit(tokens, canon(ll), canon(dl))
        self.render(tokens)
        return self


_FIXED_LC, _FIXED_DC = canon(FIXED_LL), canon(FIXED_DL)


def lens_at(cd: bytes, bit: int):
    """dynamic_code_lengths of the dynamic block that starts at that bit of cd."""
    return dynamic_code_lengths((int.from_bytes(cd, "little") >> bit).to_bytes(len(cd), "little") + b"\0\0")


# ---- the tokeniser -------------------------------------------------------------
class Tokeniser:
    """A greedy hash-chain tokeniser over one text.  tokens(start, end, ...) are
    the tokens of text[start:end): a match may reach back before `start`, across
    any number of earlier blocks (whatever their type), and is cut at `end`,
    where zlib would have gone on.  Positions are entered into the chains in
    order, so the ranges must be asked for in order (skip() enters a range that
    gets no tokens: a stored block's)."""

    def __init__(self, text: bytes):
        self.text = text
        self.heads = {}
        self.at = 0

    def _enter(self, upto):
        t, h = self.text, self.heads
        for i in range(self.at, min(upto, len(t) - 2)):
            h.setdefault(t[i:i + 3], []).append(i)
        self.at = max(self.at, upto)

    def skip(self, start, end):
        self._enter(end)

    def tokens(self, start, end, min_len=3, max_len=258, max_dist=32768, chain=6):
        t, out, i = self.text, [], start
        while i < end:
            self._enter(i)
            best, bdist = 0, 0
            lim = min(max_len, end - i)
            if lim >= min_len:
                cands = self.heads.get(t[i:i + 3], ())
                for p in cands[:-chain - 1:-1]:
                    if i - p > max_dist:
                        break
                    if best and t[p + best] != t[i + best]:
                        continue
                    n = 0
                    while n < lim and t[p + n] == t[i + n]:
                        n += 1
                    if n > best:
                        best, bdist = n, i - p
                        if n == lim:
                            break
            if best >= min_len:
                out.append((best, bdist))
                i += best
            else:
                out.append(t[i])
                i += 1
        return out


def forge(text: bytes, cuts, types, **kw):
    """text as blocks cut at `cuts` (ends; the last is len(text)) of `types` ('s',
    'f', 'd' in turn), tokenised with the parameters in kw; dynamic blocks take
    kw's `dyn` (a dict, or a function of the block index)."""
    dyn = kw.pop("dyn", {})
    tk, s, start = Tokeniser(text), Stream(), 0
    for bi, end in enumerate(cuts):
        ty, final = types[bi % len(types)], end == cuts[-1] and bi == len(cuts) - 1
        if ty == "s":
            assert end - start <= 0xffff
            tk.skip(start, end)
            s.stored(text[start:end], final)
        else:
            toks = tk.tokens(start, end, **kw)
            if ty == "f":
                s.fixed(toks, final)
            else:
                s.dynamic(toks, final, **(dyn(bi) if callable(dyn) else dyn))
        start = end
    cd, data = s.done()
    assert data == text
    return cd, s


# ---- zlib's verdict ------------------------------------------------------------
def zlib_says(cd):
    """'ok' (the stream ends, with its text), 'short' (zlib wants more input) or 'error'."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(cd) + d.flush()
    except zlib.error:
        return "error", None
    return ("ok", out) if d.eof else ("short", None)


def _check_valid(out, not_bgzf=()):
    names = [v[0] for v in out]
    assert len(set(names)) == len(names)
    for name, cd, data in out:
        assert zlib_says(cd) == ("ok", data), name
        assert len(data) <= 65536, name
        assert name in not_bgzf or len(cd) + 26 <= 65536, name


def _check_invalid(out):
    """E_INPUT: zlib reads to the end of the bytes and wants more; E_SIZE with ISIZE 0:
    zlib inflates the stream, to more than no bytes; every other status: zlib raises."""
    names = [v[0] for v in out]
    assert len(set(names)) == len(names)
    for name, cd, isize, crc, want in out:
        how, text = zlib_says(cd)
        if want == E_INPUT:
            assert how == "short", (name, how)
        elif want == E_SIZE:
            assert how == "ok" and len(text) != isize, (name, how)
        else:
            assert how == "error", (name, how)
        assert ti.zlib_verdict(cd, isize, crc) is None, name


# ---- the valid members -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text():
    return ti._texts()[0]


def _probe_tokens(base: bytes, pairs):
    """base as literals' worth of history is the caller's; here: four literals
    between the matches (length, distance[, length symbol]) of `pairs`."""
    out = []
    for i, p in enumerate(pairs):
        out += list(base[4 * i % (len(base) - 4):][:4])
        out.append(p)
    return out


def _all_symbol_pairs():
    """Every length symbol and every distance code with its extra bits all-zero
    and all-one: 60 matches (258 also as symbol 284 with extra 31)."""
    lens = []
    for s in range(257, 286):
        lens.append((LEN_BASE[s - 257], s))
        lens.append((min(len_max(s), 258), s))
    dists = []
    for ds in range(30):
        dists += [DIST_BASE[ds], dist_max(ds)]
    return [(lens[i % len(lens)][0], dists[i], lens[i % len(lens)][1]) for i in range(len(dists))]


def _ends_on_last_bit(build):
    """build(k, j) -> Stream with k and j fillers of two kinds: the first whose
    bit length is a multiple of 8, so that the final end-of-block code's last bit
    is the last bit of the last byte."""
    for k in range(16):
        for j in range(16):
            s = build(k, j)
            if s.bitlen() % 8 == 0:
                return s
    raise AssertionError("no filler count ends the stream on a byte boundary")


# the symbols that own a 15-bit code in a fixture of their own, with a match that uses them
L15 = {"eob": EOB, "len257": 257, "len264": 264, "len265": 265, "len284": 284, "len285": 285}
D15 = {"dist0": 0, "dist3": 3, "dist4": 4, "dist28": 28, "dist29": 29}
_L15_MATCH = {257: (3, 7), 264: (10, 9), 265: (12, 33), 284: (257, 100), 285: (258, 1000)}
_D15_MATCH = {0: (5, 1), 3: (9, 4), 4: (20, 6), 28: (40, 24576), 29: (258, 32768)}


@functools.lru_cache(maxsize=None)
def valid():
    """[(name, deflate bytes, text)].  Every comment names what zlib never writes."""
    tx = text()
    hist = tx[:32768]
    out = []

    def add(name, s):
        cd, data = s.done() if isinstance(s, Stream) else s
        out.append((name, cd, data))
        return cd

    def maxlens(s, cd, k=0):
        ll, dl = lens_at(cd, s.dyn[k])
        return max(ll), max(dl), ll, dl

    # a common body for the code-shape fixtures: tokenised text behind a stored block, then matches that use
    # every length and distance class, so that whichever symbol is skewed occurs
    tk = Tokeniser(tx[:40000])
    tk.skip(0, 32768)
    body = tk.tokens(32768, 36000) + _probe_tokens(tx[50000:50400], list(_L15_MATCH.values()) + list(_D15_MATCH.values()))
    # literal, length and distance codes of every maximum length 11 .. 15: the canonical walk behind both primary tables
    for L in range(11, 16):
        s = Stream(hist).dynamic(body, True, limit=L, skew_l=[ord("N"), 285], skew_d=[29])
        cd = add(f"maxlen_{L}", s)
        ml, md, ll, dl = maxlens(s, cd)
        assert (ml, md) == (L, L) and ll[ord("N")] == ll[285] == L and dl[29] == L
    # a 15-bit code on the end-of-block code, on length symbols and on distance codes, one at a time
    for name, sym in L15.items():
        s = Stream(hist).dynamic(body, True, skew_l=[sym])
        cd = add(f"l15_{name}", s)
        ml, _, ll, _ = maxlens(s, cd)
        assert ml == 15 and ll[sym] == 15
    for name, ds in D15.items():
        s = Stream(hist).dynamic(body, True, skew_d=[ds])
        cd = add(f"d15_{name}", s)
        _, md, _, dl = maxlens(s, cd)
        assert md == 15 and dl[ds] == 15
    # every length symbol and every distance code, extra bits all-zero and all-one, fixed and dynamic coding
    every = _probe_tokens(tx[40000:40400], _all_symbol_pairs())
    used_l = {t[2] for t in every if not isinstance(t, int)}
    used_d = {dist_sym(t[1]) for t in every if not isinstance(t, int)}
    assert used_l == set(range(257, 286)) and used_d == set(range(30))
    add("every_symbol_fixed", Stream(hist).fixed(every, True))
    add("every_symbol_dynamic", Stream(hist).dynamic(every, True))
    # distance alphabets: one 1-bit code in use (code 0, code 29), none, two, all 30
    lits = list(tx[100:160])
    s = Stream().dynamic(lits + [(30, 1)] + lits[:5] + [(3, 1)], True, dl=[1])
    cd = add("dist_single_code0", s)
    assert lens_at(cd, 0)[1] == [1]
    s = Stream(hist).dynamic(lits + [(30, 24577)] + lits[:5] + [(258, 32768)], True, dl=[0] * 29 + [1])
    cd = add("dist_single_code29", s)
    assert lens_at(cd, s.dyn[0])[1] == [0] * 29 + [1]
    s = Stream().dynamic(list(tx[:3000]), True)
    cd = add("dist_none", s)
    assert lens_at(cd, 0)[1] == [0]
    s = Stream().dynamic(lits + [(7, 2), (9, 33)] * 5, True)
    cd = add("dist_two_codes", s)
    assert sorted(l for l in lens_at(cd, 0)[1] if l) == [1, 1]
    s = Stream(hist).dynamic(body, True, dl=[4, 4] + [5] * 28)
    cd = add("dist_all_30", s)
    assert lens_at(cd, s.dyn[0])[1] == [4, 4] + [5] * 28
    # literal alphabets: one literal and the end-of-block code; all 256 literals and all 29 lengths (HLIT 286, HDIST 30)
    s = Stream().dynamic([65] * 50, True)
    cd = add("lit_two_codes", s)
    assert [l for l in lens_at(cd, 0)[0] if l] == [1, 1] and s.hdr["hlit"] == 257
    s = Stream(hist).dynamic(list(range(256)) + every, True, ll=[8] * 226 + [9] * 60, dl=[4, 4] + [5] * 28)
    cd = add("hlit_286_hdist_30", s)
    ll, dl = lens_at(cd, s.dyn[0])
    assert len(ll) == 286 and len(dl) == 30 and all(ll) and all(dl)
    # header shapes.  HCLEN: 5 is the least a valid block can have (the first four code-length symbols are
    # 16, 17, 18 and 0, and the end-of-block code needs a length that is not 0): 256 codes of 8 bits
    s = Stream().dynamic(list(tx[:200]), True, ll=[8] * 255 + [0, 8])
    cd = add("hclen_min", s)
    assert s.hdr["hclen"] == 5 and int.from_bytes(cd[:3], "little") >> 13 & 15 == 1
    s = Stream().dynamic(list(tx[:200]) + [(5, 3)], True, hclen=19)
    cd = add("hclen_19", s)
    assert int.from_bytes(cd[:3], "little") >> 13 & 15 == 15
    # repeats at their least and greatest counts: 16 x 3 and x 6, 17 x 3 and x 10, 18 x 11 and x 138
    ll = [0] * 257
    for sym, l in ((138, 4), (150, 4), (161, 5), (169, 2), (EOB, 5)):
        ll[sym] = l
    ll[165:169] = [5] * 4
    ll[170:177] = [4] * 7
    s = Stream().dynamic([138, 150, 161, 165, 166, 167, 168, 169, 170, 173, 176] * 9, True, ll=ll)
    add("repeat_counts", s)
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= {it[:2] for it in s.hdr["items"]}
    # one zero run from the last literal/length lengths into the first distance lengths
    s = Stream().dynamic(lits + [(4, 9), (5, 40), (6, 30)] * 3, True, hlit=286)
    add("repeat_crosses_alphabets", s)
    assert any(it[0] >= 17 and it[2] < 286 < it[2] + it[3] for it in s.hdr["items"])
    s = Stream().dynamic(lits + [(4, 9), (5, 40), (6, 30)] * 3, True, rle=False)
    add("no_repeats", s)
    assert all(it[0] < 16 for it in s.hdr["items"])
    s = Stream(hist).dynamic(body, True, cl_skew=True)
    add("cl_code_7_bits", s)
    assert max(s.hdr["cl_lens"]) == 7
    # block sequences
    add("empty_final_fixed", Stream().dynamic(body[:0] + list(tx[:500]), False).fixed([], True))
    s = Stream()
    for m in range(8):   # 10 + 9 m bits: the stored block's header at every bit of a byte
        s.fixed(list(tx[m * 10:m * 10 + 3]) + [0x90 + m] * m)
        assert s.bitlen() % 8 == (2 + m) % 8
        s.stored(b"")
    add("empty_stored_8_alignments", s.fixed(list(tx[:4]), True))
    s = Stream().dynamic([], False).fixed(list(tx[:100]), False).dynamic([], True)
    cd = add("empty_dynamic", s)
    assert [l for l in lens_at(cd, 0)[0] if l] == [1]
    tk = Tokeniser(tx)
    toks = tk.tokens(0, 60000, max_len=6)[:12000]
    s = Stream()
    for b in range(300):
        part = toks[b * 40:b * 40 + 40]
        if b % 3 == 0:
            tmp = Stream()
            tmp.data = bytearray(s.data)
            tmp.render(part)
            s.stored(bytes(tmp.data[len(s.data):]), b == 299)
        elif b % 3 == 1:
            s.fixed(part, b == 299)
        else:
            s.dynamic(part, b == 299, limit=7 + b % 9)
    add("blocks_300x40", s)
    assert len(s.dyn) == 100 and s.done()[1] == tx[:len(s.data)]
    add("stored_ffff", Stream().stored(tx[:0xffff], True))
    s = Stream()
    at = 0
    for ty in "sffddfsd":   # stored -> fixed -> fixed -> dynamic -> dynamic -> fixed, stored -> dynamic
        if ty == "s":
            s.stored(tx[at:at + 300])
        else:
            toks = list(tx[at:at + 20]) + [(40, 310), (258, 200)] + list(tx[at + 20:at + 30])   # 310 back: the previous block
            s.fixed(toks) if ty == "f" else s.dynamic(toks)
        at += 300
    add("matches_across_block_types", s.fixed([], True))
    # overlapping matches: the lane-split copy's src[i mod dist] edges; the last match ends the member
    over = [(ln, d) for d in (1, 2, 3, 63, 64, 65) for ln in (3, 64, 65, 258)]
    add("overlaps_fixed", Stream().fixed(list(tx[:65]) + _probe_tokens(tx[200:400], over)[:-1] + [(258, 64)], True))
    add("overlaps_dynamic", Stream().dynamic(list(tx[:65]) + _probe_tokens(tx[200:400], over)[:-1] + [(258, 65)], True))
    # the end of the input: the final end-of-block code of 1, 2, 7 and 15 bits ends on the last bit of the last
    # byte; and behind a match whose distance extra bits are all ones
    a, c, g, t_ = b"ACGT"
    syms = [a, c, g, t_, 259]   # (259: length 5)
    shapes = {1: dict(zip([EOB] + syms, [1] + chain_lengths(5, 2))),
              2: dict(zip([a, EOB] + syms[1:], [1, 2] + chain_lengths(4, 3)))}
    for e in (1, 2, 7, 15):
        for tail in ("lit", "match"):
            def build(k, j, e=e, tail=tail):
                toks = [a, c, g, t_] * 3 + [c] * k + [g] * j + ([(5, 6)] if tail == "match" else [])
                if e == 7:
                    toks = [0x90 if x == g else x for x in toks]   # (a 9-bit literal: the fixed code's other lengths are even)
                    return Stream().fixed(toks, True)
                if e == 15:
                    return Stream().dynamic(toks, True, skew_l=[EOB])
                ll = [0] * 260
                for sym, l in shapes[e].items():
                    ll[sym] = l
                return Stream().dynamic(toks, True, ll=ll)
            s = _ends_on_last_bit(build)
            cd = add(f"ends_on_last_bit_eob{e}_{tail}", s)
            assert len(cd) * 8 == s.bitlen()
            if e != 7:
                assert lens_at(cd, 0)[0][EOB] == e
    # members of 2 .. 9 bytes, around the 8-byte refill (one byte is too short for any stream: invalid())
    for n in range(2, 10):
        cd = add(f"in_len_{n}_fixed", Stream().fixed(list(tx[:n - 2]), True))
        assert len(cd) == n
    for n in range(5, 10):
        cd = add(f"in_len_{n}_stored", Stream().stored(tx[:n - 5], True))
        assert len(cd) == n
    _check_valid(out, not_bgzf=("stored_ffff",))
    return out


END_CASES = tuple(f"ends_on_last_bit_eob{e}_{t}" for e in (1, 2, 7, 15) for t in ("lit", "match")) + \
    tuple(f"in_len_{n}_fixed" for n in range(2, 10)) + tuple(f"in_len_{n}_stored" for n in range(5, 10))


# ---- the invalid members -----------------------------------------------------------
def _bad_header(hlit_field=0, hdist_field=0, cl_lens=None, items=None, hclen=None, tail=()):
    """A final dynamic block from raw fields; tail: (code, bits) pairs emitted as data."""
    s = Stream()
    cl_lens = cl_lens or [0] * 19
    s.raw_header(True, hlit_field, hdist_field, cl_lens, hclen or min_hclen(cl_lens), items or [])
    for c, n in tail:
        s.w.code(c, n)
    return s.w.done()


def _lens_header(ll, dl, **kw):
    """A header that carries exactly these lengths, plainly coded with a 4-bit code-length code for 0 .. 15."""
    cl = [4] * 16 + [0] * 3
    return _bad_header(len(ll) - 257, len(dl) - 1, cl, [(l, 0) for l in ll + dl], **kw)


@functools.lru_cache(maxsize=None)
def invalid():
    """[(name, deflate bytes, isize, crc, status, the rule of sa_inflate.h's header it pins)]."""
    out = []

    def add(name, cd, status, rule, isize=64, crc=0):
        out.append((name, cd, isize, crc, status, rule))

    cl5 = [0] * 19   # a complete code-length code: 0 and 8 in one bit each, or with 16 / 18 in two
    cl5[0] = cl5[8] = 1
    clr = [0] * 19
    clr[0], clr[8], clr[16], clr[18] = 1, 2, 3, 3
    ok_ll = [8] * 255 + [0, 8]   # 256 codes of 8 bits: complete, with an end-of-block code
    add("hlit_287", _bad_header(30, 0, cl5, [(8, 0)] * 288), E_CODES, "HLIT > 286")
    add("hlit_288", _bad_header(31, 0, cl5, [(8, 0)] * 289), E_CODES, "HLIT > 286")
    add("hdist_31", _bad_header(0, 30, cl5, [(8, 0)] * 288), E_CODES, "HDIST > 30")
    add("hdist_32", _bad_header(0, 31, cl5, [(8, 0)] * 289), E_CODES, "HDIST > 30")
    add("repeat_first", _bad_header(0, 0, clr, [(16, 0), (8, 0)] + [(8, 0)] * 256), E_CODES, "a repeat without a previous length")
    add("repeat_past_end", _bad_header(0, 0, clr, [(8, 0)] * 255 + [(0, 0), (8, 0), (18, 0)]), E_CODES,
        "a repeat past HLIT + HDIST")
    add("repeat_16_past_end", _bad_header(0, 0, clr, [(8, 0)] * 255 + [(0, 0), (8, 0), (16, 0)]), E_CODES,
        "a repeat past HLIT + HDIST")
    add("no_end_of_block", _lens_header([8] * 256 + [0], [0]), E_CODES, "a missing end-of-block code")
    add("hclen_4_all_zero", _bad_header(0, 0, [1 if s in (0, 18) else 0 for s in range(19)], [(18, 127), (18, 109)], hclen=4),
        E_CODES, "a missing end-of-block code")
    add("lit_oversubscribed", _lens_header([8] * 257, [0]), E_CODES, "an over-subscribed set")
    add("dist_oversubscribed", _lens_header(ok_ll, [1, 1, 1]), E_CODES, "an over-subscribed set")
    add("cl_oversubscribed", _bad_header(0, 0, [1, 1, 1] + [0] * 16, []), E_CODES, "an over-subscribed set")
    add("lit_incomplete", _lens_header([2] + [0] * 255 + [2], [0]), E_CODES, "an incomplete set")
    add("lit_one_2bit_code", _lens_header([0] * 256 + [2], [0]), E_CODES, "an incomplete set")
    add("dist_incomplete_two_2bit", _lens_header(ok_ll, [2, 2]), E_CODES, "an incomplete set")
    add("dist_incomplete_one_2bit", _lens_header(ok_ll, [2]), E_CODES, "an incomplete set")
    add("cl_incomplete", _bad_header(0, 0, [1] + [0] * 18, []), E_CODES, "an incomplete set")
    # an unused code of an incomplete (single 1-bit code) distance set, used: the code '1' has no symbol
    s = Stream()
    s.raw_header(True, 1, 0, [4] * 16 + [0] * 3, 19, [(l, 0) for l in [8] * 254 + [0, 0, 8, 8] + [1]])
    lc = canon([8] * 254 + [0, 0, 8, 8])
    s.w.bits(*lc[65])
    s.w.bits(*lc[257])
    s.w.bits(1, 1)
    s.w.bits(*lc[EOB])
    add("dist_unused_code_used", s.w.done() + b"\0\0", E_CODES, "an incomplete set")
    for sym in (286, 287):
        w = BitWriter()
        w.bits(3, 3)
        w.fixed_litlen(65)
        w.fixed_litlen(sym)
        w.code(0, 5)
        w.fixed_litlen(EOB)
        add(f"fixed_litlen_{sym}", w.done(), E_CODES, "the codes 286 / 287")
    for ds in (30, 31):
        w = BitWriter()
        w.bits(3, 3)
        w.fixed_litlen(65)
        w.fixed_litlen(257)
        w.code(ds, 5)
        w.fixed_litlen(EOB)
        add(f"fixed_dist_{ds}", w.done(), E_CODES, "the distance codes 30 / 31")
    # a length symbol complete, its 5 extra bits cut by the end of the input: 3 + 9 + 8 bits, then 4 of the 5
    w = BitWriter()
    w.bits(3, 3)
    w.fixed_litlen(0x90)
    w.fixed_litlen(284)
    w.bits(31, 5)
    w.code(0, 5)
    w.fixed_litlen(EOB)
    add("length_extra_past_input", w.done()[:3], E_INPUT, "input")
    add("in_len_1", b"\x03", E_INPUT, "input")
    # every end-of-input case with its last byte removed
    fx = {n: (cd, d) for n, cd, d in valid()}
    for name in END_CASES:
        cd, d = fx[name]
        add(name + "_cut", cd[:-1], E_INPUT, "input", isize=len(d), crc=zlib.crc32(d))
    # ISIZE 0 and CRC 0 (a zeroed trailer) in front of data: inflated like any other member, it has no room
    tfx = {n: (cd, d) for n, cd, d in ti.fixtures()}
    add("isize0_dynamic_l9", tfx["dynamic_l9"][0], E_SIZE, "isize 0", isize=0)
    add("isize0_stored", Stream().stored(text()[:100], True).done()[0], E_SIZE, "isize 0", isize=0)
    add("isize0_fixed", Stream().fixed(list(text()[:100]), True).done()[0], E_SIZE, "isize 0", isize=0)
    _check_invalid([v[:5] for v in out])
    return out


# ---- the seeded streams ------------------------------------------------------------
def _seeded_text(rng, n):
    kind = int(rng.integers(0, 4))
    tx = text()
    if kind == 0:
        at = int(rng.integers(0, len(tx) - n))
        return tx[at:at + n]
    if kind == 1:   # runs
        parts = []
        while sum(map(len, parts)) < n:
            parts.append(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 400)))
        return b"".join(parts)[:n]
    if kind == 2:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    at = int(rng.integers(0, len(tx) - n))
    half = n // 2
    return tx[at:at + half] + rng.integers(0, 256, n - half, dtype=np.uint8).tobytes()


def _random_dyn(rng):
    def dyn(bi):
        kw = dict(limit=int(rng.integers(7, 16)), rle=bool(rng.integers(0, 4)), cl_skew=not rng.integers(0, 5))
        if not rng.integers(0, 4):
            kw["hclen"] = 19
        if not rng.integers(0, 3):
            kw["hlit"], kw["hdist"] = 286, 30
        return kw
    return dyn


@functools.lru_cache(maxsize=None)
def seeded(seed):
    """24 members of 1 .. 8 KiB of text (FASTQ, runs, uniform bytes, a mix), tokenised
    and cut with random parameters: [(deflate bytes, text, the same bytes with one bit flipped)]."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(24):
        n = int(rng.integers(1024, 8193))
        tx = _seeded_text(rng, n)
        nb = int(rng.integers(1, 7))
        cuts = sorted(int(x) for x in rng.integers(1, n, nb - 1)) + [n]
        types = [("s", "f", "d", "d")[int(rng.integers(0, 4))] for _ in range(nb)]
        cd, _ = forge(tx, cuts, types, min_len=int(rng.integers(3, 6)), max_len=(8, 64, 258)[int(rng.integers(0, 3))],
                      max_dist=(64, 1024, 32768)[int(rng.integers(0, 3))], dyn=_random_dyn(rng))
        assert zlib_says(cd) == ("ok", tx)
        bit = int(rng.integers(0, len(cd) * 8))
        bad = bytearray(cd)
        bad[bit >> 3] ^= 1 << (bit & 7)
        out.append((cd, tx, bytes(bad)))
    return out


SEEDS = range(32)


# ---- the gzip path -------------------------------------------------------------------
GZ_TEXT = 600_000
GZ_BLOCK = 8192   # text bytes per forged block
HEADER_SHAPES = (dict(), dict(hclen=19), dict(rle=False), dict(cl_skew=True), dict(hlit=286, hdist=30), dict(limit=9))


def _run_tokens(part: bytes):
    """Literals, and every run of 4 .. 259 equal bytes as its first byte and a
    match at distance 1: the one distance (and distance code) the block uses."""
    out, i = [], 0
    while i < len(part):
        n = 1
        while i + n < len(part) and part[i + n] == part[i] and n < 259:
            n += 1
        out.append(part[i])
        if n >= 4:
            out.append((n - 1, 1))
            i += n
        else:
            i += 1
    return out


def _rarest(tokens):
    """The rarest literal and the rarest distance code of a block's tokens."""
    lf, df = {}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
        else:
            df[dist_sym(t[1])] = df.get(dist_sym(t[1]), 0) + 1
    return min(lf, key=lambda s: (lf[s], s)), (min(df, key=lambda s: (df[s], s)) if df else None)


@functools.lru_cache(maxsize=None)
def _gz_built():
    """The three streams' writers, with the writer's state saved after every block."""
    import test_gunzip as tg
    tx = tg.fq_text()[:GZ_TEXT]
    cuts = list(range(GZ_BLOCK, GZ_TEXT, GZ_BLOCK)) + [GZ_TEXT]
    tk, blocks, start = Tokeniser(tx), [], 0
    for end in cuts:
        blocks.append(tk.tokens(start, end))   # (matches reach back up to 32768, across four blocks)
        start = end
    out = {}
    for name in ("long_codes", "header_shapes", "odd_dist_alphabets"):
        s, snaps, start = Stream(), [], 0
        for bi, (end, toks) in enumerate(zip(cuts, blocks)):
            final = end == GZ_TEXT
            if name == "long_codes":
                lit, ds = _rarest(toks)
                s.dynamic(toks, final, skew_l=[lit], skew_d=None if ds is None else [ds])
            elif name == "header_shapes":
                s.dynamic(toks, final, **HEADER_SHAPES[bi % len(HEADER_SHAPES)])
            elif bi % 3 != 2:
                s.dynamic(toks, final)
            elif bi % 2:
                s.dynamic(list(tx[start:end]), final)   # no distance code
                assert s.hdr["dl"] == [0]
            else:
                s.dynamic(_run_tokens(tx[start:end]), final)   # one 1-bit distance code, in use
                assert s.hdr["dl"] == [1]
            snaps.append((bytes(s.w.out), s.w.acc, s.w.n, len(s.data)))
            start = end
        cd, data = s.done()
        assert data == tx and zlib_says(cd) == ("ok", tx), name
        if name == "long_codes":
            assert all(max(lens_at(cd, b)[0]) == 15 for b in s.dyn[::7])
        out[name] = (cd, tx, snaps)
    return out


@functools.lru_cache(maxsize=None)
def gz_streams():
    """{name: (gzip bytes, text)}: three one-member files of 600 KB of FASTQ in dynamic
    blocks of 8 KiB of text, so that at any chunk size most waves start inside a forged block:
    long_codes: every block's codes reach 15 bits (the rarest literal and distance code own them);
    header_shapes: the headers cycle through HEADER_SHAPES;
    odd_dist_alphabets: every third block has no distance code, or one 1-bit code in use."""
    import test_gunzip as tg
    return {name: (tg.member(cd, tx), tx) for name, (cd, tx, _) in _gz_built().items()}


@functools.lru_cache(maxsize=None)
def gz_invalid():
    """[(name, gzip bytes, status, text)]: every invalid block that breaks a rule of
    the code-length judgement, behind valid blocks: `second`: behind the first 16
    blocks of header_shapes (more than one 32 KiB chunk of them), `deep`: behind the
    first 50 blocks of long_codes.  The text before the bad block is the stream's."""
    import test_gunzip as tg
    built = _gz_built()
    out = []
    for place, src, nb in (("second", "header_shapes", 16), ("deep", "long_codes", 50)):
        cd0, tx, snaps = built[src]
        pre, acc, n, ntext = snaps[nb - 1]
        if place == "second":
            assert 32768 < len(pre) < 65536
        for name, cd, isize, crc, status, rule in invalid():
            if status != E_CODES:
                continue
            w = BitWriter()
            w.out, w.acc, w.n = bytearray(pre), acc, n
            for byte in cd:
                w.bits(byte, 8)
            raw = w.done()
            assert zlib_says(raw)[0] == "error", name
            out.append((f"{place}_{name}", tg.HDR + raw + bytes(8), status, tx[:ntext]))
    return out
