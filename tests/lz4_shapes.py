"""LZ4 blocks of every shape the format allows, for the decoder tests (plain module, like zstd_shapes.py; pure Python / numpy).

  build()         sequences [(literals, offset, match length[, count])] + final literals -> (stream, decoded).  A zero-literal
                  sequence repeated `count` times is one tile of its bytes in the stream and one long match in the output.
  inspect()       walks a VALID stream and returns the ledger keys it reaches, computed from the stream, the capacity and the
                  constants of lz4tile.h / lz4seg.h (copied below).  walk() is the sequence list under it.
  REQUIRED        the ledger keys the frame set must reach.  A missing key is a test failure.
  frames()        the deterministic shape set: named streams, each as small as its key allows, with the capacities they run at.
  damaged()       structure-aware damage of a valid frame at the fields walk() located.

What the models below restate (each with the lines it was read from):
  segments        the walks cut the stream below limit = csize - kMargin into nseg = clamp(limit / kMinSeg, 1, S) segments of
                  seglen = (ceil(limit / nseg) + r) & ~r bytes: S = 64, r = 3 for the segment-parallel walk (lz4_seg.hip:269-271),
                  S = 512, r = 31 for the tile path's fused walk (lz4_tile.hip:413-415).
  hop()           one token at an arbitrary stream byte, as the walks decode it (lz4_seg.hip:121-148, lz4_tile.hip:131-151).
  fix list        the true chain enters a segment at e; it is followed until it meets the chain walked from the segment's first
                  byte; after kFixCap hops without meeting it the segment is walked again (lz4_seg.hip:237-252).
  chunks, tiles   the tile executor's partition of the sequences into chunks (tokens of up to kChunk stream bytes from the 32-byte
                  line of the first, at most nmax <= kSeqs of them) and of a chunk's output into tiles of at most kTile - 8 bytes
                  that do not wrap around the 64 KiB ring (lz4_tile.hip:509-536, 609-650, 787-790).  The ring index of output byte
                  P is (A + P) & 0xFFFF with A the destination ADDRESS mod 65536: the ledger is computed for A = 0, and the GPU
                  test places every destination slot at such an address."""
import collections
import functools

import numpy as np

# ---- constants of the fast paths (4mc_amd/csrc) ------------------------------------------------------------------------------
K_SEGS_SEG, K_SEGS_TILE = 64, 512           # lz4seg.h:22 kSegs; lz4tile.h:26 kThreads (one segment per thread of the fused walk)
K_MARGIN, K_OMARGIN = 64, 128               # lz4tile.h:20-21, lz4seg.h:24-25
K_MINSEG, K_MINSRC, K_MINCAP = 1024, 256, 256      # lz4tile.h:22-23, lz4seg.h:26-27
K_MAXSRC, K_DSTMAX = 4210768 + 32, 4 << 20  # lz4par.h:24-25 kSrcMax, kDstMax
K_TILE, K_SEQS, K_CHUNK, K_RING = 4096, 384, 1536, 65536      # lz4tile.h:27-29, 32
K_ESCLL, K_FIXCAP, K_CAPB = 511, 128, 4032  # lz4seg.h:29, 23, 31
RETRY = -1000000003                         # lz4par.h:50 kRetryCode (lz4_decode.hip:425: what paths 12 / 14 leave in a block handed back)
MIB = 1 << 20


def eligible(csize, cap):
    """lz4_tile.hip:101-102, lz4_seg.hip:254-255"""
    return K_MINSRC <= csize <= K_MAXSRC and K_MINCAP <= cap <= K_DSTMAX


# ---- builder -------------------------------------------------------------------------------------------------------------------
def _ext(v):
    return bytes([255]) * (v // 255) + bytes([v % 255])


def encode_seq(lits, off, ml):
    ll = len(lits)
    out = bytearray([(min(ll, 15) << 4) | min(ml - 4, 15)])
    if ll >= 15: out += _ext(ll - 15)
    out += lits
    out += bytes([off & 255, off >> 8])
    if ml - 4 >= 15: out += _ext(ml - 19)
    return bytes(out)


def encode_final(lits):
    ll = len(lits)
    return bytes([min(ll, 15) << 4]) + (_ext(ll - 15) if ll >= 15 else b"") + bytes(lits)


def _b(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def _match(dec, o, off, n):
    assert 1 <= off <= min(o, 65535), (off, o)
    if off >= n: dec[o:o + n] = dec[o - off:o - off + n]
    else: dec[o:o + n] = np.resize(dec[o - off:o], n)


def build(seqs, final):
    """-> (stream, decoded) as uint8 arrays.  seqs: (literals, offset, match length) or (literals, offset, match length, count)."""
    final = _b(final)
    total = sum((len(s[0]) + s[2]) * (s[3] if len(s) > 3 else 1) for s in seqs) + len(final)
    dec, o, parts = np.empty(total, np.uint8), 0, []
    for s in seqs:
        lits, off, ml, cnt = _b(s[0]), s[1], s[2], (s[3] if len(s) > 3 else 1)
        assert ml >= 4 and cnt >= 1
        enc = encode_seq(lits, off, ml)
        parts.append(enc * cnt)
        ll = len(lits)
        if ll == 0:                                          # no literals between them: `cnt` matches are one long match
            _match(dec, o, off, ml * cnt); o += ml * cnt
            continue
        la = np.frombuffer(lits, np.uint8)
        for _ in range(cnt):
            dec[o:o + ll] = la; o += ll
            _match(dec, o, off, ml); o += ml
    parts.append(encode_final(final))
    dec[o:] = np.frombuffer(final, np.uint8)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), dec


# ---- the sequence list -----------------------------------------------------------------------------------------------------------
Walk = collections.namedtuple("Walk", "csize n tp lp ll mp off ml out ftp flp fll")
# per match sequence: token position, literal start, literal length, offset position, offset, match length, output position of
# its first literal; the final token: position, literal start, literal length; n = decoded size


@functools.lru_cache(maxsize=512)
def _walk(s):
    n, p, o = len(s), 0, 0
    tp, lp, ll_, mp, off_, ml_, out = [], [], [], [], [], [], []
    while True:
        t = s[p]; ll = t >> 4; q = p + 1
        if ll == 15:
            while True:
                b = s[q]; q += 1; ll += b
                if b != 255: break
        if q + ll >= n:
            assert q + ll == n, "not a valid block"
            a = lambda x: np.array(x, np.int64)
            return Walk(n, o + ll, a(tp), a(lp), a(ll_), a(mp), a(off_), a(ml_), a(out), p, q, ll)
        m = q + ll; ml = (t & 15) + 4; q2 = m + 2
        if ml == 19:
            while True:
                b = s[q2]; q2 += 1; ml += b
                if b != 255: break
        tp.append(p); lp.append(q); ll_.append(ll); mp.append(m); off_.append(s[m] | (s[m + 1] << 8)); ml_.append(ml); out.append(o)
        o += ll + ml; p = q2


def walk(stream):
    return _walk(_b(stream))


def sequences(stream):
    """[(token position, literal length, offset, match length, output position)] and the final (position, literals, output)"""
    w = walk(stream)
    return ([tuple(int(v) for v in r) for r in zip(w.tp, w.ll, w.off, w.ml, w.out)], (w.ftp, w.fll, w.n - w.fll))


# ---- models of the walks ---------------------------------------------------------------------------------------------------------
def segments(csize, nmax, rnd):
    """(nseg, seglen) of a stream: lz4_seg.hip:269-271 (nmax 64, rnd 3), lz4_tile.hip:413-415 (nmax 512, rnd 31)"""
    limit = csize - K_MARGIN
    nseg = max(1, min(nmax, limit // K_MINSEG))
    return nseg, ((limit + nseg - 1) // nseg + rnd) & ~rnd


def hop(s, limit, p):
    """next token position of a token assumed at p, or None where the walks stop (lz4_seg.hip:121-148)"""
    if p >= limit: return None
    t = s[p]; ll = t >> 4; q = p + 1
    if ll == 15:
        b = s[q]; q += 1; ll += b
        while b == 255:
            if q >= limit: return None
            b = s[q]; q += 1; ll += b
            if b == 255 and ll > (1 << 23): return None
    mo = q + ll
    if mo + 2 > limit: return None
    q2 = mo + 2
    if (t & 15) == 15:
        while True:
            if q2 >= limit: return None
            b = s[q2]; q2 += 1
            if b != 255: break
    return q2 if q2 <= limit else None


def taken(w):
    """how many sequences the walks take: the first token whose bytes end beyond csize - kMargin is the tail's (a valid token's
    fields all lie in front of the next token, so that is the only rule of hop() that can stop a true chain)"""
    nxt = np.append(w.tp[1:], w.ftp)
    return int(np.searchsorted(nxt, w.csize - K_MARGIN, "right"))


def fast_stop(w, cap):
    """(token position, output position) at which either fast path hands a valid block to the exact walker: the first sequence
    whose output ends beyond cap - kOMargin (lz4_tile.hip:612, 638-639, 793; lz4_seg.hip:434-438, 450), else the first token the
    walk does not take (kMetaTailIp).  kTile, kSeqs and kCapB only cut the work into tiles and batches."""
    nt = taken(w)
    end = w.out[:nt] + w.ll[:nt] + w.ml[:nt]
    over = np.flatnonzero(end > cap - K_OMARGIN)
    i = int(over[0]) if len(over) else nt
    if i < len(w.tp): return int(w.tp[i]), int(w.out[i])
    return w.ftp, w.n - w.fll


def fix_hops(s, w, nmax=K_SEGS_SEG, rnd=3):
    """per segment the true chain enters behind its first byte: (met, hops) - the hops of the true chain inside it before it meets
    the chain walked from the segment's first byte, or before it leaves the segment without meeting it (lz4_seg.hip:237-252)"""
    limit = w.csize - K_MARGIN
    nseg, seglen = segments(w.csize, nmax, rnd)
    nt = taken(w)
    tps = w.tp[:nt]
    out = {}
    for j in range(1, nseg):
        a, z = j * seglen, ((j + 1) * seglen if j + 1 < nseg else 1 << 40)
        i = int(np.searchsorted(tps, a))
        if i >= nt or tps[i] >= z or tps[i] == a: continue
        spec, p = set(), a
        while p is not None and p < z:
            spec.add(p); p = hop(s, limit, p)
        hops, met = 0, False
        while i < nt and tps[i] < z:
            if int(tps[i]) in spec: met = True; break
            hops += 1; i += 1
        out[j] = (met, hops)
    return out


def tile_model(w, cap, A=0):
    """the tile executor's chunks and tiles (lz4_tile.hip:509-536, 609-650, 787-790; left out: `sz < kSzClamp` of :612, which no
    sequence of a block of at most 4 MiB fails, and the staging of fields and literals beyond kStage, :560-589 and :726-732, which
    changes where bytes are read from, not which sequences a chunk takes) ->
    (chunks [(first sequence, tokens in the window, sequences decoded, sequences taken, window start)], tile edges [(start, end)])"""
    nt = taken(w)
    tail_ip = int(w.tp[nt]) if nt < len(w.tp) else w.ftp
    olimit = cap - K_OMARGIN
    sz = w.ll + w.ml
    i, opos, nmax, cut = 0, 0, 256, False
    chunks, tiles = [], []
    while i < nt and not cut:
        cb = int(w.tp[i]) & ~31
        cend = min(cb + K_CHUNK, tail_ip)
        ntok = int(np.searchsorted(w.tp[:nt], cend)) - i
        n = min(ntok, nmax)
        incl = np.cumsum(sz[i:i + n])
        fo = opos + incl <= olimit
        ft = incl <= K_TILE - 8; ft[0] = True
        nfo = n if fo.all() else int(np.argmin(fo))
        nft = n if ft.all() else int(np.argmin(ft))
        nfit = min(nfo, nft)
        total = int(incl[nfit - 1]) if nfit else 0
        if nfit < n and nfo <= nft: cut = True
        chunks.append((i, ntok, n, nfit, cb))
        r0 = 0
        while r0 < total:
            gb0 = A + opos; mis = gb0 & 7; gb = (gb0 - mis) & 0xFFFF
            t = min(total - r0, K_TILE - 8)
            if gb + mis + t > K_RING: t = K_RING - gb - mis
            tiles.append((opos, opos + t)); opos += t; r0 += t
        if nfit == n and total < K_TILE - 8 - (K_TILE >> 3): nmax = nmax + (nmax >> 2) + 8
        elif nfit < n: nmax = nfit + (nfit >> 4) + 2
        nmax = max(8, min(K_SEQS, nmax))
        i += nfit
    return chunks, tiles


# ---- inspector -------------------------------------------------------------------------------------------------------------------
OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, K_TILE - 9, K_TILE - 8, K_TILE - 7, 65535)
LL_EXACT = tuple(range(16)) + (269, 270, 510, 511, 512)
ML_EXACT = (4, 18, 19, 273, 274, 528, 529)          # 528: two extension bytes at their maximum (255, 254); 529: the first with three
BOUND_KINDS = ("token", "ext", "off0", "off1", "literal")
ELIGIBILITY = frozenset({"csize:255", "cap:255"})   # keys only a block outside the fast paths' sizes reaches
SIM_MAX = 1 << 19                                   # streams above this size skip the byte-by-byte simulations (the extremes)


def _kind_at(w, x):
    """what the stream byte x is: token / ext (a length extension byte) / literal / off0 / off1"""
    i = int(np.searchsorted(w.tp, x, "right")) - 1
    if x >= w.ftp or i < 0:
        return "token" if x == w.ftp else "ext" if x < w.flp else "literal"
    if x == w.tp[i]: return "token"
    if x < w.lp[i]: return "ext"
    if x < w.mp[i]: return "literal"
    return "off0" if x == w.mp[i] else "off1" if x == w.mp[i] + 1 else "ext"


def inspect(stream, cap):
    """the ledger keys a valid stream reaches when it is decoded into `cap` bytes"""
    s = _b(stream)
    w = _walk(s)
    k = set()
    ns, csize, n = len(w.tp), w.csize, w.n
    ms = w.out + w.ll                                       # output position of every match
    alll = np.append(w.ll, w.fll)
    # length fields
    for v in LL_EXACT:
        if (alll == v).any(): k.add(f"ll:{v}")
    for name, lim in (("kChunk", K_CHUNK), ("kTile", K_TILE), ("kCapB", K_CAPB), ("64K", 65536)):
        if (alll > lim).any(): k.add(f"ll>{name}")
        if ns and (w.ml > lim).any(): k.add(f"ml>{name}")
    if (alll >= MIB).any(): k.add("ll>=1M")
    if ns and (w.ml >= MIB).any(): k.add("ml>=1M")
    for v in ML_EXACT:
        if ns and (w.ml == v).any(): k.add(f"ml:{v}")
    # offsets
    for v in OFFSETS:
        if ns and (w.off == v).any(): k.add(f"off:{v}")
    if ns and (w.off == ms).any(): k.add("off=out")
    if ns and ((w.off == 65535) & (ms > 65535)).any(): k.add("off:65535+window")
    # stream-level density
    if ns:
        nxt = np.append(w.tp[1:], w.ftp)
        if (nxt - w.tp >= 2 * K_CHUNK).any(): k.add("chunk:no-token")
        if ns >= 64:
            c = np.concatenate([[0], np.cumsum(w.ll + w.ml)])
            s64 = c[64:] - c[:-64]
            plain = np.concatenate([[0], np.cumsum((w.ll >= K_ESCLL) | (w.ml > 528))])
            ok = (plain[64:] - plain[:-64]) == 0             # 64 sequences the executor takes from records (no escape among them)
            if (ok & (s64 > K_CAPB)).any(): k.add("batch:64>kCapB")
            if (ok & (s64 <= K_CAPB // 8)).any(): k.add("batch:64<<kCapB")
    # eligibility and sizes
    for v in (255, 256, 257, 65535, 65536):
        if csize == v: k.add(f"csize:{v}")
    for v in (65535, 65536):
        if csize - K_MARGIN == v: k.add(f"limit:{v}")        # where the 64th segment appears (limit / kMinSeg)
    for v in (255, 256, 257):
        if cap == v: k.add(f"cap:{v}")
    if cap - n in (0, 1, 127, 128, 129): k.add(f"slack:{cap - n}")
    if ns:
        stop = fast_stop(w, cap)[1]                          # the fast paths' last sequence ends exactly at / one before the margin
        if stop and cap - stop in (K_OMARGIN, K_OMARGIN + 1): k.add(f"omargin:last-taken-ends:cap-{cap - stop}")
    # ends
    if ns and 5 <= w.fll <= 12: k.add(f"end:final:{w.fll}")
    if csize - w.ftp in (63, 64, 65): k.add(f"margin:lasttoken:{csize - w.ftp}")
    # extremes
    if n == 4 * MIB and ns >= 1000000 and (w.ll[1:] == 0).all() and (w.ml == 4).all(): k.add("extreme:dense4M")
    if n == 4 * MIB and ns == 0: k.add("extreme:lit4M")
    if not ns: return k
    # the walks: what a segment's first byte is, live segments, the fix list
    limit = csize - K_MARGIN
    for path, nmax, rnd in (("seg", K_SEGS_SEG, 3), ("tile", K_SEGS_TILE, 31)):
        nseg, seglen = segments(csize, nmax, rnd)
        for j in range(1, nseg):
            if j * seglen < limit: k.add(f"{path}:bound:{_kind_at(w, j * seglen)}")
        if path == "seg" and nseg == K_SEGS_SEG:
            live = len(set(np.minimum(w.tp[:taken(w)] // seglen, nseg - 1).tolist()) | {0})
            if live < K_SEGS_SEG: k.add("walk:live<64")
    if csize <= SIM_MAX:
        fx = fix_hops(s, w)
        if any(h > K_FIXCAP for _, h in fx.values()): k.add("walk:fix>kFixCap")
        if any(met and 16 <= h <= K_FIXCAP for met, h in fx.values()): k.add("walk:fix<=kFixCap")
    # the tile executor's chunks and tiles (A = 0)
    chunks, tiles = tile_model(w, cap)
    for first, ntok, nd, nfit, cb in chunks:
        if ntok > K_SEQS: k.add("chunk:ntok>kSeqs")
        if ntok in (K_SEQS, K_SEQS + 1): k.add(f"chunk:ntok={ntok}")
        if nd == K_SEQS: k.add("chunk:decodes-kSeqs")
        last = first + nd - 1
        if w.tp[last] == cb + K_CHUNK - 1 and w.lp[last] > w.tp[last] + 1: k.add("chunk:token-last-byte+ext")
    if tiles:
        t0 = np.array([a for a, _ in tiles]); t1 = np.array([b for _, b in tiles])
        if ((t1 - t0 < K_TILE - 8) & ((t1 & 0xFFFF) == 0)).any(): k.add("ring:tile-clipped")
        done = int(t1[-1])
        sel = ms < done                                      # matches that begin inside a tile
        ti = np.searchsorted(t1, ms[sel], "right")           # the tile a match begins in
        a0, a1 = t0[ti], t1[ti]
        m, off, ml = ms[sel], w.off[sel], w.ml[sel]
        if ((m - off < a0) & (m - off + ml > a0) & (m > a0)).any(): k.add("tile:src-straddle")
        if ((off < ml) & (m + ml > a1)).any(): k.add("tile:overlap-cross")
        s0, span = m - off, np.minimum(ml, off)              # the distinct bytes a match reads
        if ((s0 // K_RING != (s0 + span - 1) // K_RING) & (m > K_RING)).any(): k.add("ring:src-wrap")
        if ns <= 4096 and _chase_depth(w, ms, t0, t1, done) >= 16: k.add("tile:chase>=16")
    return k


def _chase_depth(w, ms, t0, t1, done):
    """the longest chain of matches inside one tile, each with its source's first byte in the match before it"""
    depth, best = {}, 0
    for i in range(len(ms)):
        m = int(ms[i])
        if m >= done: break
        a0 = int(t0[int(np.searchsorted(t1, m, "right"))])
        src = m - int(w.off[i])
        d = 1
        if src >= a0:
            j = int(np.searchsorted(ms, src, "right")) - 1   # the sequence whose match holds the source's first byte
            if j >= 0 and ms[j] <= src < ms[j] + w.ml[j] and ms[j] >= a0: d = depth.get(j, 1) + 1
        depth[i] = d; best = max(best, d)
    return best


REQUIRED = frozenset(
    [f"ll:{v}" for v in LL_EXACT] + [f"ml:{v}" for v in ML_EXACT] + [f"off:{v}" for v in OFFSETS] +
    [f"{f}>{lim}" for f in ("ll", "ml") for lim in ("kChunk", "kTile", "kCapB", "64K")] + ["ll>=1M", "ml>=1M"] +
    ["off=out", "off:65535+window", "tile:overlap-cross", "tile:src-straddle", "ring:src-wrap", "ring:tile-clipped", "tile:chase>=16"] +
    ["chunk:ntok>kSeqs", "chunk:ntok=384", "chunk:ntok=385", "chunk:decodes-kSeqs", "chunk:no-token", "chunk:token-last-byte+ext",
     "batch:64>kCapB", "batch:64<<kCapB"] +
    [f"{p}:bound:{kind}" for p in ("seg", "tile") for kind in BOUND_KINDS] +
    ["walk:fix>kFixCap", "walk:fix<=kFixCap", "walk:live<64"] +
    [f"csize:{v}" for v in (255, 256, 257, 65535, 65536)] + [f"limit:{v}" for v in (65535, 65536)] + [f"cap:{v}" for v in (255, 256, 257)] +
    [f"end:final:{v}" for v in range(5, 13)] + [f"slack:{v}" for v in (0, 1, 127, 128, 129)] +
    [f"margin:lasttoken:{v}" for v in (63, 64, 65)] + ["omargin:last-taken-ends:cap-128", "omargin:last-taken-ends:cap-129"] + ["extreme:dense4M", "extreme:lit4M"])


# ---- the shape set ---------------------------------------------------------------------------------------------------------------
Frame = collections.namedtuple("Frame", "name stream decoded caps")
SLACKS = (0, 1, 127, 128, 129)
BIG = 300000                                  # frames with more stream or output than this run at few capacities and are not damaged


def _csize(seqs):
    return sum(len(encode_seq(_b(s[0]), s[1], s[2])) * (s[3] if len(s) > 3 else 1) for s in seqs)


def _final_for(seqs, target):
    """number of final literals with which the stream is exactly `target` bytes"""
    rest = target - _csize(seqs)
    for f in range(max(rest - 300, 5), rest):
        if len(encode_final(bytes(f))) == rest: return f
    raise AssertionError((rest, target))


@functools.lru_cache(None)
def frames():
    rng = np.random.default_rng(0x4C5A34)
    R = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = []

    def add(name, seqs, final=12, caps=None):
        st, dec = build(seqs, R(final) if isinstance(final, int) else final)
        n = len(dec)
        if caps is None:
            caps = [n + d for d in SLACKS] if max(n, len(st)) <= BIG else [n, n + 128] if n + 128 <= K_DSTMAX else [n]
        out.append(Frame(name, st, dec, tuple(caps)))

    # literal lengths
    add("ll_0..15", [(R(300), 1, 4)] + [(R(v), v + 1, 4 + v) for v in range(16)])
    add("ll_ext", [(R(40), 33, 5)] + [(R(v), 33, 5) for v in (269, 270, 510, 511, 512, 15, 16)])
    add("ll_long", [(R(64), 3, 6)] + [(R(v), 40, 8) for v in (K_CHUNK + 1, K_TILE + 1, K_CAPB + 1, 3 * K_CHUNK)])
    add("ll_64k", [(R(30), 30, 4), (R(65537), 65535, 20), (R(3), 2, 9)])
    add("ll_1m", [(R(30), 30, 4), (R(MIB), 4088, 20), (R(3), 2, 9)])
    # match lengths
    add("ml_vals", [(R(300), 7, 4)] + [(R(3 + i), 31 + i, v) for i, v in enumerate((4, 18, 19, 273, 274, 528, 529, 530, 1000))])
    add("ml_long", [(R(200), 200, K_TILE + 1), (R(5), 150, K_CAPB + 1), (R(2), 3, 9000), (R(700), 650, 9000), (R(1), 1, 5000)])
    add("ml_64k", [(R(100), 7, 65537), (R(9), 100, 70000)])
    add("ml_1m", [(R(1000), 999, MIB), (R(9), 1, 70)])
    # offsets
    add("offsets", [(R(300), 300, 4)] + [(R(i % 3), v, ml) for i, v in enumerate(OFFSETS[:12]) for ml in (4, 40)])
    add("off_tile", [(R(5000), 5000, 4)] + [(R(i), v, ml) for i, v in enumerate((K_TILE - 9, K_TILE - 8, K_TILE - 7)) for ml in (20, 5000)])
    add("off_out", [(R(20), 20, 30), (R(1), 51, 4), (R(300), 1, 4)])
    add("off_64k", [(R(65535), 65535, 200), (R(5), 65535, 70000), (R(0), 65535, 4), (R(9), 65534, 9)])
    add("ring_wrap", [(R(70000), 70000 - 65530, 20), (R(61100), 55, 20), (R(7), 65535, 300), (R(2000), 131072 + 2007 + 340 + 20 - 131070, 600),
                      (R(60000), 60000, 8000)])
    # tiles: sources across a tile edge, overlap across a tile edge, pointer chase
    add("straddle", [(R(3000), 3000, 4)] + [(R(i % 2), 600 + 7 * i, 250 + i) for i in range(60)])
    add("chase", [(R(300), 9, 8)] + [(R(1), 9, 8)] * 40 + [(R(2), 5, 4)] * 30 + [(R(1), 2, 17)] * 20)
    # density
    add("dense512", [(R(64), 61, 4), (b"", 61, 4, 3000), (R(1), 3, 4), (b"", 59, 4, 700)])
    add("chunk384", [(R(1), 1, 4)] + [(R(1), 1 + i % 5, 4) for i in range(1500)])
    add("chunk385", [(R(1), 1, 4)] + [(R(1), 1 + i % 5, 4) for i in range(380)] + [(b"", 11, 4, 4)] + [(R(1), 1 + i % 7, 4) for i in range(800)])
    edge = [(R(1000), 1000, 4), (R(500), 77, 4)] + [(R(14), 14, 5), (R(3), 3, 5)]
    assert _csize(edge) == K_CHUNK - 1
    add("chunk_edge", edge + [(R(20), 20, 5), (R(300), 300, 5)])
    add("batch_big", [(R(300), 300, 4)] + [(R(20), 100 + i, 60) for i in range(200)])
    # the walks
    mix_ll, mix_ml = (0, 0, 1, 3, 7, 15, 16, 20, 270, 300), (4, 4, 5, 9, 19, 20, 40, 274, 280)
    add("bounds", [(R(400), 400, 4)] + [(R(int(rng.choice(mix_ll))), int(rng.integers(1, 400)), int(rng.choice(mix_ml))) for _ in range(2200)])
    # (true tokens at 21 + 4 k: 10 10 10 00 reads as a token chain of its own from every other phase)
    add("falsechain", [(R(17), 16, 4)] + [(b"\x10", 16, 4)] * 20000)
    add("falsechain_met", [(R(17), 16, 4)] + ([(b"\x10", 16, 4)] * 240 + [(R(3), 16, 4)] * 60) * 70)
    add("fewlive", [(R(100), 100, 4), (R(40000), 555, 4)] + [(R(int(rng.integers(0, 30))), int(rng.integers(1, 90)), int(rng.integers(4, 30))) for _ in range(1800)])
    # eligibility and the size at which the 64th segment appears
    for n in (253, 254, 255, 256, 257):
        add(f"lit{n}", [], n, caps=sorted({c for c in (n, 255, 256, 257, n + 128) if c >= n}))
    small = [(R(120), 120, 4)] + [(R(i % 4), 3 + i, 4 + i % 9) for i in range(14)]
    for cs in (255, 256, 257):
        add(f"csize{cs}", small, _final_for(small, cs))
    base = [(R(400), 400, 4)] + [(R(int(rng.integers(0, 40))), int(rng.integers(1, 400)), int(rng.integers(4, 24))) for _ in range(2700)]
    assert 60000 < _csize(base) < 65000
    for cs in (65535, 65536, 65535 + K_MARGIN, 65536 + K_MARGIN):
        add(f"csize{cs}", base, _final_for(base, cs))
    # ends
    tail = [(R(300), 299, 7), (R(2), 5, 9), (b"", 1, 7)]        # (a match begins at least 12 bytes before the end: lz4.c MFLIMIT)
    for f in range(5, 13): add(f"final{f}", tail, f)
    for f in (61, 62, 63): add(f"lasttoken-{f + 2}", tail, f)
    # a sequence that ends at E = 332, at capacities E + 126 .. E + 129: the last one the fast paths take ends at cap - kOMargin
    # (70 final literals keep its token in front of the last kMargin stream bytes)
    add("omargin", [(R(300), 299, 7), (R(2), 5, 9), (R(3), 40, 11), (R(5), 9, 20)], 70, caps=[332 + d for d in (126, 127, 128, 129)])
    # extremes
    add("dense4m", [(R(64), 61, 4), (b"", 61, 4, (4 * MIB - 68 - 12) // 4)])
    add("lit4m", [], 4 * MIB)
    assert len({f.name for f in out}) == len(out)
    return tuple(out)


def ledger(frs, only_eligible=False):
    led = collections.Counter()
    for f in frs:
        for cap in f.caps:
            if only_eligible and not eligible(len(f.stream), cap): continue
            led.update(inspect(f.stream, cap))
    return led


# ---- damage ----------------------------------------------------------------------------------------------------------------------
def damaged(fr):
    """[(label, stream, cap)]: damage of a valid frame at the fields walk() located - at its first sequence, one in the middle, the
    last one whose offset lies in front of the last kMargin stream bytes and the first one behind that line."""
    s, w = fr.stream, walk(fr.stream)
    n, cs, ns = w.n, w.csize, len(w.tp)
    out = []

    def put(label, arr, cap=n):
        out.append((f"{fr.name}|{label}", np.ascontiguousarray(arr, dtype=np.uint8), int(cap)))

    sites = {}
    if ns:
        sites["first"], sites["mid"] = 0, ns // 2
        front = int(np.searchsorted(w.mp, cs - K_MARGIN)) - 1
        if front >= 0: sites["front-of-margin"] = front
        if front + 1 < ns: sites["in-margin"] = front + 1
        sites["last"] = ns - 1
    for where, i in sites.items():
        tp, lp, ll, mp, ml = (int(v[i]) for v in (w.tp, w.lp, w.ll, w.mp, w.ml))
        nxt = int(w.tp[i + 1]) if i + 1 < ns else w.ftp
        m = s.copy(); m[mp] = m[mp + 1] = 0
        put(f"off=0@{where}", m)
        beyond = int(w.out[i]) + ll + 1
        if beyond <= 65535:
            m = s.copy(); m[mp], m[mp + 1] = beyond & 255, beyond >> 8
            put(f"off=out+1@{where}", m)
        put(f"cut-after-token@{where}", s[:tp + 1])
        if lp > tp + 1: put(f"cut-in-ll-ext@{where}", s[:tp + 2])
        if ll: put(f"cut-in-literals@{where}", s[:lp + (ll + 1) // 2])
        put(f"cut-in-offset@{where}", s[:mp + 1])
        put(f"cut-after-offset@{where}", s[:mp + 2])
        if nxt > mp + 2: put(f"cut-in-ml-ext@{where}", s[:mp + 3])
        # a length extension run that goes on to the end of the stream
        m = s[:tp + 1].copy(); m[tp] |= 0xF0
        put(f"ll-ext-run-to-end@{where}", np.concatenate([m, np.full(9, 255, np.uint8)]))
        m = s[:mp + 2].copy(); m[tp] |= 0x0F
        put(f"ml-ext-run-to-end@{where}", np.concatenate([m, np.full(300, 255, np.uint8)]))
    # the block's end
    four = np.concatenate([s[:w.ftp], np.frombuffer(encode_final(_b(s[w.flp:w.flp + 4])), np.uint8)]) if w.fll >= 4 else None
    if four is not None and ns:                              # (= the last match ends 4 bytes before the end)
        n4 = n - w.fll + 4
        for cap in (n4, n4 + 1, n4 + 8): put(f"final-literals-4/cap+{cap - n4}", four, cap)
    if n > 0: put("cap-1", s, n - 1)
    put("cap+1", s, n + 1)
    g = np.random.default_rng(len(s))
    for extra in range(1, 21): put(f"garbage+{extra}", np.concatenate([s, g.integers(0, 256, extra, dtype=np.uint8)]))
    put("cut-last-byte", s[:-1])
    return out


def small_frames():
    return [f for f in frames() if max(len(f.stream), len(f.decoded)) <= BIG]


@functools.lru_cache(None)
def damaged_set():
    return tuple(d for f in small_frames() for d in damaged(f))


def cases():
    """every (label, stream, cap, decoded or None) the GPU tests launch: the valid frames at their capacities, then the damage"""
    out = [(f"{f.name}/cap+{c - len(f.decoded)}", f.stream, c, f.decoded) for f in frames() for c in f.caps]
    return out + [(lab, st, cap, None) for lab, st, cap in damaged_set()]
