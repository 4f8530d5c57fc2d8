"""Text lines written as the part files of a TextOutputFormat job (fourmc_gpu_lines_pack, _images_write_lines, _bstreams_write_lines /
pack_lines, write_lines_images, write_lines_bstreams).

The device is compared byte for byte with tests/text_output_model.py: the writer rule (text, newline, two write() calls per line) fed
into the closed forms of the image and block stream models, the oracle as block compressor.  A catalogue of lines is written with ONE
call per (target, level) and source: level 1 of .4mc and .4mz and the LZ4-fast / zstd-fast block streams run all of it, one higher
level per family the part whose blocks stay below 256 KiB.  Every output region is its queried size, lies between guard bytes of one
value, and everything outside the written regions must still hold that value afterwards - in d_packed and d_writes too.  Then the
one rule (the writers equal compress_images_writes / compress_bstreams on the packed text and table) and the readers."""
import numpy as np
import pytest
import torch

import bstream_model as bm
import bstream_writes_model as wm
import fourmc_stream_model as fm
import text_output_model as tm

pytestmark = pytest.mark.gpu

M = tm.M
MC, MZ = fm.MAGIC_4MC, fm.MAGIC_4MZ
CANARY, GUARD, SLACK = 0xA7, 64, 4096
WCANARY = 0x7A7A7A7A
FULL = [("img", MC, 1), ("img", MZ, 1), ("bs", 0, 0), ("bs", 3, 1)]
HIGH = [("img", MC, 3), ("img", MZ, 2), ("bs", 2, 4), ("bs", 3, 3)]
TARGETS = FULL + HIGH
NAMES = {("img", MC): "4mc", ("img", MZ): "4mz", ("bs", 0): "lz4_fast", ("bs", 2): "lz4_hc", ("bs", 3): "zstd"}
IDS = ["%s-%d" % (NAMES[k, a], lv) for k, a, lv in TARGETS]
ALIGN_LENGTHS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65)
_MEMO = {}


@pytest.fixture(scope="module")
def p(gpu):
    yield gpu
    _MEMO.clear()
    gpu.release_workspaces()
    torch.cuda.empty_cache()


# ---- the sources ----------------------------------------------------------------------------------------------------------------
class World:
    """lines in host lists, as a reader would have left them on the device, and the items of one call over them"""
    def __init__(self, row_bytes=0):
        self.buf, self.starts, self.tlen, self.items, self.row_bytes, self.pick = bytearray(), [], [], [], row_bytes, None

    def add(self, texts, aligns=None):
        """append table lines; aligns[i]: the line's start address mod 16 (None: wherever the one before ends)"""
        first = len(self.tlen)
        for i, t in enumerate(texts):
            if aligns is not None and aligns[i] is not None:
                self.buf += b"#" * ((aligns[i] - len(self.buf)) % 16)
            self.starts.append(len(self.buf)); self.tlen.append(len(t))
            self.buf += t
        return first, len(texts)

    def text_of(self, k):
        st = self.starts[k] if not self.row_bytes else k * self.row_bytes
        return bytes(self.buf[st:st + self.tlen[k]])

    def item(self, name, line_off, n_lines):
        """an item over entries [line_off, +n_lines) of the pick, or of the tables; its verdict and texts by the model"""
        picks = list(range(line_off, line_off + n_lines)) if self.pick is None else self.pick[line_off:line_off + n_lines]
        reason, T = tm.verdict(len(self.buf), self.tlen, None if self.row_bytes else self.starts, self.row_bytes, picks)
        texts = [self.text_of(k) for k in picks] if reason == tm.OK else None
        self.items.append(dict(name=name, line_off=line_off, n_lines=n_lines, reason=reason, T=T, texts=texts))

    def device(self, p):
        if "dev" not in self.__dict__:
            text = torch.from_numpy(np.frombuffer(bytes(self.buf) + bytes([CANARY]) * 64, np.uint8).copy()).cuda()
            tlen = torch.from_numpy(np.array(self.tlen, np.uint32).view(np.int32)).cuda()
            starts = None if self.row_bytes else torch.from_numpy(np.array(self.starts, np.int64)).cuda()
            pick = None if self.pick is None else torch.from_numpy(np.array(self.pick, np.int64)).cuda()
            self.dev = p.LinesSource(text, tlen, starts=starts, row_bytes=self.row_bytes, pick=pick, text_bytes=len(self.buf))
        return self.dev


def _align_lines():
    """the ten lengths at each of the 16 source alignments, each behind a filler that puts it at each of the 16 destination alignments"""
    texts, aligns, T, at = [], [], 0, 0
    for d in range(16):
        for a in range(16):
            for k in ALIGN_LENGTHS:
                f = (d - T - 1) % 16                      # the filler's piece ends where the line's first byte has address d mod 16
                texts += [tm.text(f, at), tm.text(k, at + f)]
                aligns += [None, a]
                T += f + 1 + k + 1
                at = (at + f + k) % 100000
    return texts, aligns


def packed_world(full):
    key = ("packed", full)
    if key in _MEMO:
        return _MEMO[key]
    w = World()
    if full:
        for name, lengths in tm.cut_lengths().items():
            first, n = w.add(tm.lines_of(lengths, at=len(name) * 1000))
            w.item(name, first, n)
    else:
        w.item("[0, 0, 3, 0]", *w.add(tm.lines_of([0, 0, 3, 0])))
        w.item("no line", len(w.tlen), 0)
    w.item("alignments", *w.add(*_align_lines()))
    w.item("long line", *w.add(tm.lines_of([1] * 5 + [100000] + [1] * 5, at=777)))
    first, n = w.add(tm.lines_of([int(v) for v in np.random.default_rng(5).integers(0, 40, 130)], at=31))
    w.item("tile a", first, 100)                          # the item boundary lies inside a tile of the table
    bad = len(w.tlen)
    w.starts.append(0); w.tlen.append(0x80000000)        # a length no write() may have
    w.item("write", bad - 3, 4)
    w.item("tile b", first + 100, 30)
    over = len(w.buf)
    w.buf += tm.text(70, 4242)
    w.starts += [over, over + 10]; w.tlen += [50, 60]    # two lines that overlap in the source
    w.item("overlap", len(w.tlen) - 2, 2)
    first, n = w.add(tm.lines_of([33, 0, 17], at=99))     # the last one ends with the text
    w.starts.append(w.starts[-1]); w.tlen.append(18)     # ... and this one a byte behind it
    w.item("end plus one", first, 4)
    w.item("end exact", first, 3)
    _MEMO[key] = w
    return w


def pick_world():
    if "pick" in _MEMO:
        return _MEMO["pick"]
    base = packed_world(False)
    w = World()
    w.buf, w.starts, w.tlen = base.buf, base.starts, base.tlen
    lo = next(it["line_off"] for it in base.items if it["name"] == "alignments")
    down = [lo + 300 - k // 2 for k in range(400)]        # descending, every line twice
    w.pick = down + [len(w.tlen)] + [lo + 7, lo + 7, lo + 7, 0, lo + 2000]
    w.item("descending with duplicates", 0, 400)
    w.item("the same picks again", 0, 400)
    w.item("its second half", 200, 200)
    w.item("a pick of no line", 398, 5)
    w.item("behind it", 401, 5)
    _MEMO["pick"] = w
    return w


def row_world():
    if "rows" in _MEMO:
        return _MEMO["rows"]
    w = World(row_bytes=24)
    lens = [int(v) for v in np.random.default_rng(9).integers(0, 25, 40)]
    lens[17] = 24
    for i, k in enumerate(lens + [25]):
        w.buf += tm.text(24, 50 * i)
        w.tlen.append(k)
    w.buf += b"#" * 24                                    # the bytes a 25th column would be read from
    w.tlen.append(3)
    w.item("rows 0-19", 0, 20)
    w.item("a row cut short by the reader", 30, 11)
    w.item("rows 17-39", 17, 23)
    w.item("the row behind it", 41, 1)
    _MEMO["rows"] = w
    return w


WORLDS = {"packed": packed_world, "pick": lambda full: pick_world(), "rows": lambda full: row_world()}


# ---- the model ------------------------------------------------------------------------------------------------------------------
def compressor(kind, a, level):
    raw = fm.compressor(a, level) if kind == "img" else bm.oracle_compressor(a, level)

    def comp(b):
        k = ("blk", kind, a, level, b)
        if k not in _MEMO:
            _MEMO[k] = bytes(raw(b))
        return _MEMO[k]
    return comp


def want(kind, a, level, it):
    """(bytes, blocks, stored blocks, the query's image_bytes) of an item that is OK"""
    key = ("want", kind, a, level, it["name"], it["T"], hash(tuple(it["texts"])))
    if key not in _MEMO:
        sizes = tm.schedule(it["texts"])[1]
        if kind == "img":
            img, offs, lens, stored = tm.image(it["texts"], compressor(kind, a, level), a)
            _MEMO[key] = (img, len(lens), sum(stored), fm.worst_case(sizes))
        else:
            zstd = a == 3
            img, groups, chunks = tm.bstream(it["texts"], compressor(kind, a, level), zstd)
            _MEMO[key] = (img, chunks, 0, wm.worst_case(sizes, bm.max_input(zstd), lambda k: bm.block_bound(k, zstd)))
    return _MEMO[key]


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def write(p, kind, a, level, src, rows, d_images, **kw):
    if kind == "img":
        return p.write_lines_images(src, rows, d_images, a, level, **kw)
    return p.write_lines_bstreams(src, rows, d_images, a, level, **kw)


def run(p, kind, a, level, w, caps=None):
    """query, then one write into regions of the queried size (caps: {item: image_cap} instead) between guards.  Returns (results,
    the written bytes per item or None, the query, the rows, the image buffer)."""
    src = w.device(p)
    rows = [[it["line_off"], it["n_lines"], 0, 0] for it in w.items]
    query = write(p, kind, a, level, src, [tuple(r) for r in rows], None)
    at = GUARD
    for i, (r, q) in enumerate(zip(rows, query)):
        r[2], r[3] = at, (caps or {}).get(i, q["image_bytes"])
        at += r[3] + GUARD
    d_images = torch.full((at + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    res = write(p, kind, a, level, src, [tuple(r) for r in rows], d_images, images_bytes=at)
    out = d_images.cpu().numpy()
    covered = np.zeros(len(out), bool)
    got = []
    for r, st in zip(rows, res):
        assert st["name"] == p.BSTREAM_WRITE_REASONS[st["reason"]]
        if st["reason"] == 0:
            assert st["image_bytes"] <= r[3], st
            covered[r[2]:r[2] + st["image_bytes"]] = True
            got.append(out[r[2]:r[2] + st["image_bytes"]].tobytes())
        else:
            got.append(None)
    assert (out[~covered] == CANARY).all(), "bytes written outside the images"
    return res, got, query, rows, d_images


def the_run(p, kind, a, level, world):
    """the ONE call of a (target, level) over a world, shared by the tests"""
    key = ("run", kind, a, level, world)
    if key not in _MEMO:
        _MEMO[key] = run(p, kind, a, level, WORLDS[world]((kind, a, level) in FULL))
    return _MEMO[key]


def the_pack(p, world, full):
    """ONE pack_lines over a world: regions of exactly the queried size that abut, write slices that abut, guards around both.
    Returns (results, query, rows, d_packed, d_writes)."""
    key = ("pack", world, full)
    if key in _MEMO:
        return _MEMO[key]
    w = WORLDS[world](full)
    src = w.device(p)
    rows = [[it["line_off"], it["n_lines"], 0, 0, 0] for it in w.items]
    query = p.pack_lines(src, [tuple(r) for r in rows], None)
    at, wat = GUARD + 1, 3                                # the first region starts at an odd byte
    for r, q, it in zip(rows, query, w.items):
        r[2], r[3], r[4] = at, q["packed_bytes"], wat
        at += r[3]
        wat += 2 * it["n_lines"]
    d_packed = torch.full((at + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_writes = torch.full((wat + 5,), WCANARY, dtype=torch.int32, device="cuda")
    res = p.pack_lines(src, [tuple(r) for r in rows], d_packed, d_writes)
    torch.cuda.synchronize()
    _MEMO[key] = (res, query, rows, d_packed, d_writes)
    return _MEMO[key]


def check_against_model(w, kind, a, level, res, got, query):
    for it, st, q, g in zip(w.items, res, query, got):
        assert st["reason"] == it["reason"] == q["reason"], (it["name"], st, q)
        assert st["text_bytes"] == it["T"] == q["text_bytes"], (it["name"], st)
        if it["reason"] != tm.OK:
            assert g is None and (st["image_bytes"], st["blocks"], st["stored_blocks"]) == (0, 0, 0) == (q["image_bytes"], q["blocks"], q["stored_blocks"]), it["name"]
            continue
        img, blocks, stored, worst = want(kind, a, level, it)
        assert (st["image_bytes"], st["blocks"], st["stored_blocks"]) == (len(img), blocks, stored), (it["name"], st, len(img), blocks, stored)
        assert g == img, (it["name"], next((k for k in range(min(len(img), len(g))) if g[k] != img[k]), "length"))
        assert (q["image_bytes"], q["blocks"], q["stored_blocks"]) == (worst, blocks, 0), (it["name"], q, worst)


# ---- the pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,full", [("packed", True), ("packed", False), ("pick", False), ("rows", False)], ids=["catalogue", "reduced", "pick", "rows"])
def test_pack_equals_the_models_data_and_write_sizes(p, world, full):
    w = WORLDS[world](full)
    res, query, rows, d_packed, d_writes = the_pack(p, world, full)
    out, tab = d_packed.cpu().numpy(), d_writes.cpu().numpy()
    covered, wcovered = np.zeros(len(out), bool), np.zeros(len(tab), bool)
    for it, st, q, r in zip(w.items, res, query, rows):
        assert st == q and st["name"] == p.BSTREAM_WRITE_REASONS[st["reason"]], (it["name"], st, q)
        assert (st["reason"], st["packed_bytes"]) == (it["reason"], it["T"]), (it["name"], st)
        if it["reason"] != tm.OK:
            continue
        data, sizes = tm.schedule(it["texts"])
        g = out[r[2]:r[2] + it["T"]].tobytes()
        assert g == data, (it["name"], next((k for k in range(len(data)) if g[k] != data[k]), None))
        assert tab[r[4]:r[4] + len(sizes)].tolist() == sizes, it["name"]
        covered[r[2]:r[2] + it["T"]] = True
        wcovered[r[4]:r[4] + len(sizes)] = True
    assert (out[~covered] == CANARY).all(), "bytes written outside the packed regions"
    assert (tab[~wcovered] == WCANARY).all(), "entries written outside the write slices"
    if world == "packed":
        by = {it["name"]: it for it in w.items}
        assert [by[n]["reason"] for n in ("write", "end plus one", "end exact", "overlap", "tile a", "tile b")] == [tm.WRITE, tm.LINE, 0, 0, 0, 0]
        assert by["alignments"]["n_lines"] == 2 * 16 * 16 * len(ALIGN_LENGTHS) and by["no line"]["T"] == 0
        assert any(r[2] % 2 and r[3] % 2 for r in rows)  # regions that abut at odd bytes
    if world == "pick":
        assert [it["reason"] for it in w.items] == [0, 0, 0, tm.LINE, 0]
    if world == "rows":
        assert [it["reason"] for it in w.items] == [0, tm.LINE, 0, 0] and w.tlen[17] == 24


def test_pack_cap_one_byte_short(p):
    w = packed_world(False)
    src = w.device(p)
    i = next(k for k, it in enumerate(w.items) if it["name"] == "long line")
    rows, at = [], GUARD
    for k, it in enumerate(w.items):
        cap = it["T"] - (1 if k == i else 0)
        rows.append((it["line_off"], it["n_lines"], at, cap, 2 * sum(q["n_lines"] for q in w.items[:k])))
        at += cap + 3
    d_packed = torch.full((at + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_writes = torch.full((2 * sum(q["n_lines"] for q in w.items) + 4,), WCANARY, dtype=torch.int32, device="cuda")
    res = p.pack_lines(src, rows, d_packed, d_writes)
    out, tab = d_packed.cpu().numpy(), d_writes.cpu().numpy()
    for k, (it, st, r) in enumerate(zip(w.items, res, rows)):
        if k == i:
            assert (st["name"], st["packed_bytes"]) == ("CAP", it["T"])
            assert (out[r[2] - 3:r[2] + r[3] + 3] == CANARY).all() and (tab[r[4]:r[4] + 2 * it["n_lines"]] == WCANARY).all()
        elif it["reason"] == tm.OK:
            assert st["name"] == "OK" and out[r[2]:r[2] + it["T"]].tobytes() == tm.schedule(it["texts"])[0], it["name"]


# ---- the writers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,a,level", TARGETS, ids=IDS)
def test_catalogue_equals_the_model(p, kind, a, level):
    full = (kind, a, level) in FULL
    res, got, query, rows, _ = the_run(p, kind, a, level, "packed")
    w = packed_world(full)
    check_against_model(w, kind, a, level, res, got, query)
    by = {it["name"]: st for it, st in zip(w.items, res)}
    assert [by[n]["name"] for n in ("tile a", "write", "tile b", "end plus one", "end exact")] == ["OK", "WRITE", "OK", "LINE", "OK"]
    assert by["no line"]["image_bytes"] == (44 if kind == "img" else 4)
    if full and kind == "img":
        assert [by[n]["blocks"] for n in ("[M-1]", "[M]", "[M+1]", "[M-2, 5]", "[0, 0, 3, 0]", "no line", "70000 lines")] == [1, 2, 3, 2, 1, 0, 2]
        assert by["[M]"]["stored_blocks"] == 1 and by["[M+1]"]["stored_blocks"] == 2


@pytest.mark.parametrize("kind,a,level", TARGETS, ids=IDS)
@pytest.mark.parametrize("world", ["pick", "rows"])
def test_picks_and_rows_equal_the_model(p, kind, a, level, world):
    res, got, query, rows, _ = the_run(p, kind, a, level, world)
    w = WORLDS[world](False)
    check_against_model(w, kind, a, level, res, got, query)
    if world == "pick":
        assert got[0] == got[1] and got[0] is not None and got[3] is None


@pytest.mark.parametrize("kind,a,level", TARGETS, ids=IDS)
def test_the_one_rule(p, kind, a, level):
    """each item's bytes, results and size query equal those of compress_images_writes / compress_bstreams on the packed text and table"""
    full = (kind, a, level) in FULL
    w = packed_world(full)
    res, got, query, rows, _ = the_run(p, kind, a, level, "packed")
    pres, _, prows, d_packed, d_writes = the_pack(p, "packed", full)
    direct = [(pr[2], it["T"], r[2], r[3], pr[4], 2 * it["n_lines"], 0) if it["reason"] == tm.OK else (0, 0, 0, 0, 0, 0, 0)
              for it, pr, r in zip(w.items, prows, rows)]
    fn = p.compress_images_writes if kind == "img" else p.compress_bstreams
    dq = fn(d_packed, direct, None, a, level, d_writes=d_writes)
    d_images = torch.full((rows[-1][2] + rows[-1][3] + GUARD + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    dr = fn(d_packed, direct, d_images, a, level, d_writes=d_writes, images_bytes=rows[-1][2] + rows[-1][3] + GUARD)
    out = d_images.cpu().numpy()
    count = "blocks" if kind == "img" else "chunks"
    for it, st, q, g, d, e, r in zip(w.items, res, query, got, dr, dq, rows):
        if it["reason"] != tm.OK:
            continue
        assert (d["reason"], e["reason"]) == (0, 0), (it["name"], d, e)
        assert (st["image_bytes"], st["blocks"], st["stored_blocks"]) == (d["image_bytes"], d[count], d.get("stored_blocks", 0)), (it["name"], st, d)
        assert (q["image_bytes"], q["blocks"]) == (e["image_bytes"], e[count]), (it["name"], q, e)
        assert g == out[r[2]:r[2] + d["image_bytes"]].tobytes(), it["name"]


@pytest.mark.parametrize("kind,a,level", FULL[:1] + FULL[2:3], ids=["4mc-1", "lz4_fast-0"])
def test_cap_one_byte_short_between_good_items(p, kind, a, level):
    w = packed_world(False)
    query = write(p, kind, a, level, w.device(p), [(it["line_off"], it["n_lines"], 0, 0) for it in w.items], None)
    i = next(k for k, it in enumerate(w.items) if it["name"] == "long line")
    res, got, _, rows, _ = run(p, kind, a, level, w, caps={i: query[i]["image_bytes"] - 1})
    assert res[i]["name"] == "CAP" and got[i] is None and res[i]["image_bytes"] == query[i]["image_bytes"] and res[i]["text_bytes"] == w.items[i]["T"]
    for k, (it, st, g) in enumerate(zip(w.items, res, got)):
        if k != i and it["reason"] == tm.OK:
            assert g == want(kind, a, level, it)[0], it["name"]


# ---- the readers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,a,level", FULL, ids=IDS[:4])
def test_decompress_gives_the_data(p, kind, a, level):
    w = packed_world(True)
    res, got, _, rows, d_images = the_run(p, kind, a, level, "packed")
    good = [(it, r, st) for it, r, st in zip(w.items, rows, res) if it["reason"] == tm.OK]
    dst_off = np.concatenate([[0], np.cumsum([it["T"] + 7 for it, _, _ in good])])
    d_dst = torch.full((int(dst_off[-1]) + 64,), CANARY, dtype=torch.uint8, device="cuda")
    items = [(r[2], st["image_bytes"], int(dst_off[i]), it["T"]) for i, (it, r, st) in enumerate(good)]
    back = p.decompress_images(d_images, items, d_dst, a) if kind == "img" else p.decompress_bstreams(d_images, items, d_dst, a)
    out = d_dst.cpu().numpy()
    for i, ((it, r, st), b) in enumerate(zip(good, back)):
        assert b["reason"] == 0 and b["total_bytes"] == it["T"], (it["name"], b)
        assert out[dst_off[i]:dst_off[i] + it["T"]].tobytes() == tm.schedule(it["texts"])[0], it["name"]
        assert (out[dst_off[i] + it["T"]:dst_off[i + 1]] == CANARY).all(), it["name"]


def _image(p, magic, name):
    """(item, a device copy of its image from the shared run, its size)"""
    w = packed_world(True)
    i = next(k for k, it in enumerate(w.items) if it["name"] == name)
    res, got, _, rows, d_images = the_run(p, "img", magic, 1, "packed")
    n = res[i]["image_bytes"]
    d_img = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d_img[:n] = d_images[rows[i][2]:rows[i][2] + n]
    return w.items[i], d_img, n


def _read_lines(p, d_img, n, lines, data_bytes):
    d_dst = torch.full((data_bytes + 100 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_st = torch.full((lines + 4,), -7, dtype=torch.int64, device="cuda")
    d_tl = torch.full((lines + 4,), -9, dtype=torch.int32, device="cuda")
    r = p.image_read_lines(d_img, 0, n, d_dst[:data_bytes + 100], d_st, d_tl, image_bytes=n)
    torch.cuda.synchronize()
    return r, d_dst, d_st, d_tl


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_read_lines_gives_back_starts_and_lengths(p, magic):
    for name in ("[M]", "[M-2, 5]", "[0, 0, 3, 0]", "70000 lines", "alignments", "long line", "overlap"):
        it, d_img, n = _image(p, magic, name)
        k = it["n_lines"]
        r, d_dst, d_st, d_tl = _read_lines(p, d_img, n, k, it["T"])
        assert (int(r.result), int(r.data_bytes)) == (k, it["T"]), (name, int(r.result))
        assert d_dst[:it["T"]].cpu().numpy().tobytes() == tm.schedule(it["texts"])[0], name
        assert d_tl.cpu().numpy()[:k].tolist() == [len(t) for t in it["texts"]], name
        assert d_st.cpu().numpy()[:k + 1].tolist() == np.concatenate([[0], np.cumsum([len(t) + 1 for t in it["texts"]])]).tolist(), name


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_round_trip_through_lines_by_number(p, magic):
    """rows of a shuffled pick read with image_read_lines_at, written in the row layout, read again: the picked lines"""
    it, d_img, n = _image(p, magic, "70000 lines")
    index, info = p.image_line_index(d_img, image_bytes=n)
    assert info["result"] == 0 and info["lines"] == 70000
    ks = torch.randperm(70000, generator=torch.Generator().manual_seed(11))[:777].contiguous()
    at = p.image_read_lines_at(d_img, index, ks.cuda(), 208, image_bytes=n)
    src = p.LinesSource(at["rows"], at["text_len"])
    assert src.row_bytes == 208 and src.table_lines == 777
    q = p.write_lines_images(src, [(0, 777, 0, 0)], None, magic, 1)
    d_out = torch.full((GUARD + q[0]["image_bytes"] + GUARD + 64,), CANARY, dtype=torch.uint8, device="cuda")
    st = p.write_lines_images(src, [(0, 777, GUARD, q[0]["image_bytes"])], d_out, magic, 1)
    texts = [it["texts"][int(k)] for k in ks]
    data = tm.schedule(texts)[0]
    assert st[0]["name"] == "OK" and st[0]["text_bytes"] == len(data) == q[0]["text_bytes"]
    m = st[0]["image_bytes"]
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == CANARY).all() and (out[GUARD + m:] == CANARY).all()
    d_new = torch.empty(m + 64, dtype=torch.uint8, device="cuda")
    d_new[:m] = d_out[GUARD:GUARD + m]
    r, d_dst, d_st, d_tl = _read_lines(p, d_new, m, 777, len(data))
    assert int(r.result) == 777 and d_dst[:len(data)].cpu().numpy().tobytes() == data
    assert d_tl.cpu().numpy()[:777].tolist() == [len(t) for t in texts]


# ---- arguments on the device ----------------------------------------------------------------------------------------------------
def test_nothing_to_do_and_queries_with_null_outputs(p):
    w = row_world()
    src = w.device(p)
    assert p.pack_lines(src, [], None) == [] and p.write_lines_images(src, [], None, MC, 1) == [] and p.write_lines_bstreams(src, [], None, 3, 1) == []
    d = torch.full((256,), CANARY, dtype=torch.uint8, device="cuda")
    assert p.write_lines_images(src, [], d, MZ, 1) == [] and bool((d == CANARY).all())
    q = p.pack_lines(src, [(0, 20, 0, 0, 0), (30, 11, 1 << 60, 1 << 61, 1 << 62)], None)
    assert [(s["name"], s["packed_bytes"]) for s in q] == [("OK", w.items[0]["T"]), ("LINE", 0)]
    q = p.write_lines_bstreams(src, [(0, 20, 1 << 60, 1 << 61)], None, 0, 0)
    assert q[0]["name"] == "OK" and q[0]["text_bytes"] == w.items[0]["T"] and q[0]["blocks"] == 1
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_write_lines failed \(-3\): images_write_lines: the lines of item 1"):
        p.write_lines_images(src, [(0, 20, 0, 100), (40, 3, 100, 100)], d, MC, 1)
    torch.cuda.synchronize()
    assert bool((d == CANARY).all())
