"""The lines of the splits of many images with one call on the device (fourmc_gpu_images_read_lines, _images_align_slices): every
item against the model of tests/lines_model.py and against fourmc_gpu_image_read_lines_batch on that image alone with the same
capacities.  The dataset is small on purpose: the families of lines_model.py for blocks of B = 40000 bytes (a multiple of neither
16 nor the 16 KiB scan tile), cut into blocks of B, encoded with encode_blocks as .4mc and as .4mz and framed with
assemble_container, so ~38 images of 0 to 4 blocks lie in one buffer of about 4 MB and a line longer than a block costs 40 KB."""
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
import lines_model as lm
import test_gpu_image_lines as one

pytestmark = pytest.mark.gpu
container = importlib.import_module("4mc_amd.container")

B = 40000
SENT, SSENT, TSENT = one.SENT, one.SSENT, one.TSENT
FIELDS = one.FIELDS
JUNK = 0xEE                                                 # between the images and in the slack behind the last


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def _families():
    rng = np.random.default_rng(2028)
    logs = helpers.corpus(4 * B, logs=True)
    assert not (logs == one.CR).any()
    at = [0]

    def text(n):
        a = np.roll(logs, -at[0])[:n].copy()
        at[0] += 12347
        return a

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return lm.families(B, text, noise)


class Img:
    """one image: its bytes, where its blocks lie and the model of its lines (the attributes test_gpu_image_lines.Case has)"""

    def __init__(self, p, name, z, data, csizes, sums, payloads):
        self.name, self.z, self.data = name, z, data
        self.usizes = [min(B, len(data) - o) for o in range(0, len(data), B)]
        self.csizes = [int(c) for c in csizes]
        self.img = p.assemble_container(p.MAGIC_4MZ if z else p.MAGIC_4MC, self.usizes, self.csizes, sums, payloads)
        self.size = len(self.img)
        self.offsets = [int(o) for o in container.block_offsets(self.csizes)] if self.csizes else []
        self.end_mark = self.offsets[-1] + 12 + self.csizes[-1] if self.offsets else 12
        self.model = lm.Model(data, self.offsets, self.usizes, self.end_mark)

    def splits(self, rng):
        return one.Case.splits(self, rng)


def _encode_all(p, fams, z):
    """every block of every family through ONE encode_blocks call -> {name: Img}"""
    names = list(fams)
    src = np.concatenate([fams[n] for n in names] + [np.zeros(64, np.uint8)])
    so, sl, owner, at = [], [], [], 0
    for n in names:
        for o in range(0, len(fams[n]), B):
            so.append(at + o); sl.append(min(B, len(fams[n]) - o)); owner.append(n)
        at += len(fams[n])
    batch = p.DeviceBatch(p.make_blocks(so, so, sl, sl))
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.zeros(len(src) + 64, dtype=torch.uint8, device="cuda")
    p.encode_blocks(d_src, d_dst, batch, p.CODEC_ZSTD if z else p.CODEC_LZ4_FAST, 1 if z else 0)
    enc, out = batch.download(), d_dst.cpu().numpy()
    res = {}
    for n in names:
        k = [i for i, w in enumerate(owner) if w == n]
        assert all(0 < enc["result"][i] <= sl[i] for i in k), (n, z)
        res[n] = Img(p, n, z, fams[n], [enc["result"][i] for i in k], [enc["xxh32"][i] for i in k],
                     [out[so[i]:so[i] + enc["result"][i]] for i in k])
    return res


class Dataset:
    """images in one device buffer: image i at an offset of residue i mod 16 (the few bytes between are junk), or abutting; 64
    bytes of slack behind the last.  raws: the images' bytes; imgs: the Img of each, None for one that is not a clean image."""

    def __init__(self, raws, imgs=None, abut=False):
        self.refs, off = [], 0
        for i, raw in enumerate(raws):
            if not abut:
                off += (i - off) % 16
            self.refs.append((off, len(raw)))
            off += len(raw)
        self.bytes = off + 64
        buf = np.full(self.bytes, JUNK, np.uint8)
        for (o, n), raw in zip(self.refs, raws):
            buf[o:o + n] = np.frombuffer(bytes(raw), np.uint8)
        self.d = torch.from_numpy(buf).cuda()
        self.imgs = list(imgs) if imgs is not None else [None] * len(raws)


@pytest.fixture(scope="module")
def world(p):
    """.imgs: the clean images, .4mc and .4mz alternating; .ds: all of them at every residue; .abut: the same, abutting"""
    fams = _families()
    mc, mz = _encode_all(p, fams, False), _encode_all(p, fams, True)
    imgs = []
    for n in fams:
        imgs += [mc[n], mz[n]]

    class W:
        pass
    w = W()
    w.imgs, w.by = imgs, {(i.name, "4mz" if i.z else "4mc"): i for i in imgs}
    w.ds = Dataset([i.img for i in imgs], imgs)
    w.abut = Dataset([i.img for i in imgs], imgs, abut=True)
    assert 30 <= len(imgs) <= 48 and w.ds.bytes < 6 << 20
    assert {len(i.offsets) for i in imgs} == {0, 1, 2, 3, 4}
    yield w
    p.release_workspaces()
    torch.cuda.empty_cache()


class Call:
    """One images_read_lines call, or the one-image calls that define it (`single`): the regions packed into one destination and
    one pair of tables, and what came back, on the host.  rows: (image, split_start, split_end, dst_cap, lines_cap).  guards:
    sentinel bytes in front of every region with region i at an offset of residue phase + i mod 16 (table region i behind
    1 + i % 5 sentinel entries); without, the regions abut."""

    def __init__(self, p, ds, rows, guards=True, count_only=False, stream=None, max_line_len=lm.DEFAULT_MAX, tdtype=torch.int32, phase=0,
                 single=False):
        self.ds, self.rows, self.count_only, self.max_line_len = ds, rows, count_only, max_line_len
        off, toff, self.items = 0, 0, []
        for i, (im, s, e, cap, lcap) in enumerate(rows):
            if guards:
                off += 16
                off += (phase + i - off) % 16
                toff += 1 + i % 5
            self.items.append((im, s, e, off, cap, toff, lcap))
            off += cap
            toff += lcap
        d_dst = torch.full((off + 64,), SENT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((toff + 8,), SSENT, dtype=torch.int64, device="cuda")
        d_tl = torch.full((toff + 8,), TSENT, dtype=torch.int32, device="cuda")
        st, tl = (None, None) if count_only else (d_st, d_tl.view(tdtype))
        if stream is not None:
            torch.cuda.synchronize()
        if single:
            self.out = [None] * len(rows)
            for k in sorted({it[0] for it in self.items}):
                idx = [i for i, it in enumerate(self.items) if it[0] == k]
                o, n = ds.refs[k]
                got = p.image_read_lines_batch(ds.d[o:], [self.items[i][1:] for i in idx], d_dst, st, tl, max_line_len=max_line_len,
                                               image_bytes=n, stream=stream)
                for i, g in zip(idx, got):
                    self.out[i] = g
        else:
            self.out = p.images_read_lines(ds.d, ds.refs, self.items, d_dst, st, tl, max_line_len=max_line_len, images_bytes=ds.bytes,
                                           stream=stream)
        torch.cuda.synchronize()
        self.dst, self.st, self.tl = d_dst.cpu().numpy(), d_st.cpu().numpy(), d_tl.cpu().numpy()

    def region(self, i):
        _, _, _, off, cap, _, _ = self.items[i]
        return self.dst[off:off + cap]

    def tables(self, i):
        toff, lcap = self.items[i][5:]
        return self.st[toff:toff + lcap], self.tl[toff:toff + lcap]

    def outside_untouched(self, key=None):
        may, tmay = np.zeros(len(self.dst), bool), np.zeros(len(self.st), bool)
        for _, _, _, off, cap, toff, lcap in self.items:
            may[off:off + cap] = True
            tmay[toff:toff + lcap] = True
        assert (self.dst[~may] == SENT).all(), (key, "bytes written outside the regions")
        assert (self.st[~tmay] == SSENT).all() and (self.tl[~tmay] == TSENT).all(), (key, "table entries written outside the regions")
        if self.count_only:
            assert (self.st == SSENT).all() and (self.tl == TSENT).all(), (key, "count only wrote a table")

    def equals(self, ref, key=None, items=None, other=None):
        """item for item what `ref` holds (the one-image calls, or another call with the same rows): the fields, the content up to
        data_bytes, the tables' whole regions; a region `ref` leaves untouched is untouched.  items / other: item items[j] of
        this call against item other[j] of ref."""
        items = range(len(self.items)) if items is None else items
        other = items if other is None else other
        for i, j in zip(items, other):
            got, res = self.out[i], ref.out[j]
            assert {f: got[f] for f in FIELDS} == {f: res[f] for f in FIELDS}, (key, i, self.items[i], got, res)
            nb = res["data_bytes"] if res["result"] >= 0 or res["reserved"] else 0
            assert np.array_equal(self.region(i)[:nb], ref.region(j)[:nb]), (key, i, "content")
            if (ref.region(j) == SENT).all():
                assert (self.region(i) == SENT).all(), (key, i, "the reference leaves the region untouched")
            (a, b), (c, d) = self.tables(i), ref.tables(j)
            assert np.array_equal(a, c) and np.array_equal(b, d), (key, i, "tables")

    def equals_model(self, key=None):
        """every item of a clean image against the model"""
        n = 0
        for i, (im, s, e, _, cap, _, lcap) in enumerate(self.items):
            c = self.ds.imgs[im]
            if c is None:
                continue
            c.model.max_line_len = self.max_line_len
            want = c.model.lines(s, e, dst_cap=cap, lines_cap=None if self.count_only else lcap)
            res = self.out[i]
            assert {f: res[f] for f in FIELDS} == {f: want[f] for f in FIELDS}, (key, i, self.items[i], res, {f: want[f] for f in FIELDS})
            if res["result"] >= 0 or (res["result"] == -5 and res["data_bytes"] <= cap):     # the -5 of lines_cap comes after the content
                nb = res["data_bytes"]
                assert np.array_equal(self.region(i)[:nb], c.data[want["base"]:want["base"] + nb]), (key, i, "content")
            else:
                assert (self.region(i) == SENT).all(), (key, i, "a refused item's region was written")
            st, tl = self.tables(i)
            k = res["result"]
            if self.count_only or k < 0:
                assert (st == SSENT).all() and (tl == TSENT).all(), (key, i, "tables written")
            else:
                assert np.array_equal(st[:k + 1], want["starts"]) and (st[k + 1:] == SSENT).all(), (key, i, "starts")
                assert np.array_equal(tl[:k], want["text_len"].astype(np.int32)) and (tl[k:] == TSENT).all(), (key, i, "text_len")
            n += 1
        return n


def _rows(ds, which, rng, exact=False, max_line_len=lm.DEFAULT_MAX):
    """the splits test_gpu_image_lines.Case.splits enumerates for the images `which` of ds, with room to spare (or none)"""
    rows = []
    for k in which:
        c = ds.imgs[k]
        c.model.max_line_len = max_line_len
        for s, e in c.splits(rng):
            w = c.model.lines(s, e)
            i = len(rows)
            rows.append((k, s, e, w["need"] + (0 if exact else (i * 7) % 23), max(w["result"], 0) + 1 + (0 if exact else i % 3)))
    return rows


def _both(p, ds, rows, key=None, **kw):
    """the call, checked against the one-image calls and the model"""
    call = Call(p, ds, rows, **kw)
    call.equals(Call(p, ds, rows, single=True, **kw), key)
    call.equals_model(key)
    call.outside_untouched(key)
    return call


# ---- 1: every split of every image, one call -------------------------------------------------------------------------------
def test_every_split_of_every_image_in_one_call(p, world):
    rng = np.random.default_rng(21)
    rows = _rows(world.ds, range(len(world.imgs)), rng)
    rows = [rows[i] for i in rng.permutation(len(rows))]                 # shuffled across the images
    call = _both(p, world.ds, rows, "guards")
    assert len(rows) > 200 and {it[3] % 16 for it in call.items if it[4]} == set(range(16))
    assert min(r["result"] for r in call.out) >= 0 and sum(r["result"] for r in call.out) > 10000
    assert {o % 16 for o, _ in world.ds.refs} == set(range(16))


def test_abutting_regions_and_abutting_images(p, world):
    rng = np.random.default_rng(22)
    rows = _rows(world.abut, range(len(world.imgs)), rng, exact=True)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    call = _both(p, world.abut, rows, "abut", guards=False)
    assert all(a[3] + a[4] == b[3] and a[5] + a[6] == b[5] for a, b in zip(call.items, call.items[1:]))
    assert all(a[0] + a[1] == b[0] for a, b in zip(world.abut.refs, world.abut.refs[1:]))
    assert sum(1 for it in call.items if it[4] and it[3] % 16) > 100


# ---- 2: groups and what the statistics count -------------------------------------------------------------------------------
class _Env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old
        return False


def _counted(p, fn):
    a, one_image = p.images_lines_stats(), p.image_lines_batch_stats()
    out = fn()
    b = p.images_lines_stats()
    assert p.image_lines_batch_stats() == one_image, "the one-image call's counters moved"
    return out, tuple(y - x for x, y in zip(a, b))


def test_group_cuts_change_nothing_but_the_statistics(p, world):
    rng = np.random.default_rng(23)
    rows = _rows(world.ds, range(len(world.imgs)), rng)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    n = len(rows)
    with _Env("FOURMC_SPLIT_GROUP", None):
        Call(p, world.ds, rows)                                            # the workspaces have their size from here on
        base, (g, r, d, x) = _counted(p, lambda: Call(p, world.ds, rows))
    assert g == -(-n // 256) and x == 2, (g, x)
    assert d <= 2 * r + 2 * g and r >= 2, (g, r, d)                        # both formats: at most two decodes per round and per body phase
    for group in (1, 3):
        with _Env("FOURMC_SPLIT_GROUP", group):
            cut, (g, r, d, x) = _counted(p, lambda: Call(p, world.ds, rows))
        assert g == -(-n // group) and x == 2, (group, g, x)
        assert d <= 2 * r + 2 * g, (group, g, r, d)
        cut.equals(base, group)
        cut.outside_untouched(group)
        assert [o for o in cut.out] == [o for o in base.out]


@pytest.mark.parametrize("tag", ["4mc", "4mz"])
def test_one_format_with_one_tail_round_per_split_costs_two_decodes_a_group(p, world, tag):
    """every split ends at a block header and its tail block holds a line end: one round each, so rounds == groups, and with one
    format a round is one decode and the bodies are one decode"""
    which = [k for k, c in enumerate(world.imgs) if c.name in ("lf_only", "crlf_text", "mixed", "stored_block") and (tag == "4mz") == c.z]
    rows = []
    for k in which:
        c = world.imgs[k]
        heads = c.offsets
        for i in range(len(heads) - 1):
            w = c.model.lines(heads[i] if i else 0, heads[i + 1])
            assert c.model.doff[i + 1] < w["base"] + w["need"] < c.model.doff[i + 2] - 1, (c.name, i)   # hi inside the next block
            rows.append((k, heads[i] if i else 0, heads[i + 1], w["need"], w["result"] + 1))
    assert len(rows) >= 8
    for group in (None, 1, 3):
        with _Env("FOURMC_SPLIT_GROUP", group):
            Call(p, world.ds, rows)
            call, (g, r, d, x) = _counted(p, lambda: Call(p, world.ds, rows))
        assert g == -(-len(rows) // (group or 256)) and r == g and d == 2 * g and x == 2, (group, g, r, d, x)
        call.equals_model(group)


@pytest.mark.parametrize("tag", ["4mc", "4mz"])
def test_last_block_is_the_last_of_the_splits_own_image(p, world, tag):
    """Block 1 of the second image ends with a CR and is its first staged tail block with a line end; it is not that image's last
    block, so the LF that opens block 2 belongs to the line.  Image 0 has two blocks: block 1 would be ITS last."""
    first, c, d = world.by[("all_lf", tag)], world.by[("tail_only_cr_last_lf", tag)], world.by[("tail_only_cr_last", tag)]
    assert len(first.offsets) == 2 and len(c.offsets) == 4 and len(d.offsets) == 4
    assert c.model.lines(0, c.offsets[1])["data_bytes"] == 2 * B + 1 and d.model.lines(0, d.offsets[1])["data_bytes"] == 2 * B
    ds = Dataset([first.img, c.img, d.img], [first, c, d])
    rows = _rows(ds, range(3), np.random.default_rng(30))
    assert (1, 0, c.offsets[1]) in {r[:3] for r in rows} and (2, 0, d.offsets[1]) in {r[:3] for r in rows}
    _both(p, ds, rows, tag)


# ---- 3: isolation ----------------------------------------------------------------------------------------------------------
def test_a_bad_image_costs_only_its_own_items(p, world):
    rng = np.random.default_rng(24)
    clean = [world.by[k] for k in (("three_blocks", "4mc"), ("mixed", "4mz"), ("cr_at_block_end", "4mz"), ("lf_only", "4mc"),
                                   ("stored_block", "4mz"), ("one_block", "4mc"))]
    a = world.by[("lf_only", "4mz")]
    tgt, nb = world.by[("lf_only", "4mc")], a                              # nb: the neighbour whose header offsets tgt's splits borrow
    assert len(a.offsets) == 3 and nb.offsets[1] not in tgt.offsets and nb.offsets[2] not in tgt.offsets and nb.offsets[2] < tgt.end_mark
    small_z = world.by[("one_block", "4mz")]
    foot = bytearray(a.img); foot[-6] ^= 0x01
    flip = bytearray(a.img); flip[a.offsets[1] + 12 + a.csizes[1] // 2] ^= 0x10
    empty = world.by[("zero_blocks", "4mc")]
    assert empty.size == 44
    bad = {"footer": bytes(foot), "two streams": small_z.img + a.img, "0 bytes": b"", "11 bytes": a.img[:11], "no blocks": empty.img,
           "flipped": bytes(flip), "borrowed": tgt.img}
    # interleaved: a bad image between every two clean ones
    raws, imgs, where = [], [], {}
    names = list(bad)
    for i, c in enumerate(clean):
        raws.append(c.img); imgs.append(c)
        where[names[i]] = len(raws)
        raws.append(bad[names[i]]); imgs.append(None)
    where[names[6]] = len(raws)
    raws.append(bad[names[6]]); imgs.append(None)
    ds = Dataset(raws, imgs, abut=True)
    rows = _rows(ds, [k for k, c in enumerate(imgs) if c is not None], rng)
    nclean = len(rows)
    ds.imgs[where["borrowed"]] = tgt                                       # its -3s are the model's too
    for name in names:
        k = where[name]
        n = len(raws[k])
        for s, e in sorted(set(a.splits(rng))) if name in ("flipped", "two streams", "footer") else [(0, n), (0, 0), (12, max(n, 12))]:
            rows.append((k, s, e, 3 * B + 100, 4000))
    first_borrowed = len(rows)
    rows += [(where["borrowed"], nb.offsets[1], tgt.size, 3 * B, 4000), (where["borrowed"], 0, nb.offsets[2], 3 * B, 4000),
             (where["borrowed"], tgt.offsets[1], tgt.size, 3 * B, 4000)]
    order = rng.permutation(len(rows))
    shuffled = [rows[i] for i in order]
    call = _both(p, ds, shuffled, "isolation")
    at = {int(j): i for i, j in enumerate(order)}                         # row j is item at[j]
    # the codes, spelled out
    res = lambda j: call.out[at[j]]["result"]                              # noqa: E731
    for j in range(nclean, len(rows)):
        k, s, e = rows[j][:3]
        name = [n for n in names if where[n] == k][0]
        if name == "footer":
            assert res(j) == -2, (name, res(j))
        elif name == "two streams":
            assert res(j) < 0 and res(j) == res(nclean + [r[0] for r in rows[nclean:]].index(k)), (name, res(j))
        elif name in ("0 bytes", "11 bytes"):
            assert res(j) == -1, (name, res(j))
        elif name == "flipped":
            a.model.max_line_len = lm.DEFAULT_MAX
            w = a.model.lines(s, e)
            lo, hi = w["base"], w["base"] + w["need"]
            covers = w["result"] >= 0 and lo < a.model.doff[2] and hi > a.model.doff[1]
            assert (res(j) == -4) == covers and (covers or res(j) == w["result"]), (name, s, e, res(j), w["result"])
    assert [res(first_borrowed + i) for i in range(3)][:2] == [-3, -3] and res(first_borrowed + 2) >= 0
    assert sum(1 for j in range(nclean, len(rows)) if res(j) == -4) >= 3
    # the clean images' items, from a call without the others
    alone = Dataset([c.img for c in clean], clean)
    renum = {k: i for i, k in enumerate(k for k, c in enumerate(imgs) if c is not None)}    # imgs: before `borrowed` got its model
    ref = Call(p, alone, [(renum[r[0]],) + r[1:] for r in rows[:nclean]])
    call.equals(ref, "clean items", items=[at[j] for j in range(nclean)], other=list(range(nclean)))


# ---- 4: capacities, count only, max_line_len, table types, a side stream -----------------------------------------------------
def _capacity_rows(world, ds):
    rng = np.random.default_rng(25)
    rows = []
    for k, c in enumerate(ds.imgs):
        for s, e in c.splits(rng):
            c.model.max_line_len = lm.DEFAULT_MAX
            w = c.model.lines(s, e)
            need, lines = w["need"], max(w["result"], 0)
            rows += [(k, s, e, 0, lines + 1), (k, s, e, need, lines + 1)]
            if need:
                rows.append((k, s, e, need - 1, lines + 1))                # -5 with data_bytes
            rows.append((k, s, e, need + 5, lines))                       # -5 with reserved, the tables untouched
    return rows


@pytest.fixture(scope="module")
def small(world):
    imgs = [world.by[k] for k in (("three_blocks", "4mc"), ("mixed", "4mz"), ("cr_at_block_end", "4mz"), ("alternating_crlf", "4mc"),
                                  ("zero_blocks", "4mz"), ("tail_only_cr_last_lf", "4mc"))]
    return Dataset([c.img for c in imgs], imgs)


def test_capacities(p, world, small):
    rows = _capacity_rows(world, small)
    call = _both(p, small, rows, "capacities")
    got = [r for r in call.out]
    assert sum(1 for r, row in zip(got, rows) if row[3] == 0 and r["result"] == -5 and r["data_bytes"] > 0) > 10      # size queries
    assert sum(1 for r in got if r["result"] == -5 and r["reserved"]) > 10 and sum(1 for r in got if r["result"] > 0) > 10
    # the size query's answer is the capacity that works
    again = [(row[0], row[1], row[2], r["data_bytes"], row[4]) for r, row in zip(got, rows) if row[3] == 0]
    assert all(r["result"] >= 0 for r in _both(p, small, again, "queried").out)


@pytest.mark.parametrize("variant", ["count_only", "max0", "max7", "uint32", "stream"])
def test_count_only_line_limits_table_types_and_a_side_stream(p, world, small, variant):
    rng = np.random.default_rng(26)
    mx = {"max0": 0, "max7": 7}.get(variant, lm.DEFAULT_MAX)
    rows = _rows(small, range(len(small.imgs)), rng, max_line_len=mx)
    kw = {}
    if variant == "count_only":
        kw["count_only"] = True
    elif variant == "uint32":
        kw["tdtype"] = getattr(torch, "uint32", torch.int32)
    elif variant == "stream":
        kw["stream"] = torch.cuda.Stream()
    call = _both(p, small, rows, variant, max_line_len=mx, **kw)
    assert sum(r["result"] for r in call.out) > 1000


# ---- 5: the same bytes twice -----------------------------------------------------------------------------------------------
def test_the_same_image_twice_and_the_same_split_twice(p, world):
    c = world.by[("three_blocks", "4mz")]
    ds = Dataset([c.img], [c])
    ds.refs, ds.imgs = [ds.refs[0], ds.refs[0], (ds.refs[0][0], c.size)], [c, c, c]
    rows = []
    for s, e in c.splits(np.random.default_rng(27)):
        w = c.model.lines(s, e)
        rows += [(k, s, e, w["need"] + 3, w["result"] + 2) for k in (0, 1, 0, 2)]
    call = _both(p, ds, rows, "twice")
    for i in range(0, len(rows), 4):
        call.equals(call, "copies", items=[i + 1, i + 2, i + 3], other=[i, i, i])
    # overlapping images: a one-block image's bytes are also the tail of a region that starts 5 bytes earlier and cannot be indexed
    ob = world.by[("one_block", "4mc")]
    ds2 = Dataset([b"\x00" * 5 + ob.img], [None])
    ds2.refs, ds2.imgs = [(0, ob.size + 5), (5, ob.size)], [None, ob]
    w = ob.model.lines(0, ob.size)
    call = _both(p, ds2, [(0, 0, ob.size + 5, w["need"], w["result"] + 1), (1, 0, ob.size, w["need"], w["result"] + 1)], "overlap")
    assert call.out[0]["result"] == -2 and call.out[1]["result"] == w["result"] > 0


# ---- 6: real blocks --------------------------------------------------------------------------------------------------------
def test_images_of_4_mib_blocks(p):
    B4 = helpers.B
    logs = helpers.corpus(2 * B4 + 100000, logs=True)
    cases = [one.Case(p, "two_and_a_tail", False, logs), one.Case(p, "two_and_a_tail", True, logs[4321:].copy()),
             one.Case(p, "one_block", True, logs[:B4 // 4].copy())]
    assert [len(c.offsets) for c in cases] == [3, 3, 1]
    ds = Dataset([c.img for c in cases], cases)
    rng = np.random.default_rng(28)
    rows = _rows(ds, range(3), rng)
    try:
        call = Call(p, ds, rows)
        call.equals(Call(p, ds, rows, single=True), "4 MiB")
        call.equals_model("4 MiB")
        call.outside_untouched("4 MiB")
        assert len(rows) >= 12
    finally:
        del cases, ds
        p.release_workspaces()
        torch.cuda.empty_cache()


# ---- 7: decode settings ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["exact", "seg", "tile", "zsingle"])
def test_decode_settings_give_the_same_lines(p, world, setting):
    L = p.lib()
    path, split = L.fourmc_gpu_get_lz4_decode_path(), L.fourmc_gpu_get_zstd_decode_split()
    rng = np.random.default_rng(21)
    rows = _rows(world.ds, range(len(world.imgs)), rng)
    try:
        base = Call(p, world.ds, rows)
        if setting == "zsingle":
            L.fourmc_gpu_set_zstd_decode_split(0)
        else:
            L.fourmc_gpu_set_lz4_decode_path({"exact": 2, "seg": 11, "tile": 13}[setting])
        call = Call(p, world.ds, rows)
    finally:
        L.fourmc_gpu_set_lz4_decode_path(path)
        L.fourmc_gpu_set_zstd_decode_split(split)
    call.equals(base, setting)
    call.equals_model(setting)
    call.outside_untouched(setting)


# ---- 8: align --------------------------------------------------------------------------------------------------------------
def test_align_equals_the_one_image_call_and_its_partitions_read_every_line_once(p, world):
    a = world.by[("lf_only", "4mz")]
    foot = bytearray(a.img); foot[-6] ^= 0x01
    raws = [c.img for c in world.imgs] + [bytes(foot), world.by[("one_block", "4mz")].img + a.img, b"", a.img[:11]]
    ds = Dataset(raws, world.imgs + [None] * 4)
    slices, thirds = [], {}
    for k, raw in enumerate(raws):
        n = len(raw)
        slices += [(k, 0, e) for e in (0, 1, 11, 12)]
        edges = [0, n // 3, 2 * n // 3, n]
        thirds[k] = range(len(slices), len(slices) + 3)
        slices += [(k, x, y) for x, y in zip(edges, edges[1:])]
        c = ds.imgs[k]
        if c is not None and len(c.offsets) >= 2:
            slices.append((k, c.offsets[0] + 1, c.offsets[1]))            # finds no block before its end: dropped
            slices.append((k, c.offsets[-1] + 1, n + 100))
    order = np.random.default_rng(29).permutation(len(slices))
    got = p.images_align_slices(ds.d, ds.refs, [slices[i] for i in order], images_bytes=ds.bytes)
    got = {int(j): g for j, g in zip(order, got)}
    dropped = 0
    for k, (o, n) in enumerate(ds.refs):
        mine = [j for j, sl in enumerate(slices) if sl[0] == k]
        want = p.image_align_slices(ds.d[o:], [slices[j][1:] for j in mine], image_bytes=n)
        for j, w in zip(mine, want):
            assert got[j] == dict(w, image=k), (k, slices[j], got[j], w)
            if ds.imgs[k] is not None:
                m = lm.align_slice(ds.imgs[k].offsets, slices[j][1], slices[j][2], n)
                assert {f: got[j][f] for f in m} == m, (k, slices[j], got[j], m)
                dropped += got[j]["result"] == 0
    assert dropped >= 20
    codes = {got[j]["result"] for j in range(len(slices)) if slices[j][0] >= len(world.imgs)}
    assert {-1, -2} <= codes and max(codes) < 0
    empty = [k for k, c in enumerate(world.imgs) if not c.offsets]
    assert all(got[j]["result"] == 1 and got[j]["split_end"] == slices[j][2] for j in range(len(slices)) if slices[j][0] in empty)
    # the kept thirds of every clean image, read in one call: every line exactly once
    rows, owner = [], []
    for k, c in enumerate(world.imgs):
        c.model.max_line_len = lm.DEFAULT_MAX
        for j in thirds[k]:
            if got[j]["result"] == 1:
                w = c.model.lines(got[j]["split_start"], got[j]["split_end"])
                rows.append((k, got[j]["split_start"], got[j]["split_end"], w["need"], max(w["result"], 0) + 1))
                owner.append(k)
    call = Call(p, ds, rows)
    call.equals_model("thirds")
    lines = {k: [] for k in range(len(world.imgs))}
    for i, k in enumerate(owner):
        r = call.out[i]
        lines[k] += (r["base"] + call.tables(i)[0][:max(r["result"], 0)]).tolist()
    for k, c in enumerate(world.imgs):
        assert lines[k] == c.model.file_lines()[:-1].tolist(), (c.name, c.z)
