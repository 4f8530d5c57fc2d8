"""fourmc_gpu_images_compress_writes / fourmc_gpu_image_writes_bound without a GPU: Hadoop's FourMcOutputStream restated buffer by
buffer (tests/fourmc_stream_model.py) against the rule in closed form and the block streams' grouping rule, the bound against every
schedule, the model's images at the real block size read by the oracle and by the reference's own reader, the symbols, and every
argument error refused before a device is looked for."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bstream_writes_model as wm
import fourmc_stream_cases as cases
import fourmc_stream_model as fm
import helpers

ROOT = helpers.ROOT
OK, ENODEV, EINVAL, EUNSUP = 0, -1, -3, -5
MC, MZ = fm.MAGIC_4MC, fm.MAGIC_4MZ
NAMES = ["fourmc_gpu_images_compress_writes", "fourmc_gpu_image_writes_bound"]
NO_REF = "oracle/_ref is missing: __graft_entry__.build() makes it where the reference tree exists"


def shrink(b):
    """a fake compressor: one byte shorter than its input, so every block above one byte is written compressed"""
    return bytes(len(b) - 1) if len(b) > 1 else b"\x07"


def grow(b):
    """a fake compressor whose result passes the stream's byte buffer: every block is stored, and at a small M the part of the result
    the buffer did not take is dropped by the stored branch's reset()"""
    return b"\xEE" * (2 * len(b) + 3)


def model_cuts(sizes, M, comp):
    data = bytes(range(256)) * (sum(sizes) // 256 + 1)
    img = fm.write_image(data[:sum(sizes)], sizes, comp, MC, M)
    return [u for _, u, _, _ in fm.parse(img)], img


# ---- the cuts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 5, 8])
def test_every_schedule_stream_model_equals_closed_form_equals_the_block_streams_plan(M):
    """Every schedule of up to 6 writes of 0 .. 2M + 1 bytes.  There are 18^6 of them at M = 8, so they are not run one by one: the
    stream model is a state machine whose whole state after a write is (position of the direct buffer, saved bytes, pending output,
    bytesRead, bytesWritten, finish, finished), the blocks a write emits depend on that state and the write alone, and the closed form
    is a state machine over `acc`.  The walk below visits every (stream state, acc, writes left) reachable from the start once, applies
    every write size to it and compares the blocks the two emit for that write, and what close() adds; two prefixes that reach the
    same pair of states have the same continuations, so this covers every schedule.  Beside it, the three are compared directly, image
    for image, on every schedule of up to 3 writes (4 at M = 4) and on the representative prefix of every state the walk met."""
    V = range(2 * M + 2)

    def key(s):
        c = s.c
        return (len(c.direct), len(c.user), len(c.out), c.bytes_read, c.bytes_written, c.finish_, c.finished_)

    def clone(s):
        t = fm.FourMcOutputStream(s.c.cb, MC, M)
        t.c.direct, t.c.user, t.c.out, t.c.mem = bytearray(s.c.direct), s.c.user, s.c.out, bytearray(s.c.mem)
        t.c.bytes_read, t.c.bytes_written, t.c.finish_, t.c.finished_ = s.c.bytes_read, s.c.bytes_written, s.c.finish_, s.c.finished_
        return t

    def step_closed(acc, w):
        """(blocks emitted by this write, acc after it): fm.cuts, one write at a time"""
        out = []
        if w == 0:
            return out, acc
        if acc > 0 and acc + w > M:
            out.append(acc)
            acc = 0
        if w > M:
            return out + [M] * (w // M) + ([w % M] if w % M else []), 0
        acc += w
        if acc == M:
            out.append(acc)
            acc = 0
        return out, acc

    for comp in (shrink, grow):
        seen, reps = set(), []
        todo = [(fm.FourMcOutputStream(comp, MC, M), 0, 6, ())]
        while todo:
            s, acc, left, prefix = todo.pop()
            k = (key(s), acc, left)
            if k in seen:
                continue
            seen.add(k)
            reps.append(prefix)
            fin = clone(s)
            fin.sink, fin.block_offsets = bytearray(), []
            fin.finish()
            assert [u for _, u, _, _ in fm.parse(b"\0" * 12 + bytes(fin.sink) + b"\0" * 12)] == ([acc] if acc else []), (M, prefix)
            if not left:
                continue
            for w in V:
                t = clone(s)
                t.sink, t.block_offsets = bytearray(), []
                t.write(bytes(w))
                got = [u for _, u, _, _ in fm.parse(b"\0" * 12 + bytes(t.sink) + b"\0" * 12)]
                want, acc2 = step_closed(acc, w)
                assert got == want, (M, prefix, w)
                todo.append((t, acc2, left - 1, prefix + (w,)))
        assert len(seen) > M
        direct = list(itertools.chain.from_iterable(itertools.product(V, repeat=k) for k in range(5 if M == 4 else 4))) + reps
        for sizes in direct:
            sizes = list(sizes)
            got, img = model_cuts(sizes, M, comp)
            want = fm.cuts(sizes, M)
            assert got == want == [c for _, cs in wm.plan(sizes, M)[0] for c in cs], (M, sizes)
            data = (bytes(range(256)) * (sum(sizes) // 256 + 1))[:sum(sizes)]
            closed, offs, lens, stored = fm.image(data, sizes, comp, MC, M)
            assert img == closed and [o for o, _, _, _ in fm.parse(img)] == offs, (M, sizes)
            assert len(img) <= fm.worst_case(sizes, M) <= fm.writes_bound(sum(sizes), M), (M, sizes)
            assert all(stored) if comp is grow else stored == [u <= 1 for u in lens]


def test_the_closed_form_steps_are_the_closed_form():
    """the one-write-at-a-time form used above is fm.cuts: on every schedule of up to 5 writes at M = 4"""
    M = 4
    for k in range(6):
        for sizes in itertools.product(range(2 * M + 2), repeat=k):
            blocks, acc = [], 0
            for w in sizes:
                if w and acc > 0 and acc + w > M:
                    blocks.append(acc); acc = 0
                if w > M:
                    blocks += [M] * (w // M) + ([w % M] if w % M else [])
                elif w:
                    acc += w
                    if acc == M:
                        blocks.append(acc); acc = 0
            assert blocks + ([acc] if acc else []) == fm.cuts(list(sizes), M)


@pytest.mark.parametrize("M", [4, 5, 8])
def test_plan_chunks_equal_cuts_on_longer_schedules(M):
    """the block streams' rule and this one, on every schedule of 5 writes at M = 4 and 5 and a seeded sample of 5 and 6 writes at 8"""
    V = range(2 * M + 2)
    rng = np.random.default_rng(M)
    some = itertools.product(V, repeat=5) if M < 8 else (tuple(int(v) for v in rng.integers(0, 2 * M + 2, 5 + k % 2)) for k in range(60000))
    for sizes in some:
        sizes = list(sizes)
        assert fm.cuts(sizes, M) == [c for _, cs in wm.plan(sizes, M)[0] for c in cs], sizes


# ---- the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 5, 8])
def test_bound_formula_is_the_most_blocks_of_any_schedule(M):
    """for every S up to 4M, over schedules of any number of writes: best[s][acc] = the most blocks already written by a schedule
    whose writes sum to s and leave acc bytes accumulated, by the closed form's transitions.  The formula is that maximum wherever
    S mod (M + 2) is 0, 1 or M + 1, and one above it for the remainders 2 .. M: two bytes behind a run of (1, M + 1) pairs accumulate
    into one block, and only a remainder of M + 1 is two blocks again.  (The formula is the documented bound and stays as it is: it
    holds everywhere and is off by at most one block, 16 bytes.)"""
    top = 4 * M
    NEG = -1
    best = [[NEG] * (M + 1) for _ in range(top + 1)]
    best[0][0] = 0
    for s in range(top + 1):
        for acc in range(M + 1):
            have = best[s][acc]
            if have < 0:
                continue
            for w in range(1, top - s + 1):
                n, a = have, acc
                if a > 0 and a + w > M:
                    n, a = n + 1, 0
                if w > M:
                    n, a = n + -(-w // M), 0
                else:
                    a += w
                    if a == M:
                        n, a = n + 1, 0
                best[s + w][a] = max(best[s + w][a], n)
    for S in range(top + 1):
        most = max(best[S][acc] + (1 if acc else 0) for acc in range(M + 1) if best[S][acc] >= 0)
        r = S % (M + 2)
        assert fm.max_blocks(S, M) == wm.max_chunks(S, M) == most + (1 if 2 <= r <= M else 0), (M, S, most)
    assert len(fm.cuts([1, M + 1] * 5, M)) == 15 == fm.max_blocks(5 * (M + 2), M)


def test_the_librarys_bound_is_the_formula_at_4_mib():
    p = helpers.pkg()
    M = fm.M4
    for k in range(4):
        for d in (-2, -1, 0, 1, 2, 3):
            S = k * (M + 2) + d
            if S >= 0:
                assert p.image_writes_bound(S) == fm.writes_bound(S, M) == 12 + 16 * fm.max_blocks(S, M) + S + 32, S
    for S in (0, 1, 2, M, M + 1, 1 << 30, (1 << 40) + 12345):
        assert p.image_writes_bound(S) == fm.writes_bound(S, M)
    assert p.image_writes_bound(0) == 44
    for c in cases.full():
        assert fm.worst_case(c.sizes) <= p.image_writes_bound(len(c.data)), c.name


# ---- the model's images at the real block size ------------------------------------------------------------------------------------
def _decode(img, magic):
    """the image's content by the oracle: the container decoder for .4mc, block by block for .4mz"""
    if magic == MC:
        n, out, used = helpers.orc_container_decode(np.frombuffer(img, np.uint8), sum(u for _, u, _, _ in fm.parse(img)) + 1)
        assert used == len(img)
        return out.tobytes() if n >= 0 else None
    out = b""
    for at, u, c, x in fm.parse(img):
        pay = img[at + 12:at + 12 + c]
        assert fm.xxh32(pay) == x
        if c == u:
            out += pay
        else:
            r, got = helpers.orc_zstd_decompress(pay, u)
            assert r == u
            out += got.tobytes()
    return out


@pytest.fixture(scope="module")
def model_images():
    """(magic) -> [(case, stream model's image)] at level 1, the closed form held against it"""
    out = {}
    for magic in (MC, MZ):
        comp = fm.compressor(magic, 1)
        rows = []
        for c in cases.full():
            img = fm.write_image(c.data, c.sizes, comp, magic)
            closed, offs, lens, stored = fm.image(c.data, c.sizes, comp, magic)
            assert img == closed, c.name
            rows.append((c, img, lens, stored))
        out[magic] = rows
    return out


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_model_images_decode_to_the_data(model_images, magic, tmp_path):
    cli = helpers.ref_cli()
    assert cli is not None, NO_REF
    M = fm.M4
    for c, img, lens, stored in model_images[magic]:
        assert lens == [k for _, cs in wm.plan(c.sizes, M)[0] for k in cs], c.name
        assert _decode(img, magic) == c.data, c.name
        if not c.data:
            assert len(img) == 44, c.name
    by = {c.name: (lens, stored) for c, _, lens, stored in model_images[magic]}
    assert by["[1]"] == ([1], [True]) and by["[M+1, 5]"][0] == [M, 1, 5] and by["[1, M+1]"][0] == [1, M, 1]
    assert by["[M-1, 1, 1]"][0] == [M, 1] and by["[M/2, M/2, 1]"][0] == [M, 1] and by["[M-1, 2]"][0] == [M - 1, 2] and by["[2M]"][0] == [M, M]
    assert by["noise [M]"][1] == [True] and by["noise [70000]"][1] == [True] and by["text then noise"][1] == [False, True]
    assert by["70000 writes of 100 with zeros"][0] == [4194300, 69992 * 100 - 4194300] and by["uniform M+1"][0] == [M, 1, 9]
    # the reference's own reader accepts what the model writes: one file of every image glued would hide which failed, so each alone,
    # the small ones only by their count of distinct shapes (the reader is the same code for all)
    for c, img, _, _ in model_images[magic]:
        f, o = tmp_path / "m.img", tmp_path / "m.out"
        f.write_bytes(img)
        r = subprocess.run([cli, "-d"] + (["-z"] if magic == MZ else []) + ["-f", str(f), str(o)], capture_output=True)
        assert r.returncode == 0, (c.name, r.stderr)
        assert o.read_bytes() == c.data, c.name


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_oracle_equals_reference_on_every_block_payload(model_images, magic):
    ref = helpers.ref()
    assert ref is not None, NO_REF
    n = 0
    for c, img, lens, stored in model_images[magic]:
        src = 0
        for (at, u, csz, _), st in zip(fm.parse(img), stored):
            raw = np.frombuffer(c.data[src:src + u], np.uint8)
            src += u
            cap = helpers.zstd_bound(u) if magic == MZ else helpers.oracle().orc_lz4_compress_bound(u)
            dst = np.empty(cap + 64, np.uint8)
            r = ref.ZSTD_compress(dst.ctypes.data, cap, raw.ctypes.data, u, 1) if magic == MZ else ref.LZ4_compress_default(raw.ctypes.data, dst.ctypes.data, u, cap)
            assert 0 < r <= cap
            assert st == (u <= r), c.name
            assert img[at + 12:at + 12 + csz] == (raw.tobytes() if st else dst[:r].tobytes()), (c.name, at)
            n += 1
    assert n >= 25


def test_one_write_of_compressible_text_is_the_clis_4mc_file(model_images):
    """for the LZ4 codecs the stream's stored rule (u <= c, unlimited output) and the CLI's (compress into u - 1 bytes) give the same file"""
    by = {c.name: (c, img) for c, img, _, _ in model_images[MC]}
    for name in ("[2M]", "uniform 0", "[1]", "noise [70000]", "noise [M]"):
        c, img = by[name]
        assert img == helpers.orc_container(np.frombuffer(c.data, np.uint8)).tobytes(), name


def test_4mz_stream_rule_against_the_clis_capacity_recorded():
    """.4mz: the CLI compresses each block into u - 1 bytes, the stream into the bound and then compares.  A few hundred seeded tries,
    noise mixed with a little text at 1 to 64 KiB, look for a block on which the two give different bytes while the result stays below
    u - which would be the capacity effect, not an error.  The outcome is recorded: the catalogue holds such a block if one exists."""
    text = helpers.corpus(1 << 20)
    found, below = [], 0
    for level in (1, 3, 6, 12):
        for seed in range(100):
            rng = np.random.default_rng(1000 + seed)
            n = int(rng.integers(1 << 10, (64 << 10) + 1))
            buf = rng.integers(0, 256, n, dtype=np.uint8)
            k = max(1, int(n * (0.01, 0.03, 0.06, 0.12, 0.25)[seed % 5]))
            parts = 1 + seed % 4
            for _ in range(parts):
                L = max(1, k // parts)
                at, t0 = int(rng.integers(0, max(1, n - L))), int(rng.integers(0, len(text) - L))
                buf[at:at + L] = text[t0:t0 + L]
            c, free = helpers.orc_zstd_compress(buf, level)
            c1, tight = helpers.orc_zstd_compress(buf, level, cap=n - 1)
            below += c < n
            if (c < n and (c1 != c or not np.array_equal(free, tight))) or (c >= n and c1 > 0):
                found.append((level, seed, n, c, c1))
    print("\n.4mz capacity search: %d tries, %d with c < u, %d where the capacity changes the block: %s" % (400, below, len(found), found[:5]))
    assert below > 50
    assert bool(found) == (cases.zstd_capacity_case() is not None), found[:5]
    # the whole-image comparison on compressible text, recorded as well: equal here
    c = next(c for c in cases.full() if c.name == "uniform 0")
    comp = fm.compressor(MZ, 1)
    img = fm.write_image(c.data, c.sizes, comp, MZ)
    r, tight = helpers.orc_zstd_compress(np.frombuffer(c.data, np.uint8), 1, cap=len(c.data) - 1)
    (_, u, csz, _), = fm.parse(img)
    assert r == csz and img[24:24 + csz] == tight.tobytes()


# ---- the symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    I = p.ImageWrItem
    assert C.sizeof(I) == 80 and I.reason.offset == 52 and I.image_bytes.offset == 56 and I.blocks.offset == 64 and I.stored_blocks.offset == 72
    for f in (p.compress_images_writes, p.image_writes_bound):
        assert callable(f)


# ---- arguments ------------------------------------------------------------------------------------------------------------------
SRC, TAB, IMAGES = 5000, 100, 16384
FIELDS = ("src_off", "src_bytes", "image_off", "image_cap", "writes_off", "n_writes", "write_bytes")
GOOD = [(0, 2500, 0, 4000, 0, 0, 1000), (2500, 0, 4000, 44, 0, 0, 0), (2500, 2500, 4044, 4000, 10, 5, 0), (0, 5000, 9000, 0, 0, 0, 0)]


def _items(p, rows):
    arr = (p.ImageWrItem * max(len(rows), 1))()
    for i, row in enumerate(rows):
        for f, v in zip(FIELDS, row):
            setattr(arr[i], f, v)
        arr[i].reason, arr[i].image_bytes, arr[i].blocks, arr[i].stored_blocks = 66, 77 + i, 88, 99
    return arr


def _call(p, rows, magic=MC, level=1, src=True, tab=True, images=True, n=None, items=True):
    L = p.lib()
    s = np.zeros(SRC, np.uint8)
    t = np.full(TAB, 500, np.uint32)
    img = np.full(IMAGES, 0xC3, np.uint8)
    arr = _items(p, rows)
    rc = L.fourmc_gpu_images_compress_writes(s.ctypes.data if src else None, SRC, t.ctypes.data if tab else None, TAB,
                                             img.ctypes.data if images else None, IMAGES, magic, level,
                                             C.cast(arr, C.c_void_p) if items else None, len(rows) if n is None else n, None)
    for i, row in enumerate(rows):                                  # the items are untouched, and so are the images
        assert tuple(getattr(arr[i], f) for f in FIELDS) == tuple(row), i
        assert (arr[i].reason, arr[i].image_bytes, arr[i].blocks, arr[i].stored_blocks) == (66, 77 + i, 88, 99), i
    assert (img == 0xC3).all()
    return rc


MANY_EINVAL = {
    "magic": (GOOD, dict(magic=0x344D4301)), "magic, everything else wrong too": (GOOD, dict(magic=0, src=False, tab=False, items=False)),
    "magic, size query": (GOOD, dict(magic=7, images=False)), "magic, no items": (GOOD, dict(magic=1, n=0)),
    "null items": (GOOD, dict(items=False)), "null source": (GOOD, dict(src=False)), "null table": (GOOD, dict(tab=False)),
    "null table, size query": (GOOD, dict(tab=False, images=False)), "null source, size query": (GOOD, dict(src=False, images=False)),
    "source starts beyond the buffer": ([(SRC + 1, 0, 0, 100, 0, 0, 0)], {}),
    "source ends beyond the buffer": ([(SRC - 9, 10, 0, 100, 0, 0, 0)], {}),
    "source ends beyond the buffer, size query": ([(SRC - 9, 10, 0, 100, 0, 0, 0)], dict(images=False)),
    "src_off + src_bytes wraps": ([(8, 2 ** 64 - 4, 0, 100, 0, 0, 0)], {}),
    "table range starts beyond the table": ([(0, 0, 0, 100, TAB + 1, 0, 0)], {}),
    "table range ends beyond the table": ([(0, 500, 0, 1000, TAB - 4, 5, 0)], {}),
    "table range ends beyond the table, size query": ([(0, 500, 0, 1000, TAB - 4, 5, 0)], dict(images=False)),
    "writes_off + n_writes wraps": ([(0, 500, 0, 1000, 8, 2 ** 64 - 4, 0)], {}),
    "region starts beyond the images": ([(0, 10, IMAGES + 1, 0, 0, 0, 0)], {}),
    "region ends beyond the images": ([(0, 10, 0, 100, 0, 0, 0), (0, 10, IMAGES - 99, 100, 0, 0, 0)], {}),
    "image_off + image_cap wraps": ([(0, 10, 16, 2 ** 64 - 8, 0, 0, 0)], {}),
    "regions overlap by one byte": ([(0, 10, 100, 50, 0, 0, 0), (0, 10, 0, 101, 0, 0, 0)], {}),
    "one region inside another": ([(0, 10, 0, 1000, 0, 0, 0), (0, 10, 3000, 10, 0, 0, 0), (0, 10, 500, 1, 0, 0, 0)], {}),
    "the same region twice": ([(0, 10, 64, 64, 0, 0, 0)] * 2, {}),
}


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
@pytest.mark.parametrize("name", list(MANY_EINVAL))
def test_argument_errors_are_einval_before_any_device(name, magic):
    p = helpers.pkg()
    rows, kw = MANY_EINVAL[name]
    assert _call(p, rows, **dict(dict(magic=magic), **kw)) == EINVAL, name
    assert p.lib().fourmc_gpu_last_error()


def test_no_items_is_ok_whatever_else_is_missing():
    p = helpers.pkg()
    for magic in (MC, MZ):
        for level in (0, 1, 4, 9):
            assert _call(p, GOOD, magic=magic, level=level, n=0) == OK
            assert _call(p, GOOD, magic=magic, level=level, n=0, items=False, src=False, tab=False, images=False) == OK


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_well_formed_calls_fail_with_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    for magic in (MC, MZ):
        for level in (1, 2, 3, 4):
            for images in (True, False):
                assert _call(p, GOOD, magic=magic, level=level, images=images) == ENODEV
                assert p.lib().fourmc_gpu_last_error()
    # regions that touch or are empty do not overlap; the regions of a size query are nobody's business; no table is needed without entries
    assert _call(p, [(0, 10, 0, 100, 0, 0, 0), (0, 10, 100, 100, 0, 0, 0), (0, 10, 50, 0, 0, 0, 0), (0, 0, IMAGES, 0, TAB, 0, 0)], tab=False) == ENODEV
    assert _call(p, [(0, 10, 0, 100, 0, 0, 0)] * 2 + [(0, 10, IMAGES + 5, 7, 0, 0, 0)], images=False) == ENODEV
    assert _call(p, [(0, 0, 0, 44, 0, 0, 0)], src=False, tab=False) == ENODEV
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_images_writes(torch.zeros(64, dtype=torch.uint8), [(0, 64, 0, 200, 0, 0, 0)], torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_images_writes(None, [], None, d_writes=torch.zeros(4, dtype=torch.int32))
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what=None):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_writes_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    src, img, tab = torch.zeros(SRC, dtype=torch.uint8), torch.zeros(IMAGES, dtype=torch.uint8), torch.full((TAB,), 500, dtype=torch.int32)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress_writes failed \(-1\)"):
        p.compress_images_writes(src, GOOD, img, p.MAGIC_4MZ, 4, d_writes=tab)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress_writes failed \(-1\)"):
        p.compress_images_writes(src, GOOD, None, d_writes=tab)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress_writes failed \(-3\)"):
        p.compress_images_writes(src, [(0, 10, 64, 64, 0, 0, 0)] * 2, img)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress_writes failed \(-3\)"):
        p.compress_images_writes(src, GOOD, img, 0x1234, d_writes=tab)
    with pytest.raises(p.EngineError, match="beyond the tensor"):
        p.compress_images_writes(src, GOOD, img, images_bytes=IMAGES + 1)
    assert p.compress_images_writes(src, [], img) == [] and p.compress_images_writes(None, [], None) == []
