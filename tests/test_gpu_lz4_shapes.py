"""GPU: LZ4 block decode on every shape of tests/lz4_shapes.py, per decode path.

Every launch is one DeviceBatch of all shapes; each destination slot lies between 64 guard bytes of 0xA5.  In the per-path
launches every slot begins at an address that is 0 mod 65536, the ring phase the catalogue's ledger is computed for.  The expected
result of every block is the oracle's (tests/test_lz4_shapes_cpu.py holds the oracle to the reference's LZ4_decompress_safe on
exactly these streams and capacities); what a fast path may hand back is computed from the documented eligibility rule
(lz4_shapes.eligible), never from the kernel's answer."""
import functools

import numpy as np
import pytest
import torch

import helpers
import lz4_shapes as ls

pytestmark = pytest.mark.gpu
GUARD, G = 0xA5, 64
CORRUPT = -1000000002                       # FOURMC_BLK_CORRUPT (include/fourmc_gpu.h)
PATHS = {"exact": 2, "seg": 11, "tile": 13, "auto": 6}
ALONE = {"segonly": 12, "tileonly": 14}
MAGIC = 0x344D4300

# valid eligible shapes a fast path hands back by a rule its source states: {path: {frame name: "file:line rule"}}.  Empty: the
# tile path clips a sequence of any length to its tiles, and the segment path's escape decode declines only lengths above 1 << 23
# (lz4_seg.hip:445, 448), which no block of at most 4 MiB has.
HANDED_BACK = {"segonly": {}, "tileonly": {}}


@functools.lru_cache(None)
def _cases():
    """[(label, stream, cap, valid, (oracle result, oracle bytes))]"""
    return tuple((lab, st, cap, dec is not None, helpers.orc_decompress(st, cap)) for lab, st, cap, dec in ls.cases())


def _launch(gpu, items, path, container=False, src_res=None, dst_res=None, abut=False):
    """items [(stream, cap)] in one launch -> (results, output buffer, destination offsets).  src_res / dst_res: every source /
    destination ADDRESS is that residue mod 16; default: sources back to back from an odd offset, destinations at 0 mod 65536."""
    off, pos = [], 3
    for st, _ in items:
        if src_res is not None: pos += (src_res - pos) % 16
        off.append(pos); pos += len(st)
    buf = np.zeros(pos + 64, np.uint8)
    for (st, _), o in zip(items, off): buf[o:o + len(st)] = st
    d_src = torch.from_numpy(buf).cuda()
    assert d_src.data_ptr() % 16 == 0
    dst, dpos = [], 0
    for _, cap in items:
        dpos += G
        if abut: pass
        elif dst_res is not None: dpos += (dst_res - dpos) % 16
        else: dpos += -dpos % 65536
        dst.append(dpos); dpos += cap
    d_dst = torch.full((dpos + G + 65536,), GUARD, dtype=torch.uint8, device="cuda")
    shift = -d_dst.data_ptr() % 65536
    dst = [d + shift for d in dst]
    sums = [helpers.orc_xxh32(st) for st, _ in items] if container else None
    batch = gpu.DeviceBatch(gpu.make_blocks(off, dst, [len(st) for st, _ in items], [c for _, c in items], sums))
    L = gpu.lib()
    L.fourmc_gpu_set_lz4_decode_path(path)
    try:
        if container: gpu.decode_blocks(d_src, d_dst, batch)
        else: gpu.lz4_decompress(d_src, d_dst, batch)
        torch.cuda.synchronize()
    finally:
        L.fourmc_gpu_set_lz4_decode_path(6)
    return [int(r) for r in batch.download()["result"]], d_dst.cpu().numpy(), dst


def _guards(out, d, cap):
    return bool((out[d - G:d] == GUARD).all() and (out[d + cap:d + cap + G] == GUARD).all())


def _want(st, cap, orc, container):
    """what a block has to come back with: (result, bytes)"""
    wr, wb = orc
    if container and len(st) == cap: return cap, st              # a stored block (native/4mc.c:635-642)
    if container and wr < 0: return CORRUPT, None
    return wr, wb


@pytest.mark.parametrize("container", [False, True], ids=["raw", "container"])
@pytest.mark.parametrize("path", list(PATHS))
def test_every_path_agrees_with_the_oracle(gpu, path, container):
    cases = _cases()
    res, out, dst = _launch(gpu, [(st, cap) for _, st, cap, _, _ in cases], PATHS[path], container)
    bad = []
    for (lab, st, cap, valid, orc), r, d in zip(cases, res, dst):
        wr, wb = _want(st, cap, orc, container)
        if valid and not (container and len(st) == cap): assert wr == len(wb) and wr <= cap, lab
        if r != wr: bad.append((lab, "result", r, wr))
        elif wr > 0 and not np.array_equal(out[d:d + wr], wb): bad.append((lab, "bytes", int(np.flatnonzero(out[d:d + wr] != wb)[0])))
        if not _guards(out, d, cap): bad.append((lab, "guard"))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("container", [False, True], ids=["raw", "container"])
@pytest.mark.parametrize("path", list(ALONE))
def test_the_fast_paths_do_the_work(gpu, path, container):
    """Without the exact walker's redo behind them (decode paths 12 / 14) a block keeps kRetryCode only if it is ineligible by size
    or listed in HANDED_BACK; every other valid block comes back with the oracle's size and bytes, a damaged one with the oracle's
    verdict or handed back, never with another verdict.  The keys of the catalogue's ledger, but for those only ineligible blocks
    reach, are all reached by blocks the path finished; test_the_fast_paths_stop_where_the_margins_begin shows how far into such a
    block the path itself went."""
    cases = _cases()
    res, out, dst = _launch(gpu, [(st, cap) for _, st, cap, _, _ in cases], ALONE[path], container)
    bad, finished, table = [], set(), HANDED_BACK[path]
    for (lab, st, cap, valid, orc), r, d in zip(cases, res, dst):
        wr, wb = _want(st, cap, orc, container)
        stored = container and len(st) == cap
        if not _guards(out, d, cap): bad.append((lab, "guard"))
        if r == ls.RETRY:
            if stored or (valid and ls.eligible(len(st), cap) and lab.split("/")[0] not in table): bad.append((lab, "handed back"))
            continue
        if not stored and not ls.eligible(len(st), cap): bad.append((lab, "ineligible, yet", r)); continue
        if r != wr: bad.append((lab, "result", r, wr))
        elif wr > 0 and not np.array_equal(out[d:d + wr], wb): bad.append((lab, "bytes", int(np.flatnonzero(out[d:d + wr] != wb)[0])))
        elif valid and not stored: finished.add((lab, cap))
    assert not bad, (len(bad), bad[:12])
    reached = set()
    for lab, st, cap, valid, _ in cases:
        if (lab, cap) in finished: reached |= ls.inspect(st, cap)
    missing = sorted(ls.REQUIRED - ls.ELIGIBILITY - reached)
    assert not missing, missing


TILE_SLOT = 4 * ((48 + (ls.K_MAXSRC + 31) // 32 + 512 + 32 + 3) & ~3)                 # lz4tile.h:36-44 kWsWords, in bytes
SEG_SLOT = 4 * ((320 + 2 * (64 * (128 + 8) + ls.K_MAXSRC // 3 + 512) + 3) & ~3)       # lz4seg.h:35-39 kWsWords, in bytes
RES_AT = {"tileonly": (TILE_SLOT, 4 * 2), "segonly": (SEG_SLOT, 4 * 3)}               # kMetaResIp (the output position follows it)


@pytest.mark.parametrize("path", list(ALONE))
def test_the_fast_paths_stop_where_the_margins_begin(gpu, path):
    """What a fast path leaves for the exact walker is read from the block's workspace slot (kMetaResIp, kMetaResOp; the research
    side build exports the read): for every valid eligible block it is exactly the first sequence whose output ends beyond
    cap - kOMargin, or the first token within the last kMargin stream bytes (lz4_shapes.fast_stop) - the path executed every
    sequence in front of that itself, and none behind it."""
    cases = [c for c in _cases() if c[3] and ls.eligible(len(c[1]), c[2])]
    assert len(cases) > 200
    slot, at = RES_AT[path]
    gpu.use_research(True)
    try:
        gpu.gpu_init()
        res, out, dst = _launch(gpu, [(st, cap) for _, st, cap, _, _ in cases], ALONE[path])
        got = np.zeros((len(cases), 2), np.uint32)
        for b in range(len(cases)):
            assert gpu.lib().fourmc_gpu_debug_read_workspace(got[b].ctypes.data, b * slot + at, 8) == 0, b
    finally:
        gpu.use_research(False)
    bad = []
    for (lab, st, cap, _, (wr, wb)), r, d, (rip, rop) in zip(cases, res, dst, got.tolist()):
        if r != wr or not np.array_equal(out[d:d + wr], wb): bad.append((lab, "result", r, wr))
        want = ls.fast_stop(ls.walk(st), cap)
        if (rip, rop) != want: bad.append((lab, "stopped at", (rip, rop), "model", want))
    assert not bad, (len(bad), bad[:12])
    assert sum(ls.fast_stop(ls.walk(st), cap)[1] > 0 for _, st, cap, _, _ in cases) > 150


def test_every_alignment_of_source_and_destination(gpu):
    """The valid set (without the two 4 MiB extremes) with every block's source address r mod 16 and its destination address
    (5 r + 3) mod 16, r = 0 .. 15, and once with the slots abutting (only the guards between); every launch on both fast paths."""
    items = [(f.name, f.stream, cap, f.decoded) for f in ls.frames() if len(f.decoded) < 4 * ls.MIB for cap in (f.caps[0], f.caps[-1])]
    assert len(items) > 90
    runs = [(r, (5 * r + 3) % 16, False) for r in range(16)] + [(None, None, True)]
    for r, r2, abut, path in [(*run, path) for run in runs for path in ("tile", "seg")]:
        res, out, dst = _launch(gpu, [(st, cap) for _, st, cap, _ in items], PATHS[path], False, r, r2, abut)
        for (name, st, cap, dec), got, d in zip(items, res, dst):
            if r is not None: assert d % 16 == r2
            assert got == len(dec), (name, cap, path, r, r2, abut, got)
            assert np.array_equal(out[d:d + got], dec), (name, cap, path, r, r2, abut)
            assert _guards(out, d, cap), (name, cap, path, r, r2, abut)


def _be(v):
    return int(v).to_bytes(4, "big")


def _image(frs):
    """a .4mc file image of the frames' outputs, one block each: the hand-built payload where it is smaller than the output, the
    output stored where it is not (oracle/container_port.c:34-61: header, blocks, end mark, footer)"""
    parts, deltas, pos, prev = [], [], 12, 0
    head = _be(MAGIC) + _be(1)
    parts.append(head + _be(helpers.orc_xxh32(np.frombuffer(head, np.uint8))))
    for f in frs:
        pay = f.stream if len(f.stream) < len(f.decoded) else f.decoded
        deltas.append(pos - prev); prev = pos
        parts.append(_be(len(f.decoded)) + _be(len(pay)) + _be(helpers.orc_xxh32(pay)) + pay.tobytes())
        pos += 12 + len(pay)
    parts.append(bytes(12))
    fsz = 20 + 4 * len(frs)
    foot = _be(fsz) + _be(1) + b"".join(_be(d) for d in deltas) + _be(fsz) + _be(MAGIC)
    parts.append(foot + _be(helpers.orc_xxh32(np.frombuffer(foot, np.uint8))))
    return np.frombuffer(b"".join(parts), np.uint8).copy()


def test_through_the_image_calls(gpu):
    frs = list(ls.frames())
    img = _image(frs)
    want = np.concatenate([f.decoded for f in frs])
    n, back, used = helpers.orc_container_decode(img, len(want))
    assert n == len(want) and used == len(img) and np.array_equal(back, want)          # the oracle's reader takes the framing
    assert sum(len(f.stream) < len(f.decoded) for f in frs) > 30
    d_img = torch.from_numpy(np.concatenate([img, np.zeros(64, np.uint8)])).cuda()
    d_out = torch.full((len(want) + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    st = gpu.decompress_image(d_img, d_out[: len(want)], image_bytes=len(img))
    torch.cuda.synchronize()
    assert st["decoded_bytes"] == len(want), st
    got = d_out.cpu().numpy()
    assert np.array_equal(got[: len(want)], want) and (got[len(want):] == GUARD).all()
    edges = np.cumsum([len(f.decoded) for f in frs])
    dense = int(edges[[f.name for f in frs].index("dense4m") - 1])
    assert frs[-1].name == "lit4m" and frs[-2].name == "dense4m"
    ranges = [(int(edges[3]) - 100, int(edges[6] - edges[3]) + 200), (dense - 10, 70000), (int(edges[-2]) - 3000, 70001)]
    d_out.fill_(GUARD)
    at, q = 0, []
    for a, ln in ranges: q.append((a, ln, at)); at += ln + G
    r = gpu.image_read(d_img, q, d_out, image_bytes=len(img))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert list(r) == [ln for _, ln in ranges], r
    for a, ln, o in q:
        assert np.array_equal(got[o:o + ln], want[a:a + ln]), (a, ln)
        assert (got[o + ln:o + ln + G] == GUARD).all(), (a, ln)
