"""GPU: the streamed .zst encoder (fourmc_gpu_zst_compress / fourmc_gpu_zsts_compress) on the catalogue of
tests/zst_write_shapes.py.  All inputs of a level go through ONE compress_zsts call.  Every image is compared byte for byte with
the image of the oracle's port of the streaming compressor (orc_zstd_stream_compress_ex, which the CPU suite holds to the
reference's bytes), and with zst_model.zstcodec's where oracle/_ref is built."""
import functools
import time

import numpy as np
import pytest
import torch

import helpers
import zst_model as zm
import zst_write_shapes as ws

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
OK = 0


def _layout(rows, lead=0):
    """rows: [(source, level, image_cap)] -> (source buffer, items, image buffer length): sources one behind the other (`lead` bytes
    in front of the first), each image region with GUARD bytes in front"""
    so, io, items, parts = lead, GUARD, [], [np.full(lead, 0x77, np.uint8)]
    for src, level, cap in rows:
        items.append((so, len(src), io, cap, level))
        pad = 64 + (-len(src)) % 64
        parts += [src, np.zeros(pad, np.uint8)]
        so += len(src) + pad; io += cap + GUARD
    return np.concatenate(parts), items, io


def _call(gpu, names, exact=False, lead=0):
    """one compress_zsts over the named inputs -> (statuses, device image buffer, host copy, items, seconds)"""
    rows = []
    for n in names:
        src, lv = ws.source(n)
        rows.append((src, lv, gpu.zst_bound(len(src)) + (0 if exact else 64)))
    buf, items, total = _layout(rows, lead)
    d_src = torch.from_numpy(buf).cuda()
    d_img = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t = time.perf_counter()
    st = gpu.compress_zsts(d_src, items, d_img)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return st, d_img, d_img.cpu().numpy(), items, dt


def _check(gpu, names, st, img, items):
    """status, bytes (the port's, and the reference's where it is built), fill bytes in front of and behind every image"""
    at, bad = 0, []
    for n, s, (_, nbytes, io, cap, _) in zip(names, st, items):
        assert (s["reason"], s["codec_result"]) == (OK, 0), (n, s)
        got = img[io:io + s["image_bytes"]].tobytes()
        if got != ws.port(n): bad.append(n)
        elif helpers.ref() is not None and got != ws.reference(n): bad.append(n + " (reference)")
        assert s["blocks"] == nbytes // ws.B + 1, (n, s)
        assert (img[at:io] == FILL).all(), (n, "in front")
        assert (img[io + s["image_bytes"]:io + cap] == FILL).all(), (n, "behind the image")
        at = io + cap
    assert (img[at:] == FILL).all()
    assert bad == []


def _level_names(level):
    return [n for n in ws.names() if n.endswith(f":l{level}")]


@functools.lru_cache(None)
def _level(level):
    return _call(helpers.pkg(), _level_names(level))


@pytest.mark.parametrize("level", ws.LEVELS)
def test_every_image_of_a_level_equals_the_port(gpu, level):
    st, _, img, items, dt = _level(level)
    print(f"level {level}: {len(items)} streams, {sum(i[1] for i in items) / 2 ** 20:.1f} MiB, compress_zsts {dt * 1e3:.0f} ms")
    _check(gpu, _level_names(level), st, img, items)


@pytest.mark.parametrize("level", ws.LEVELS)
def test_every_image_of_a_level_decodes_to_its_source_on_the_device(gpu, level):
    st, d_img, _, items, _ = _level(level)
    names = _level_names(level)
    rows, at = [], 0
    for s, (_, n, io, _, _) in zip(st, items):
        rows.append((io, s["image_bytes"], at, n)); at += n + 64
    d_out = torch.zeros(at + 64, dtype=torch.uint8, device="cuda")
    back = gpu.decompress_zsts(d_img, rows, d_out)
    out = d_out.cpu().numpy()
    for b, (_, _, do, n), name in zip(back, rows, names):
        assert (b["reason"], b["decoded_bytes"], b["frames"]) == (0, n, 1), (name, b)
        assert np.array_equal(out[do:do + n], ws.source(name)[0]), name


# every input with a short last block, and one per search arm
EXACT = ("G:R+1", "G:R+6", "G:R+7", "G:R+8", "G:R+9", "G:R+4096", "G:R+B-1", "G:R+B+1", "W:cycle", "W:handover-short", "W:rle", "C:dict-1:exact", "C:dict:exact", "C:dict+1:exact", "Y2:dev_max+1",
         "K:rep1=max:idle", "K:rep2=max:idle", "Y:dev_max+1", "A:first:ext", "A:second:pfx", "A:rep:ext", "A:run", "A:short:ext", "A:upgrade:pfx", "P:loop2")


def test_a_region_of_exactly_the_bound_is_room_enough(gpu):
    names = [f"{b}:l{lv}" for lv in ws.LEVELS for b in EXACT if f"{b}:l{lv}" in ws.names()]
    st, _, img, items, dt = _call(gpu, names, exact=True)
    print(f"exact capacity: {len(items)} streams, compress_zsts {dt * 1e3:.0f} ms")
    _check(gpu, names, st, img, items)


def test_a_source_at_an_odd_offset_gives_the_same_bytes(gpu):
    names = ["P:search:-3:l1", "U:65:mismatch:l3"]                   # one per parser family
    st, _, img, items, _ = _call(gpu, names, lead=3)
    assert items[0][0] == 3 and items[1][0] % 2 == 1
    _check(gpu, names, st, img, items)


@pytest.mark.parametrize("name", ("F:wrap:l1", "C:dict-1:l2", "A:upgrade:ext:l4"))
def test_the_single_stream_call_equals_the_port(gpu, name):
    src, level = ws.source(name)
    cap = gpu.zst_bound(len(src)) + 64
    d_src = torch.from_numpy(np.concatenate([src, np.zeros(64, np.uint8)])).cuda()
    d_img = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    one = gpu.compress_zst(d_src, d_img, level=level, src_bytes=len(src))
    got = d_img.cpu().numpy()
    assert one["reason"] == OK and got[:one["image_bytes"]].tobytes() == ws.port(name)
    assert (got[one["image_bytes"]:] == FILL).all()


def test_mixed_levels_in_one_call(gpu):
    names = [f"{b}:l{lv}" for b in ("W:rawmid", "P:behind:+0", "L:all") for lv in ws.LEVELS]
    st, _, img, items, dt = _call(gpu, names)
    print(f"mixed levels: {len(items)} streams, compress_zsts {dt * 1e3:.0f} ms")
    _check(gpu, names, st, img, items)
