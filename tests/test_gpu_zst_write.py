"""GPU: .zst streams written in device memory (fourmc_gpu_zst_compress / fourmc_gpu_zsts_compress) on the inputs of
tests/zst_write_model.py.  Every image is compared with the reference's bytes: with zst_model.zstcodec where oracle/_ref is built,
with the SHA-256 of the committed fixture (tests/golden/zst_write.json) otherwise."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import helpers
import zst_model as zm
import zst_write_model as wm

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
OK, DST_SMALL, LEVEL, TOO_LONG = 0, 1, 2, 3


def _same_as_reference(name, got):
    """got: bytes of the device's image of input `name`"""
    if helpers.ref() is not None: return got == wm.reference()[name]
    e = wm.fixture()[name]
    return len(got) == e["bytes"] and hashlib.sha256(got).hexdigest() == e["sha256"] and ("hex" not in e or got.hex() == e["hex"])


def _layout(rows, slack=64):
    """rows: [(source, level, image_cap)] -> (source buffer, items, image buffer length): the sources one behind the other, each
    region with GUARD bytes in front"""
    so, io, items, parts = 0, GUARD, [], []
    for src, level, cap in rows:
        items.append((so, len(src), io, cap, level))
        pad = slack + (-len(src)) % 64
        parts += [src, np.zeros(pad, np.uint8)]
        so += len(src) + pad; io += cap + GUARD
    return np.concatenate(parts), items, io


def _run(gpu, rows):
    buf, items, total = _layout(rows)
    d_src = torch.from_numpy(buf).cuda()
    d_img = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    st = gpu.compress_zsts(d_src, items, d_img)
    return st, d_img, items


@functools.lru_cache(None)
def _batch():
    """All inputs through ONE call, capacity bound + 64 -> (statuses, images on the device, images on the host, items, names)."""
    gpu = helpers.pkg()
    names = list(wm.REQUIRED)
    rows = [(wm.inputs()[n][0], wm.inputs()[n][1], gpu.zst_bound(len(wm.inputs()[n][0])) + 64) for n in names]
    st, d_img, items = _run(gpu, rows)
    return st, d_img, d_img.cpu().numpy(), items, names


def test_every_image_equals_the_reference(gpu):
    st, _, img, items, names = _batch()
    for s, (_, n, io, cap, _), name in zip(st, items, names):
        assert (s["reason"], s["codec_result"], s["name"], s["message"]) == (OK, 0, "OK", ""), (name, s)
        assert s["image_bytes"] <= gpu.zst_bound(n) and s["blocks"] == n // wm.B + 1, (name, s)
        assert _same_as_reference(name, img[io:io + s["image_bytes"]].tobytes()), name


def test_nothing_is_written_outside_the_image(gpu):
    st, _, img, items, names = _batch()
    at = 0
    for s, (_, _, io, cap, _), name in zip(st, items, names):
        assert (img[at:io] == FILL).all(), (name, "in front")
        assert (img[io + s["image_bytes"]:io + cap] == FILL).all(), (name, "behind the image")
        at = io + cap
    assert (img[at:] == FILL).all()


def test_every_image_decodes_to_its_source_on_the_device(gpu):
    st, d_img, _, items, names = _batch()
    rows, at = [], 0
    for s, (_, n, io, _, _) in zip(st, items):
        rows.append((io, s["image_bytes"], at, n)); at += n + 64
    d_out = torch.zeros(at + 64, dtype=torch.uint8, device="cuda")
    back = gpu.decompress_zsts(d_img, rows, d_out)
    out = d_out.cpu().numpy()
    for b, (_, _, do, n), name in zip(back, rows, names):
        assert (b["reason"], b["decoded_bytes"], b["frames"]) == (0, n, 1), (name, b)
        assert np.array_equal(out[do:do + n], wm.inputs()[name][0]), name


@pytest.mark.parametrize("name", ("G:l1:R+1", "P:l3:b", "G:l1:0"))
def test_single_call_equals_the_batch(gpu, name):
    st, _, img, items, names = _batch()
    k = names.index(name)
    src, level = wm.inputs()[name]
    cap = gpu.zst_bound(len(src)) + 64
    d_src = torch.from_numpy(np.concatenate([src, np.zeros(64, np.uint8)])).cuda()
    d_img = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    one = gpu.compress_zst(d_src, d_img, level=level, src_bytes=len(src))
    assert one == st[k]
    got = d_img.cpu().numpy()
    io = items[k][2]
    assert np.array_equal(got[:one["image_bytes"]], img[io:io + one["image_bytes"]]) and (got[one["image_bytes"]:] == FILL).all()


def test_mixed_levels_and_refused_items_in_one_call(gpu):
    I = wm.inputs()
    names = ["G:l1:R+1", "G:l2:R+B+1", "G:l3:R+1", "G:l4:R+B+1"]
    rows = [(I[n][0], I[n][1], gpu.zst_bound(len(I[n][0]))) for n in names]
    rows.insert(1, (I["G:l1:131073"][0], 5, 200000))
    buf, items, total = _layout(rows)
    items.append((0, 0xC0000001, total, 4096, 1))                    # only a descriptor: no such source exists
    d_src = torch.from_numpy(buf).cuda()
    d_img = torch.full((total + 4096 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    st = gpu.compress_zsts(d_src, items, d_img)
    img = d_img.cpu().numpy()
    assert (st[1]["reason"], st[1]["name"], st[1]["image_bytes"]) == (LEVEL, "LEVEL", 0)
    assert (st[-1]["reason"], st[-1]["name"], st[-1]["image_bytes"]) == (TOO_LONG, "TOO_LONG", 0)
    for k in (1, len(items) - 1):
        io, cap = items[k][2], items[k][3]
        assert (img[io - GUARD:io + cap + GUARD] == FILL).all()
    for name, k in zip(names, (0, 2, 3, 4)):
        io = items[k][2]
        assert st[k]["reason"] == OK and _same_as_reference(name, img[io:io + st[k]["image_bytes"]].tobytes()), name


def test_an_image_that_does_not_fit_costs_only_itself(gpu):
    bg = wm.background()
    bound = gpu.zst_bound(len(bg))
    name = "G:l1:R+1"
    src, level = wm.inputs()[name]
    st, d_img, items = _run(gpu, [(bg, 1, bound), (bg, 1, bound - 1000), (src, level, gpu.zst_bound(len(src))), (bg, 3, bound - 1000)])
    img = d_img.cpu().numpy()
    assert (st[0]["reason"], st[0]["image_bytes"]) == (OK, bound)     # every block raw: the bound is exact
    raw = img[items[0][2]:items[0][2] + bound]
    assert bytes(raw[:6]) == bytes.fromhex("28b52ffd0048") and np.array_equal(raw[9:9 + wm.B], bg[:wm.B])
    for k in (1, 3):
        assert (st[k]["reason"], st[k]["name"], st[k]["codec_result"], st[k]["image_bytes"]) == (DST_SMALL, "DST_SMALL", -70, 0), st[k]
    assert st[2]["reason"] == OK and _same_as_reference(name, img[items[2][2]:items[2][2] + st[2]["image_bytes"]].tobytes())
    at = 0
    for s, (_, _, io, cap, _) in zip(st, items):                     # nothing outside any region, the refused ones included
        assert (img[at:io] == FILL).all()
        at = io + cap
    assert (img[at:] == FILL).all()
    assert (img[items[0][2] + bound:items[0][2] + items[0][3]] == FILL).all()


def test_the_bound_is_room_enough_for_every_source(gpu):
    """image_cap exactly zst_bound(n): one and two bytes, incompressible sources with a last block of 1 and 2 bytes, short last
    blocks that barely compress, and the inputs whose last block is short."""
    I = wm.inputs()
    rng = wm.background()
    small = np.concatenate([np.frombuffer(b"abcabcabcabd" * 3, np.uint8), rng[:40]])
    cases = [(I["G:l1:1"][0], 1), (I["G:l3:R+1"][0][:2], 3), (rng[:wm.B + 1], 1), (rng[:wm.B + 2], 3), (rng[:7], 1),
             (np.concatenate([rng[:wm.B], small]), 1), (small, 3), (I["G:l1:131073"][0], 1), (I["G:l1:131071"][0], 1)]
    rows = [(src, level, gpu.zst_bound(len(src))) for src, level in cases]
    st, d_img, items = _run(gpu, rows)
    img = d_img.cpu().numpy()
    at = 0
    for s, (src, level), (_, n, io, cap, _) in zip(st, cases, items):
        assert s["reason"] == OK and s["image_bytes"] <= cap, (n, level, s)
        got = img[io:io + s["image_bytes"]].tobytes()
        if helpers.ref() is not None: assert got == zm.zstcodec(src, level), (n, level)
        assert (img[at:io] == FILL).all() and (img[io + s["image_bytes"]:io + cap] == FILL).all(), (n, level)
        at = io + cap
    back = gpu.decompress_zsts(d_img, [(io, s["image_bytes"], 0, 0) for s, (_, _, io, _, _) in zip(st, items)], None)
    assert [b["total_bytes"] for b in back] == [len(src) for src, _ in cases]
    assert st[0]["image_bytes"] == 10 and st[2]["image_bytes"] == gpu.zst_bound(wm.B + 1)


def test_a_source_at_an_odd_offset_gives_the_same_bytes(gpu):
    st, _, img, items, names = _batch()
    name = "G:l1:2R+1"
    k = names.index(name)
    src, level = wm.inputs()[name]
    d_src = torch.from_numpy(np.concatenate([np.full(3, 0x77, np.uint8), src, np.zeros(64, np.uint8)])).cuda()
    cap = gpu.zst_bound(len(src))
    d_img = torch.full((cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    got_st = gpu.compress_zsts(d_src, [(3, len(src), GUARD, cap, level)], d_img)[0]
    assert got_st == st[k]
    got = d_img.cpu().numpy()
    io = items[k][2]
    assert np.array_equal(got[GUARD:GUARD + got_st["image_bytes"]], img[io:io + got_st["image_bytes"]])
    one = gpu.compress_zst(d_src[3:3 + len(src) + 32], d_img[GUARD:GUARD + cap], level=level, src_bytes=len(src))   # the same through a view
    assert one == st[k] and np.array_equal(d_img.cpu().numpy()[GUARD:GUARD + one["image_bytes"]], img[io:io + one["image_bytes"]])
