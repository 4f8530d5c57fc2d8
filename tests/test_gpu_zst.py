"""GPU: .zst streams decoded in device memory (fourmc_gpu_zst_decompress / fourmc_gpu_zsts_decompress) on the inputs of
tests/zst_model.py.  The committed files (tests/golden/zst_*.zst) always run; the inputs A-F and the damaged inputs G are built
with the reference's library and need oracle/_ref, as do the reference's verdicts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers
import zst_model as zm

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not present")
GUARD, FILL = 64, 0xA5
ROUNDS = (0, 64, 100)                      # table entries per round: the default, one wave's worth, and a count that cuts a wave in two


class _Round:
    def __init__(self, gpu, blocks): self.lib, self.blocks = gpu.lib(), blocks

    def __enter__(self): self.lib.fourmc_gpu_set_zst_round_blocks(self.blocks)

    def __exit__(self, *a): self.lib.fourmc_gpu_set_zst_round_blocks(0)


def _status(gpu, st):
    return {name: int(getattr(st, name)) for name, _ in gpu.ZstStatus._fields_ if name != "pad"}


def _upload(images):
    """The images one behind the other, 64 bytes of slack behind each -> (tensor, [(offset, bytes)])."""
    at, rows, parts = 0, [], []
    for img in images:
        rows.append((at, len(img)))
        parts += [np.frombuffer(img, np.uint8), np.zeros(64 + (-len(img)) % 64, np.uint8)]
        at += len(img) + 64 + (-len(img)) % 64
    return torch.from_numpy(np.concatenate(parts)).cuda(), rows


def _call(gpu, d_images, rows, caps):
    """One call over `rows` of d_images; caps None: the size query.  -> (statuses, raw destination, [region offset])."""
    arr = (gpu.ZstItem * len(rows))()
    at, offs = GUARD, []
    for i, (io, ib) in enumerate(rows):
        arr[i].image_off, arr[i].image_bytes = io, ib
        if caps is not None:
            arr[i].dst_off, arr[i].dst_cap = at, caps[i]
            offs.append(at)
            at += caps[i] + GUARD
    raw = torch.full((at if caps is not None else 1,), FILL, dtype=torch.uint8, device="cuda")
    L = gpu.lib()
    rc = L.fourmc_gpu_zsts_decompress(d_images.data_ptr(), d_images.numel(), raw.data_ptr() if caps is not None else None, raw.numel(),
                                      C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == 0, (rc, L.fourmc_gpu_last_error())
    return [_status(gpu, arr[i].status) for i in range(len(rows))], raw.cpu().numpy(), offs


def _single(gpu, img, cap):
    """fourmc_gpu_zst_decompress of one image; cap None: the size query.  -> (status, region bytes, guards intact)."""
    d_img, rows = _upload([img])
    st = gpu.ZstStatus()
    raw = torch.full((2 * GUARD + (cap or 0),), FILL, dtype=torch.uint8, device="cuda")
    L = gpu.lib()
    rc = L.fourmc_gpu_zst_decompress(d_img.data_ptr(), len(img), raw.data_ptr() + GUARD if cap is not None else None, cap or 0, C.byref(st), None)
    assert rc == 0, (rc, L.fourmc_gpu_last_error())
    out = raw.cpu().numpy()
    intact = bool((out[:GUARD] == FILL).all() and (out[GUARD + (cap or 0):] == FILL).all())
    return _status(gpu, st), out[GUARD:GUARD + (cap or 0)], intact


def _check_valid(gpu, name, img, src):
    """Size query, decode at the exact capacity, one byte short: the model's counts, the source's bytes, no serial frame."""
    w = zm.walk(img)
    q, _, _ = _single(gpu, img, None)
    want = {"decoded_bytes": 0, "total_bytes": len(src), "fail_offset": len(img), "frames": w["frames"], "skippable": w["skippable"],
            "blocks": w["blocks"], "reason": 0, "codec_result": 0}
    assert q == want, (name, q)
    gpu.zst_stats()                                                      # (reset)
    st, out, intact = _single(gpu, img, len(src))
    stats = gpu.zst_stats()
    assert st == dict(want, decoded_bytes=len(src)), (name, st)
    assert intact and out.tobytes() == src, name
    assert stats == {"fast_frames": w["frames"], "serial_frames": 0, "fast_blocks": w["blocks"]}, (name, stats)
    if len(src):
        st, out, intact = _single(gpu, img, len(src) - 1)
        assert st["reason"] == 2 and gpu.ZST_REASONS[2] == "DST_SMALL" and st["total_bytes"] == len(src) and st["decoded_bytes"] == 0, (name, st)
        assert intact and (out == FILL).all(), name


@pytest.mark.parametrize("blocks", ROUNDS)
def test_committed_files_decode(gpu, blocks):
    """Input B with a skippable frame, a checksum frame and the empty frame behind it, and input C streamed: treeless blocks and
    Repeat-mode tables whose defining block lies in an earlier wave and an earlier round."""
    with _Round(gpu, blocks):
        for name, (img, src) in zm.fixture().items(): _check_valid(gpu, name, img, src)


def test_committed_files_as_many_streams_and_damaged(gpu):
    """Without the reference: the files as items of one call, one of them twice, a damaged copy between them - a flipped checksum,
    which fails the second frame and nothing else."""
    F = zm.fixture()
    small, small_src = F["zst_small.zst"]
    blocks_, blocks_src = F["zst_blocks.zst"]
    spans = zm.walk(small)["spans"]
    bad = small[:spans[1][1] - 1] + bytes([small[spans[1][1] - 1] ^ 1]) + small[spans[1][1]:]
    d_images, rows = _upload([small, bad, blocks_])
    rows = [rows[0], rows[1], rows[2], rows[0]]
    caps = [len(small_src), len(small_src), len(blocks_src), len(small_src)]
    sts, raw, offs = _call(gpu, d_images, rows, caps)
    for i, (src, ok) in enumerate(((small_src, True), (small_src, False), (blocks_src, True), (small_src, True))):
        region = raw[offs[i]:offs[i] + caps[i]]
        assert (raw[offs[i] - GUARD:offs[i]] == FILL).all() and (raw[offs[i] + caps[i]:offs[i] + caps[i] + GUARD] == FILL).all(), i
        if ok: assert sts[i]["reason"] == 0 and sts[i]["decoded_bytes"] == len(src) and region.tobytes() == src, (i, sts[i])
    st = sts[1]
    assert (st["reason"], st["fail_offset"], st["decoded_bytes"], st["frames"], st["skippable"], st["blocks"]) == \
        (1, spans[1][0], 260000, 1, 1, 200) and st["codec_result"] < 0, st
    assert raw[offs[1]:offs[1] + 260000].tobytes() == small_src[:260000]
    single, _, _ = _single(gpu, bad, len(small_src))
    assert single == st


# ---------------------------------------------------------------------------------------------- with the reference
@needs_ref
@pytest.mark.parametrize("blocks", ROUNDS)
def test_valid_inputs(gpu, blocks):
    """A-F: the source's bytes at the exact capacity, DST_SMALL with an untouched destination one byte below it, the model's
    counts from the size query, every block through the lane-per-block stages.  B and C cross rounds inside a frame at 64 and 100."""
    with _Round(gpu, blocks):
        for name, (img, src) in zm.inputs().items(): _check_valid(gpu, name, img, src)


@functools.lru_cache(None)
def _g_expect():
    I = zm.inputs()
    return [(cls, label, img, len(I[base][1]), zm.ref_decode(img, len(I[base][1])), zm.expect(img, len(I[base][1])))
            for cls, label, img, base in zm.damaged()]


def _check_damaged(label, st, region, ref, e):
    r, ref_out = ref
    assert (st["reason"] == 0) == (r >= 0), (label, st, r)
    if r >= 0:
        assert st["decoded_bytes"] == r == st["total_bytes"] and region[:r].tobytes() == ref_out, (label, st)
        assert st["codec_result"] == 0 and st["fail_offset"] == e["fail_offset"], (label, st)
    else:
        assert st["reason"] == 1 and st["codec_result"] < 0, (label, st)
        assert st["fail_offset"] == e["fail_offset"] and st["decoded_bytes"] == e["decoded"], (label, st, e["fail_offset"], e["decoded"])
        assert region[:e["decoded"]].tobytes() == e["data"], label
        assert st["total_bytes"] >= st["decoded_bytes"], (label, st)
    assert (st["frames"], st["skippable"], st["blocks"]) == (e["frames"], e["skippable"], e["blocks"]), (label, st, e["frames"], e["skippable"], e["blocks"])


@needs_ref
def test_damaged_inputs(gpu):
    """G: OK exactly when the reference's ZSTD_decompress of the whole file succeeds, then with its bytes; else FRAME with a
    negative codec result at the failing frame, and the frames in front of it decoded."""
    for cls, label, img, cap, ref, e in _g_expect():
        st, region, intact = _single(gpu, img, cap)
        assert intact, label
        _check_damaged(label, st, region, ref, e)
        q, _, _ = _single(gpu, img, None)
        assert q["total_bytes"] <= st["total_bytes"] and q["decoded_bytes"] == 0, (label, q, st)


@needs_ref
def test_many_streams_equal_their_single_calls(gpu):
    """Every input of A-G as items of one call, the first two images named twice: each item's status and bytes are its single
    call's, and the regions next to damaged items are whole."""
    I = zm.inputs()
    items = [(name, img, len(src)) for name, (img, src) in I.items()]
    g = _g_expect()
    mixed = []                                                           # a damaged item after every valid one while they last
    for k, it in enumerate(items):
        mixed.append(it)
        if k < len(g): mixed.append((g[k][1], g[k][2], g[k][3]))
    mixed += [(x[1], x[2], x[3]) for x in g[len(items):]]
    d_images, rows = _upload([img for _, img, _ in mixed])
    names = [n for n, _, _ in mixed] + [mixed[0][0], mixed[2][0]]
    rows = rows + [rows[0], rows[2]]
    caps = [c for _, _, c in mixed] + [mixed[0][2], mixed[2][2]]
    images = [img for _, img, _ in mixed] + [mixed[0][1], mixed[2][1]]
    sts, raw, offs = _call(gpu, d_images, rows, caps)
    gd = {x[1]: x for x in g}
    for i, name in enumerate(names):
        assert (raw[offs[i] - GUARD:offs[i]] == FILL).all() and (raw[offs[i] + caps[i]:offs[i] + caps[i] + GUARD] == FILL).all(), name
        region = raw[offs[i]:offs[i] + caps[i]]
        single, out, _ = _single(gpu, images[i], caps[i])
        assert sts[i] == single, (name, sts[i], single)
        n = single["decoded_bytes"]
        assert region[:n].tobytes() == out[:n].tobytes(), name
        if name in gd: _check_damaged(name, sts[i], region, gd[name][4], gd[name][5])
        else: assert sts[i]["reason"] == 0 and region.tobytes() == I[name][1], name
    q, _, _ = _call(gpu, d_images, rows, None)
    for i, name in enumerate(names):
        assert q[i]["decoded_bytes"] == 0 and q[i]["total_bytes"] <= sts[i]["total_bytes"], name
        if name not in gd: assert q[i] == dict(sts[i], decoded_bytes=0), name
