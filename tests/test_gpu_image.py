"""Whole .4mc / .4mz file images in device memory (fourmc_gpu_image_compress / _decompress): the bytes the CLI writes, and the
verdict, message and output the CLI's decoder gives for the same bytes as a file - under both parsers (FOURMC_IMAGE_PARSE)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
B = helpers.B
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus_manifest.json")))
PAD = 4096                                       # device images keep slack behind them, as the block decode's callers do


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _dev(b, pad=PAD):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    if len(a):
        t[:len(a)] = torch.from_numpy(a.copy()).cuda()
    return t


def _magic(p, z):
    return p.MAGIC_4MZ if z else p.MAGIC_4MC


def compress(p, data, z, level):
    d_src = torch.from_numpy(np.ascontiguousarray(data)).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_img = torch.empty(p.image_bound(len(data)), dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_img, _magic(p, z), level)
    return d_img[:n].cpu().numpy().tobytes()


def decode(p, image, z, cap=None, query=False, parser=None):
    """decompress_image of `image` (bytes); returns (status, output bytes up to decoded_bytes)"""
    old = os.environ.get("FOURMC_IMAGE_PARSE")
    if parser:
        os.environ["FOURMC_IMAGE_PARSE"] = parser
    try:
        d_img = _dev(image)
        if query:
            return p.decompress_image(d_img, None, _magic(p, z), image_bytes=len(image)), b""
        if cap is None:
            cap = p.decompress_image(d_img, None, _magic(p, z), image_bytes=len(image))["total_bytes"]
        d_dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        st = p.decompress_image(d_img, d_dst[:cap] if cap else d_dst[:0], _magic(p, z), image_bytes=len(image))
        return st, d_dst[:st["decoded_bytes"]].cpu().numpy().tobytes()
    finally:
        if parser:
            if old is None:
                os.environ.pop("FOURMC_IMAGE_PARSE", None)
            else:
                os.environ["FOURMC_IMAGE_PARSE"] = old


def decode_both(p, image, z):
    """both parsers; their statuses and outputs must be identical"""
    a = decode(p, image, z, parser="auto")
    b = decode(p, image, z, parser="walk")
    assert a[0] == b[0], (a[0], b[0])
    assert a[1] == b[1]
    return a


def cli_compress(exe, tmp_path, data, z, level, tag):
    src = tmp_path / f"in_{tag}"
    out = tmp_path / f"out_{tag}"
    src.write_bytes(bytes(data))
    r = subprocess.run([exe] + (["-z"] if z else []) + [f"-{level}", "-f", str(src), str(out)], capture_output=True)
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


def cli_decode(exe, tmp_path, image, z, tag):
    src = tmp_path / f"dmg_{tag}"
    out = tmp_path / f"dec_{tag}"
    src.write_bytes(bytes(image))
    r = subprocess.run([exe, "-d"] + (["-z"] if z else []) + ["-f", str(src), str(out)], capture_output=True)
    return r.returncode, r.stderr.decode(errors="replace"), out.read_bytes() if out.exists() else b""


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


@pytest.fixture(scope="module")
def golden():
    c = MANIFEST["corpus"]
    data = helpers.corpus(c["bytes"], first_block=c["first_block"], seed=c["seed"])
    assert _sha(data) == c["sha256"]
    return data


# ---- 1 + 2: encode parity and the round trip -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4mc-1", "4mc-2", "4mc-3", "4mc-4", "4mz-1", "4mz-2"])
def test_golden_image_and_round_trip(p, golden, name):
    z, level = name.startswith("4mz"), int(name[-1])
    img = compress(p, golden, z, level)
    want = MANIFEST["levels"][name]
    assert len(img) == want["file_bytes"] and _sha(img) == want["sha256"], name
    q, _ = decode(p, img, z, query=True)
    assert q["exit_code"] == 0 and q["total_bytes"] == len(golden) and q["blocks"] == 13 and q["streams"] == 1
    for parser in ("auto", "walk"):
        st, out = decode(p, img, z, parser=parser)
        assert st["exit_code"] == 0 and st["reason"] == 0 and st["message"] == "", (parser, st)
        assert st["blocks"] == 13 and st["total_bytes"] == len(golden) and st["decoded_bytes"] == len(golden), st
        assert st["fail_offset"] == len(img)
        assert out == golden.tobytes(), parser


SIZES = [0, 1, B - 1, B, B + 1]


@pytest.mark.parametrize("z,level,sizes", [(True, 3, None), (True, 4, None), (False, 1, SIZES), (True, 1, SIZES), (False, 4, [1, B + 1])])
def test_image_equals_the_cli_files(p, golden, tmp_path, z, level, sizes):
    ref = helpers.ref_cli()
    for n in (sizes or [len(golden)]):
        data = golden[:n]
        img = compress(p, data, z, level)
        mine = cli_compress(p.cli_path(), tmp_path, data, z, level, f"{n}")
        assert img == mine, (z, level, n)
        if ref is not None:
            theirs = cli_compress(ref, tmp_path, data, z, level, f"{n}_ref")
            assert img == theirs, (z, level, n, "reference CLI")
            files = [theirs]
        else:
            files = []
        for f in [img] + files:
            st, out = decode_both(p, f, z)
            assert st["exit_code"] == 0 and out == data.tobytes() and st["total_bytes"] == n, (n, st)
            assert st["blocks"] == (n + B - 1) // B


# ---- 3: shapes the reference accepts that the CLI never writes -------------------------------------------------------
def _lz4_blocks(p, data, cuts):
    """variable block sizes (Hadoop's FourMcOutputStream flushes), reference-encoded; a block that does not shrink is stored"""
    us, cs, sums, pays = [], [], [], []
    at = 0
    for u in cuts:
        blk = data[at:at + u]
        at += u
        r, comp = helpers.orc_compress(blk, u - 1) if u > 1 else (0, None)
        pay = comp.tobytes() if r > 0 else blk.tobytes()
        us.append(u); cs.append(len(pay)); sums.append(helpers.orc_xxh32(np.frombuffer(pay, np.uint8))); pays.append(pay)
    return data[:at].tobytes(), p.assemble_container(p.MAGIC_4MC, us, cs, sums, pays)


def test_variable_blocks_stored_blocks_concatenations_and_a_lying_index(p, golden, tmp_path):
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, 300000, dtype=np.uint8)
    data = np.concatenate([golden[:3 * B], noise, golden[5 * B:5 * B + 700000]])
    want, img = _lz4_blocks(p, data, [65536, 1, B, 1000000, 300000 + 17, B - 5, 123])
    cli = cli_decode(p.cli_path(), tmp_path, img, False, "var")
    assert cli[0] == 0 and cli[2] == want
    st, out = decode_both(p, img, False)
    assert st["exit_code"] == 0 and out == want and st["blocks"] == 7
    # concatenations of 2 and 3 streams, 4mc and 4mz
    for z in (False, True):
        parts = [compress(p, golden[:B + 5], z, 1), compress(p, golden[B:B + 777], z, 2 if not z else 1), img if not z else compress(p, golden[:0], z, 1)]
        outs = [golden[:B + 5].tobytes(), golden[B:B + 777].tobytes(), want if not z else b""]
        for k in (2, 3):
            cat = b"".join(parts[:k])
            cli = cli_decode(p.cli_path(), tmp_path, cat, z, f"cat{k}{z}")
            assert cli[0] == 0 and cli[2] == b"".join(outs[:k])
            st, out = decode_both(p, cat, z)
            assert st["exit_code"] == 0 and st["streams"] == k and out == cli[2], (z, k, st)
    # a footer whose index lies, checksum recomputed: the reference never reads the index
    lie = bytearray(img)
    fsz = int.from_bytes(lie[-12:-8], "big")
    f0 = len(lie) - fsz
    lie[f0 + 12:f0 + 16] = (12345).to_bytes(4, "big")
    lie[-4:] = helpers.orc_xxh32(np.frombuffer(bytes(lie[f0:-4]), np.uint8)).to_bytes(4, "big")
    cli = cli_decode(p.cli_path(), tmp_path, bytes(lie), False, "lie")
    assert cli[0] == 0 and cli[2] == want
    st, out = decode_both(p, bytes(lie), False)
    assert st["exit_code"] == 0 and out == want


# ---- 4: damage, one case per rule of decode_stream -------------------------------------------------------------------
def _be(v):
    return int(v).to_bytes(4, "big")


def _refoot(img):
    """recompute the footer checksum of a single-stream image after an edit of its footer"""
    b = bytearray(img)
    fsz = int.from_bytes(b[-12:-8], "big")
    f0 = len(b) - fsz
    b[-4:] = _be(helpers.orc_xxh32(np.frombuffer(bytes(b[f0:-4]), np.uint8)))
    return bytes(b)


def _damage_cases(p, golden):
    # three blocks: compressed, stored (random bytes do not shrink), a compressed tail
    data = np.concatenate([golden[:B], np.random.default_rng(5).integers(0, 256, B, dtype=np.uint8), golden[2 * B:2 * B + 40000]])
    base = compress(p, data, False, 1)
    n = len(base)
    c0 = int.from_bytes(base[16:20], "big")                    # block 0: header at 12, payload at 24
    h1 = 24 + c0                                               # block 1's header
    c1 = int.from_bytes(base[h1 + 4:h1 + 8], "big")
    assert c1 == B == int.from_bytes(base[h1:h1 + 4], "big")
    h2 = h1 + 12 + c1
    c2 = int.from_bytes(base[h2 + 4:h2 + 8], "big")
    eos = h2 + 12 + c2
    foot = eos + 12
    assert base[eos:eos + 12] == b"\0" * 12 and foot + 20 + 12 == n
    cases = {"empty": b"", "trunc_2": base[:2], "trunc_8": base[:8], "trunc_12": base[:12], "trunc_hdr1": base[:18],
             "trunc_after_hdr": base[:24], "trunc_payload": base[:24 + c0 // 2], "trunc_block_boundary": base[:h1],
             "trunc_block1_hdr": base[:h1 + 7], "trunc_before_eos": base[:eos], "trunc_in_eos": base[:eos + 5],
             "trunc_after_eos": base[:foot], "trunc_footer_2": base[:foot + 2], "trunc_footer_size": base[:foot + 4],
             "trunc_footer_last": base[:n - 1]}
    m = bytearray(base); m[1] ^= 0x40; cases["bad_magic"] = bytes(m)
    m = bytearray(base); m[7] = 2; cases["bad_version"] = bytes(m)
    m = bytearray(base); m[11] ^= 1; cases["bad_header_checksum"] = bytes(m)
    m = bytearray(base); m[h1 + 4:h1 + 8] = _be(B + 1); cases["csize_beyond"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); cases["usize_beyond_sum_ok"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); m[30] ^= 1; cases["usize_beyond_sum_bad"] = bytes(m)
    m = bytearray(base); m[24 + c0 // 3] ^= 0x10; cases["flipped_payload"] = bytes(m)
    m = bytearray(base); m[h2 + 12:h2 + 12 + c2] = b"\xff" * c2
    m[h2 + 8:h2 + 12] = _be(helpers.orc_xxh32(np.frombuffer(bytes(m[h2 + 12:h2 + 12 + c2]), np.uint8))); cases["corrupt_payload_sum_ok"] = bytes(m)
    cases["missing_eos"] = base[:eos] + base[foot:]
    m = bytearray(base); m[-1] ^= 1; cases["bad_footer_checksum"] = bytes(m)
    m = bytearray(base); m[foot + 7] = 2; cases["bad_footer_version"] = _refoot(bytes(m))
    m = bytearray(base); m[foot:foot + 4] = _be(5); cases["footer_size_below_8"] = bytes(m)
    cases["trailing_3"] = base + b"xyz"
    cases["trailing_16"] = base + bytes(range(16))
    second = bytearray(base); second[24 + 100] ^= 1
    cases["second_stream_flip"] = base + bytes(second)
    cases["second_stream_trunc"] = base + base[:h1 + 3]
    return cases


def test_damaged_images_end_as_the_cli_ends(p, golden, tmp_path):
    ref = helpers.ref_cli()
    cases = _damage_cases(p, golden)
    seen = set()
    for name, img in cases.items():
        code, err, out = cli_decode(p.cli_path(), tmp_path, img, False, name)
        st, got = decode_both(p, img, False)
        assert st["exit_code"] == code, (name, st, err)
        if code:
            assert st["message"] and st["message"] in err, (name, st["message"], err)
        else:
            assert st["reason"] == 0
        assert got == out, (name, len(got), len(out))
        seen.add(st["reason"])
        if ref is not None:
            rcode, _, rout = cli_decode(ref, tmp_path, img, False, name + "_ref")
            assert (rcode == 0) == (code == 0) and rout == out, (name, "reference CLI", rcode, code)
        q, _ = decode(p, img, False, query=True)
        if st["reason"] not in (10, 11):                       # payload verdicts are the decode's; the size query parses only
            assert (q["exit_code"], q["reason"]) == (st["exit_code"], st["reason"]), name
    assert seen == set(range(16)), sorted(seen)                # every verdict of decode_stream is reached


def test_damaged_4mz_and_a_small_destination(p, golden, tmp_path):
    base = compress(p, golden[:B + 3000], True, 1)
    c0 = int.from_bytes(base[16:20], "big")
    m = bytearray(base); m[24 + c0 - 1] ^= 0x55
    m[20:24] = _be(helpers.orc_xxh32(np.frombuffer(bytes(m[24:24 + c0]), np.uint8)))
    for name, img in {"z_flip": base[:24] + bytes([base[24] ^ 1]) + base[25:], "z_corrupt": bytes(m), "z_trunc": base[:-3],
                      "z_cat_second": base + base[:30]}.items():
        code, err, out = cli_decode(p.cli_path(), tmp_path, img, True, name)
        st, got = decode_both(p, img, True)
        assert st["exit_code"] == code and got == out, (name, st, err)
        if code:
            assert st["message"] in err, (name, st, err)
    st, _ = decode(p, base, True, cap=B)
    assert st["reason"] == 16 and st["exit_code"] == 1 and st["decoded_bytes"] == 0


# ---- 5: at size ------------------------------------------------------------------------------------------------------
def test_2048_blocks_against_the_host_image_encoder(p):
    import ctypes as C
    nb, distinct = 2048, 48
    base = helpers.corpus(distinct * B)
    d_src = torch.from_numpy(base).cuda().repeat(nb // distinct + 1)[:nb * B].contiguous()
    d_img = torch.empty(p.image_bound(nb * B), dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    # the host image encoder on the same input: block headers + payloads, and the offsets the footer is made of
    host_src = d_src.cpu().numpy()
    blocks = p.make_blocks(np.arange(nb, dtype=np.uint64) * B, np.arange(nb, dtype=np.uint64) * B, [B] * nb, [B] * nb)
    piece = np.empty(nb * (B + 12), dtype=np.uint8)
    ioff = np.zeros(nb, dtype=np.uint64)
    ib = C.c_size_t(0)
    enc_image = C.CDLL(p.lib_path()).fourmc_host_4mc_encode_image        # not in the binding's table: its prototype here
    enc_image.restype = C.c_int
    enc_image.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    rc = enc_image(host_src.ctypes.data, host_src.nbytes, blocks.ctypes.data, nb, p.CODEC_LZ4_FAST, 0,
                   piece.ctypes.data, piece.nbytes, ioff.ctypes.data, C.byref(ib))
    assert rc == 0, p.lib().fourmc_gpu_last_error()
    del host_src
    ib = ib.value
    want = hashlib.sha256()
    want.update(bytes(p.frame_header(p.MAGIC_4MC)))
    want.update(piece[:ib].data)
    want.update(b"\0" * 12)
    want.update(bytes(p.frame_footer(p.MAGIC_4MC, ioff + 12)))
    assert n == 12 + ib + 12 + 20 + 4 * nb
    got = hashlib.sha256(d_img[:n].cpu().numpy().data).hexdigest()
    assert got == want.hexdigest()
    del piece
    d_dst = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    for parser in ("auto", "walk"):
        os.environ["FOURMC_IMAGE_PARSE"] = parser
        try:
            d_dst.zero_()
            st = p.decompress_image(d_img[:n], d_dst, p.MAGIC_4MC)
        finally:
            os.environ.pop("FOURMC_IMAGE_PARSE", None)
        assert st["exit_code"] == 0 and st["blocks"] == nb and st["decoded_bytes"] == nb * B, (parser, st)
        assert torch.equal(d_dst, d_src), parser


# ---- an empty stream ends the file (decompress_file: `do got = decode_stream(..); while (got)`) ----------------------
def test_an_empty_stream_ends_the_file_whatever_follows(p, golden, tmp_path):
    ref = helpers.ref_cli()
    for z in (False, True):
        empty = compress(p, golden[:0], z, 1)
        assert len(empty) == 44
        good = compress(p, golden[:B + 999], z, 1)
        bad = bytearray(good); bad[24 + 100] ^= 1; bad = bytes(bad)
        cases = {"empty_then_3": empty + b"xyz", "empty_then_junk": empty + bytes(range(40)),
                 "empty_then_damaged": empty + bad, "empty_then_stream": empty + good,
                 "stream_empty_then_3": good + empty + b"xyz", "stream_empty_then_damaged": good + empty + bad,
                 "empty_empty_then_damaged": empty + empty + bad}
        for name, img in cases.items():
            code, err, out = cli_decode(p.cli_path(), tmp_path, img, z, f"{name}{z}")
            st, got = decode_both(p, img, z)
            assert code == 0 and st["exit_code"] == 0 and st["reason"] == 0, (name, z, code, err, st)
            assert got == out, (name, z)
            assert out == (golden[:B + 999].tobytes() if name.startswith("stream") else b""), (name, z)
            if ref is not None and not z:
                rcode, _, rout = cli_decode(ref, tmp_path, img, z, f"{name}_ref")
                assert rcode == 0 and rout == out, (name, "reference CLI")


# ---- which parser took an image --------------------------------------------------------------------------------------
def test_the_fast_path_takes_single_streams_and_the_walk_the_rest(p, golden):
    def parsed(img, z, parser=None):
        f0, w0 = p.image_parse_stats()
        old = os.environ.pop("FOURMC_IMAGE_PARSE", None)
        if parser:
            os.environ["FOURMC_IMAGE_PARSE"] = parser
        try:
            d_img = _dev(img)
            d_dst = torch.zeros(len(golden) + 64, dtype=torch.uint8, device="cuda")
            st = p.decompress_image(d_img, d_dst, _magic(p, z), image_bytes=len(img))
        finally:
            os.environ.pop("FOURMC_IMAGE_PARSE", None)
            if old is not None:
                os.environ["FOURMC_IMAGE_PARSE"] = old
        f1, w1 = p.image_parse_stats()
        return st, f1 - f0, w1 - w0
    for z in (False, True):
        img = compress(p, golden, z, 1)
        st, f, w = parsed(img, z)
        assert st["exit_code"] == 0 and (f, w) == (1, 0), (z, st, f, w)            # a CLI-written image: the fast path
        st, f, w = parsed(img, z, "walk")
        assert st["exit_code"] == 0 and (f, w) == (0, 1)
        empty = compress(p, golden[:0], z, 1)
        assert parsed(empty, z)[1:] == (1, 0)                                      # an empty file is one stream too
        assert parsed(img + empty, z)[1:] == (0, 1)                               # a concatenation: the walk
        bad = bytearray(img); bad[-1] ^= 1                                         # a bad footer checksum: the walk
        st, f, w = parsed(bytes(bad), z)
        assert (f, w) == (0, 1) and st["reason"] == 14
        lie = bytearray(img); fsz = int.from_bytes(lie[-12:-8], "big"); f0 = len(lie) - fsz
        lie[f0 + 12:f0 + 16] = (777).to_bytes(4, "big")                           # a lying index, checksum recomputed: the walk
        lie[-4:] = helpers.orc_xxh32(np.frombuffer(bytes(lie[f0:-4]), np.uint8)).to_bytes(4, "big")
        st, f, w = parsed(bytes(lie), z)
        assert (f, w) == (0, 1) and st["exit_code"] == 0
