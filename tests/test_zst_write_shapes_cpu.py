"""CPU: the catalogue of tests/zst_write_shapes.py and the port of the streaming compressor it is computed with
(oracle.h: orc_zstd_stream_compress_ex).  The port is compared with the reference's ZSTD_compressStream bytes: directly where
oracle/_ref is built, with the committed fixture (tests/golden/zst_write_shapes.json) otherwise."""
import functools
import hashlib
import itertools

import numpy as np
import pytest

import helpers
import zst_write_model as wm
import zst_write_shapes as ws


@functools.lru_cache(None)
def _images():
    """name -> the port's image, without a trace"""
    return {name: ws.port(name) for name in ws.names()}


def _same_as_reference(key, img, reference):
    if helpers.ref() is not None: return img == reference()
    e = ws.fixture()[key]
    return len(img) == e["bytes"] and hashlib.sha256(img).hexdigest() == e["sha256"]


def test_the_ledger_covers_what_is_required():
    led = ws.ledger()
    assert [k for k in ws.REQUIRED if k not in led] == []


def test_unreached_keys_are_not_reached_and_say_why():
    led = ws.ledger()
    assert [k for k in ws.UNREACHED if k in led] == []
    assert not set(ws.UNREACHED) & set(ws.REQUIRED)
    assert all(".c:" in why for why in ws.UNREACHED.values())


def test_the_catalogue_stays_small():
    assert ws.total_bytes() < 400 << 20
    assert set(ws.fixture()) == set(ws.names()) | {"zst_write_model/" + n for n in wm.inputs()}


def test_the_port_writes_the_reference_bytes_on_the_catalogue():
    bad = [n for n, img in _images().items() if not _same_as_reference(n, img, lambda: ws.reference(n))]
    assert bad == []


def test_the_port_writes_the_reference_bytes_on_the_older_inputs():
    bad = []
    for n, (src, lv) in wm.inputs().items():
        if not _same_as_reference("zst_write_model/" + n, helpers.orc_zstd_stream_compress(src, lv), lambda: wm.reference()[n]): bad.append(n)
    assert bad == []


def test_the_fixture_is_what_the_reference_writes():
    if helpers.ref() is None: pytest.skip("oracle/_ref is not built")
    assert ws.fixture_build() == ws.fixture()


def test_the_trace_changes_no_byte():
    assert [n for n in ws.names() if ws.trace(n)[0] != _images()[n]] == []


def test_the_images_decode_to_their_sources():
    for n, img in _images().items():
        src, _ = ws.source(n)
        r, out = helpers.orc_zstd_decompress(img, len(src))
        assert r == len(src) and np.array_equal(out, src), n


def test_every_mutant_changes_some_image():
    """A mutant that no input tells from the port means a missing input."""
    caught = {}
    for mu, what in ws.MUTANTS.items():
        caught[mu] = next((n for n in ws.names() if ws.port(n, mutate=mu) != _images()[n]), None)
        print(f"mutant {mu} ({what}): {caught[mu]}")
    assert [ws.MUTANTS[mu] for mu, n in caught.items() if n is None] == []
    assert len(caught) == 12


def test_the_carry_mutant_is_caught_through_either_offset():
    """the carried offset above dev_max as the first one (Y:) and as the second one (Y2:), at every level"""
    for lv in ws.LEVELS:
        for n in (f"Y:dev_max+1:l{lv}", f"Y2:dev_max+1:l{lv}"):
            assert ws.port(n, mutate=11) != _images()[n], n
        for n in (f"Y:dev_max:l{lv}", f"Y2:dev_max:l{lv}"):          # at dev_max itself both rules keep it
            assert ws.port(n, mutate=11) == _images()[n], n


def test_the_levels_are_told_apart():
    """for every pair of levels the text input of the higher one gives two images (the same bytes go through both)"""
    for a, b in itertools.combinations(ws.LEVELS, 2):
        src, _ = ws.source(f"T:text:l{b}")
        assert helpers.orc_zstd_stream_compress(src, a) != helpers.orc_zstd_stream_compress(src, b), (a, b)
        if helpers.ref() is not None: assert helpers.orc_zstd_stream_compress(src, b) == ws.zm.zstcodec(src, b)
