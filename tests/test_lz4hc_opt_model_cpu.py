"""tools/model/lz4hc_opt_model.c on the CPU: the LZ4 HC level 9..12 kernel's serial parse (4mc_amd/csrc/lz4hc_opt_core.h, the
same text the kernel compiles) with its lane-parallel pieces restated lane by lane - batched insert, chain-swap scan over chunks
of 64 deltas, price updates that read before they write - gives the reference's LZ4_compress_HC bytes and return values.
Catches a parse error here, before the device runs it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
from hc_opt_inputs import shapes
from helpers import B, ROOT


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hcopt") / "liblz4hc_opt_model.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "4mc_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tools", "model", "lz4hc_opt_model.c")], check=True)
    L = C.CDLL(so)
    L.lz4hc_opt_model_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lz4hc_opt_model_compress.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def ref():
    r = helpers.ref()
    if r is None:
        pytest.fail("oracle/_ref/libref4mc.so is missing: __graft_entry__.build() makes it where /root/reference exists")
    return r


def _run(fn, s, cap, level):
    s = np.ascontiguousarray(s, dtype=np.uint8)
    d = np.zeros(max(cap, 1) + 64, np.uint8)
    r = fn(s.ctypes.data, d.ctypes.data, len(s), cap, level)
    return r, d[:max(r, 0)].tobytes()


@pytest.mark.parametrize("level", [9, 10, 11, 12])
def test_model_equals_the_reference_on_the_shapes(model, ref, level):
    for k, s in shapes().items():
        if level == 12:
            s = s[: 256 << 10]
        n = len(s)
        for cap in (n + n // 255 + 16, max(n - 1, 0), n // 2):
            assert _run(model.lz4hc_opt_model_compress, s, cap, level) == _run(ref.LZ4_compress_HC, s, cap, level), (level, k, cap)


@pytest.mark.parametrize("level", [9, 10, 11, 12])
def test_model_equals_the_reference_on_corpus_blocks(model, ref, level):
    for k in ((0, 5, 8) if level < 12 else (3,)):
        s = helpers.corpus(B, first_block=k)
        assert _run(model.lz4hc_opt_model_compress, s, B - 1, level) == _run(ref.LZ4_compress_HC, s, B - 1, level), (level, k)


def test_model_maps_levels_like_the_reference(model, ref):
    s = helpers.edge_inputs()["text_60k"]
    for level in (0, -7, 13, 1000):
        assert _run(model.lz4hc_opt_model_compress, s, 70000, level) == _run(ref.LZ4_compress_HC, s, 70000, level), level
