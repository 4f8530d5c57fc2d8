"""The streams the tests of fourmc_gpu_images_compress_writes share: (name, data, write sizes or a uniform write_bytes), with M = 4 MiB.
Built once per process; tests/test_fourmc_stream_cpu.py runs the model over them and tests/test_gpu_images_writes.py the device."""
import functools

import numpy as np

import helpers

M = 4 << 20


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def zstd_capacity_case():
    """A block on which ZSTD_compress at level 1 gives other bytes into u - 1 bytes (the CLI's call) than into its bound (the JNI's),
    while the result stays below u: noise with a little text.  None: the seeded search of tests/test_fourmc_stream_cpu.py found none
    (DESIGN_NOTES.md says which)."""
    return None


class Case:
    def __init__(self, name, data, sizes=None, write_bytes=None):
        self.name, self.data = name, bytes(data)
        self.uniform = sizes is None
        self.write_bytes = write_bytes or 0
        if self.uniform:
            n, w = len(self.data), self.write_bytes or len(self.data)
            sizes = ([w] * (n // w) + ([n % w] if n % w else [])) if n else []
        self.sizes = [int(s) for s in sizes]
        assert sum(self.sizes) == len(self.data), name


@functools.lru_cache(maxsize=None)
def full():
    """about 20 streams, 12 full-size blocks in all"""
    text = helpers.corpus(3 * M).tobytes()

    def t(n, at=0):
        return text[at:at + n]
    many = [100] * 70000
    for k in (0, 63, 64, 4095, 4096, 4097, 41943, 69999):
        many[k] = 0
    out = [
        Case("no writes", b"", []),
        Case("only zero-length writes", b"", [0, 0, 0]),
        Case("[1]", t(1), [1]),
        Case("[0, 3, 0, 0, 5, 0]", t(8, 100), [0, 3, 0, 0, 5, 0]),
        Case("[M/2, M/2, 1]", t(M + 1), [M // 2, M // 2, 1]),
        Case("[M-1, 2]", t(M + 1, 4096), [M - 1, 2]),
        Case("[M-1, 1, 1]", t(M + 1, 8192), [M - 1, 1, 1]),
        Case("[M+1, 5]", t(M + 6, 12288), [M + 1, 5]),
        Case("[1, M+1]", t(M + 2, 16384), [1, M + 1]),
        Case("[2M]", t(2 * M, M), [2 * M]),
        Case("70000 writes of 100 with zeros", t(sum(many), 1000), many),
        Case("noise [M]", _noise(M, 11), [M]),
        Case("noise [70000]", _noise(70000, 12), [70000]),
        Case("text then noise", t(M - 100000, 2 * M) + _noise(200000, 13), [M - 100000, 200000]),
        Case("uniform 0", t(50000, 777), write_bytes=0),
        Case("uniform 1000", t(50500, 999), write_bytes=1000),
        Case("uniform M", t(100000, 5555), write_bytes=M),
        Case("uniform M+1", t(M + 10, 2 * M - 50), write_bytes=M + 1),
        Case("uniform, empty", b"", write_bytes=100),
    ]
    z = zstd_capacity_case()
    if z is not None:
        out.append(Case("zstd capacity", z, [len(z)]))
    return out


@functools.lru_cache(maxsize=None)
def reduced():
    """for the slow levels: every block at or below 256 KiB"""
    text = helpers.corpus(1 << 20).tobytes()
    return [
        Case("[1]", text[:1], [1]),
        Case("[0, 3, 0, 0, 5, 0]", text[100:108], [0, 3, 0, 0, 5, 0]),
        Case("3000 writes of 100, table", text[5000:5000 + 250000] + text[:50000], [100] * 3000),
        Case("3000 writes of 100, uniform", text[5000:5000 + 250000] + text[:50000], write_bytes=100),
        Case("noise [70000]", _noise(70000, 12), [70000]),
        Case("text and noise", text[300000:400000] + _noise(60000, 14) + text[400000:440000], [100000, 60000, 40000]),
    ]
