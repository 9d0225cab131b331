"""CPU-side check (no GPU) of level 1 of the bucket partition with per-chunk count rows: tests/host_emul/part_rows_emul.cpp runs
k_count_rows -> k_scan_rows -> k_tiles -> k_place_rows and the unchanged level 2 (nova_amd/csrc/msm_partition.hpp) thread by thread
on tests/host_emul/simt.hpp and compares with DigitsFn + a sort: per-bucket multisets of (row | sign) words, contiguous start / end,
total = the non-zero digits, the same error word -- the checks tests/test_emul.py makes of the sequence with global atomics -- plus
the two matrices themselves (written from garbage, row by row), guard words around everything the new kernels write, and the layout
of the intermediate arrays that level 2 reads.  The older sequence runs through the same checks alongside.

Level 2 is unchanged code and most of the emulation's run time (a fiber per thread of ~256 tiles on random scalars), so some cases
stop after level 1 (level2=0): they still check everything level 2 reads -- every bin's region, aligned and packed, holding exactly
the bin's (low bits, value) pairs -- the total and the error word; every width, scalar set, grid and mode also runs to the end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "part_rows_emul.cpp")
SO = os.path.join(HERE, "host_emul", "libnmx_part_rows_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "nova_amd", "csrc")
R = util.MODULI[0]  # BN254 Fr: the scalar field the helper instantiates

SETS = ["random", "zero", "equal", "u1", "zero_rm1", "u10"]


@pytest.fixture(scope="module")
def emul():
    deps = [SRC, os.path.join(HERE, "host_emul", "simt.hpp")] + [
        os.path.join(CSRC, f) for f in ("fp.hpp", "curve.hpp", "curves.hpp", "msm_kernels.hpp", "msm_pipeline.hpp", "msm_partition.hpp",
                                        "msm_seg.hpp", "curve_quad.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.emul_part_rows_check.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_uint32] * 9
    L.emul_part_rows_bs1.argtypes = [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
    L.emul_part_rows_bs1.restype = ctypes.c_uint32
    L.emul_part_rows_default.restype = ctypes.c_uint32
    return L


def scalars(n, kind):
    if kind == "zero":  # every row empty, total 0
        return np.zeros((n, 32), np.uint8)
    return np.ascontiguousarray(util.scalar_set(0, n, kind))  # equal: one bin per window takes everything; zero_rm1: negative digits, carries through every window; u10: four bins


def check(L, sc, n, c, rows, grid=0, count_grid=0, stride=None, offset=3, identity_every=0, u64_bits=0, level2=1):
    sc = np.ascontiguousarray(sc)
    return L.emul_part_rows_check(sc.ctypes.data, n, c, u64_bits, grid, count_grid, n + 7 if stride is None else stride, offset,
                                  identity_every, rows, level2)


def sizes(L, c):
    bs1 = L.emul_part_rows_bs1(1 << 12, c, 0)
    assert bs1 == {15: 704, 16: 768, 17: 768}[c]
    return bs1, [1, bs1 - 1, bs1, bs1 + 1, 3 * bs1 + 5]


@pytest.mark.parametrize("c", [15, 16, 17])
def test_count_rows_sequence_every_size_and_scalar_set(emul, c):
    """One chunk, one short of / exactly / one past a chunk, four chunks with a ragged tail; table mode with stride = n + 7,
    offset = 3."""
    _, ns = sizes(emul, c)
    for n in ns:
        for kind in SETS:
            full = kind != "random" or n in (ns[0], ns[3], ns[4])
            assert check(emul, scalars(n, kind), n, c, 1, level2=full) == 0, (c, n, kind)


@pytest.mark.parametrize("c", [15, 16, 17])
@pytest.mark.parametrize("grid", [1, 2])
def test_count_rows_are_indexed_by_chunk_not_by_block(emul, c, grid):
    """Four chunks over one and over two blocks: both passes stride over chunks and address rows by chunk; the counting pass on a
    smaller grid than the placing pass (option hist_grid) as well."""
    bs1, ns = sizes(emul, c)
    n = ns[-1]
    for kind in SETS:
        assert check(emul, scalars(n, kind), n, c, 1, grid=grid) == 0, (c, grid, kind)
    assert check(emul, scalars(n, "random"), n, c, 1, grid=3, count_grid=grid, level2=0) == 0
    n = 7 * bs1 - 1  # seven chunks: blocks with different numbers of chunks
    assert check(emul, scalars(n, "random"), n, c, 1, grid=grid + 1, level2=0) == 0


@pytest.mark.parametrize("c", [15, 16, 17])
def test_count_rows_skip_identity_points_and_report_range_errors_once(emul, c):
    """Keys with identity points among the bases (load() returns false: the pair contributes nothing, in both passes); a scalar
    >= r sets the error word exactly as the sequence with global atomics does, and its pair is dropped."""
    _, ns = sizes(emul, c)
    for n in (ns[3], ns[4]):
        for kind in ("random", "equal", "zero_rm1"):
            assert check(emul, scalars(n, kind), n, c, 1, identity_every=5, level2=kind != "random" or n == ns[4]) == 0, (c, n, kind)
        sc = scalars(n, "random").copy()
        sc[n // 2] = util.int_to_le32(R)      # out of range
        sc[n - 1] = 0xFF                      # out of range, last pair
        assert check(emul, sc, n, c, 1, level2=0) == 0
        assert check(emul, sc, n, c, 1, grid=2, identity_every=3, level2=n == ns[4]) == 0


@pytest.mark.parametrize("c", [15, 16, 17])
def test_count_rows_u64_mode(emul, c):
    """Small-scalar mode (three windows at 33 bits: 1024-thread chunks), in range and with values past 2^bits."""
    for bits in (33, 64):
        bs1 = emul.emul_part_rows_bs1(5000, c, bits)
        assert bs1 == 1024
        for n in (1, bs1 + 1, 3 * bs1 + 5):
            s = np.ascontiguousarray(util.small_scalars(n, bits))
            assert check(emul, s, n, c, 1, stride=n, offset=0, u64_bits=bits, level2=(bits, n) == (33, 3 * bs1 + 5)) == 0, (c, bits, n)
    n = 2 * 1024 + 9
    s = np.ascontiguousarray(util.small_scalars(n, 40))  # most exceed 2^33: ERR_SMALL_RANGE, the pairs dropped
    assert check(emul, s, n, c, 1, stride=n, offset=0, u64_bits=33, grid=1) == 0


@pytest.mark.parametrize("c", [15, 16, 17])
def test_sequence_with_global_atomics_still_passes_alongside(emul, c):
    """k_hist_hi -> k_tiles -> k_part_hi, untouched, through the same checks on the same inputs."""
    _, ns = sizes(emul, c)
    for n in (ns[0], ns[3], ns[4]):
        for kind in SETS:
            assert check(emul, scalars(n, kind), n, c, 0, level2=n == ns[4]) == 0, (c, n, kind)
    n = ns[4]
    assert check(emul, scalars(n, "random"), n, c, 0, grid=2, identity_every=5) == 0


def test_rows_are_off_unless_asked_for(emul):
    """Default-constructed pipeline arguments keep the older kernels: a backend or caller that predates the rows sees no change."""
    assert emul.emul_part_rows_default() == 0


def test_unsupported_shapes_are_refused(emul):
    """The rows cover compile-time widths 15, 16, 17 in the narrow geometry with more than one bin; the helper says so for others."""
    sc = scalars(100, "random")
    for c in (8, 12, 20):
        assert check(emul, sc, 100, c, 1) == -2
