"""The sparse-matrix row primitive at its class, operand and length edges, without a GPU.  (1) The fixtures of
tests/spmv_edges_common.py are what they claim to be.  (2) The C oracle oracle.cref.spmv -- the yardstick of
tests/r1cs_sat_common.Instance.products and of most GPU tests -- equals oracle.pyref.spmv on the canonical variant of every fixture.
(3) spmv_row + st (nova_amd/csrc/spmv_row.hpp) run on the CPU with limb bounds asserted (tests/host_emul/spmv_emul.cpp, built here
with -DNMX_DEBUG_BOUNDS) over the grid and the pile-up matrices, tagged and untagged, operand words >= p included: every output is the
big-integer product byte for byte and < p.  What the emulation does NOT run: registration (SpmvClassifyFn, the conversion of the
coefficients), SpmvPairFn, k_spmv_heavy and transposed_of -- tests/test_gpu_spmv_edges.py covers those."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import cref
from tests import fv_common as C
from tests import spmv_edges_common as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SRC = os.path.join(ROOT, "tests", "host_emul", "spmv_emul.cpp")
EMUL_SO = os.path.join(ROOT, "tests", "host_emul", "libnmx_spmv_emul.so")
CSRC = os.path.join(ROOT, "nova_amd", "csrc")
RI = 1 << 261  # the internal residue form: x * 2^261 mod p (nova_amd/csrc/fp.hpp)
FIDS = sorted(C.FIELDS)


# ---- (1) the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_fixtures_are_what_they_claim(fid):
    p = C.FIELDS[fid]
    co, z = X.COEFFS(p), X.ZVALS(p)
    assert {X.coefficient_class(p, c) for c in co} == set(range(15)), "COEFFS must hold all fifteen classes"
    assert [X.coefficient_class(p, c) for c in (0, 8, p - 8, (p - 1) // 2, 1 << 253)] == [0] * 5
    assert len(set(co)) == len(co) == 21 and all(0 <= c < p for c in co)
    assert z[X.P_MINUS_1_COL] == p - 1 and z[X.ALL_ONES_COL] == (1 << 256) - 1
    assert all(w < p for w in z[:X.NONCANON_FROM]) and z[X.NONCANON_FROM:] == [p, p + 1, 2 * p + 5, (1 << 256) - 1]
    assert all(w < (1 << 256) for w in z)
    g = X.grid_csr(fid)
    assert (g.rows, g.cols) == (len(co) * len(z), len(z)) and g.classes() == set(range(15))
    assert np.array_equal(np.diff(g.indptr.astype(np.int64)), np.ones(g.rows, np.int64))
    assert g.times(z) == [c * (w % p) % p for c in co for w in z]
    t = X.grid_T(fid)
    assert (t.rows, t.cols) == (g.cols, g.rows) and t.column_lengths() == [1] * g.rows
    assert t.transposed_times(z) == g.times(z)
    pl = X.pileup_csr(fid)
    assert np.diff(pl.indptr.astype(np.int64)).tolist() == [n for n in X.PILEUP_LENGTHS for _ in X.PILEUP_FILLS]
    assert set(X.PILEUP_LENGTHS) >= {5, 6, 7, 11, 12, 13, 18, 19} and set(pl.indices.tolist()) == {X.P_MINUS_1_COL}
    assert pl.classes() == {0, 2, 8, 14}
    other = X.pileup_csr(fid, X.ALL_ONES_COL)
    assert other.coeffs == pl.coeffs and set(other.indices.tolist()) == {X.ALL_ONES_COL}
    for v in X.COLUMN_VARIANTS:
        m = X.column_lengths_csr(fid, v)
        assert (m.rows, m.cols) == (32768, 16)
        assert m.column_lengths() == list(X.COLUMN_LENGTHS)
    assert sorted(X.COLUMN_LENGTHS) == [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4096, 4097, 24576, 24577, 32768]
    # the partials a split column leaves (chunks of 16): one full block of lanes, one more, six per lane, one more, eight per lane
    assert [-(-n // 16) for n in (4096, 4097, 24576, 24577, 32768)] == [256, 257, 1536, 1537, 2048]
    assert X.COLUMN_LENGTHS[0] > 32 and X.COLUMN_LENGTHS[-1] > 32 and all(n > 32 for n in X.COLUMN_LENGTHS[12:])
    assert X.column_lengths_csr(fid, "classes").classes() == set(range(15))
    m = X.column_lengths_csr(fid, "general")
    assert {0, 1, p - 1, p - 2, 2} <= set(m.coeffs) and {0, 1, p - 1, p - 2, 2} <= set(X.column_x(fid, "general"))
    sh = {s.name: s for s in X.shape_csrs(fid)}
    assert [sh[n].rows for n in ("rows1", "rows255", "rows256", "rows257")] == [1, 255, 256, 257]
    assert len(sh["nnz0"].coeffs) == 0 and sh["nnz0"].times([1, 2, 3]) == [0] * 5
    assert sh["last_row_only"].indptr.tolist() == [0] * 257 + [9]


# ---- (2) the C oracle on the canonical variants ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_c_oracle_equals_python_integers_on_every_canonical_fixture(fid):
    import __graft_entry__
    __graft_entry__.build()
    for m, z in X.canonical_fixtures(fid):
        assert all(w < m.p for w in z), m.name
        want = X.column_expect_forward(fid, m.name[len("columns_"):]) if m.name.startswith("columns_") else m.times(z)
        got = C.ints(np.frombuffer(cref.spmv(fid, m.indptr, m.indices, m.data if len(m.coeffs) else np.zeros((1, 32), np.uint8), m.rows, C.vec(z)), np.uint8))
        assert got == list(want), m.name


# ---- (3) spmv_row under the emulation, limb bounds asserted ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in ("fp.hpp", "spmv_row.hpp")]
    if not os.path.exists(EMUL_SO) or os.path.getmtime(EMUL_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DNMX_DEBUG_BOUNDS", "-shared", "-fPIC", "-o", EMUL_SO, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_SO)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emul_spmv.argtypes = [ctypes.c_int, vp, vp, vp, vp, u32, u32, vp]
    lib.emul_spmv_index_mask.argtypes = [ctypes.c_uint64]
    lib.emul_spmv_index_mask.restype = u32
    return lib


def u32_words(vals):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals) or bytes(32), np.uint32).copy()


def emulate(E, m, words, tagged):
    """the device-side arrays as registration leaves them, made here with big integers: class bits in the index (tagged) or none
    (colmask all ones: every entry takes the general product), coefficients as c * 2^261 mod p; the words go in as they are"""
    p = m.p
    cls = [X.coefficient_class(p, c) if tagged else 0 for c in m.coeffs]
    ip = m.indptr.astype(np.uint32)
    ix = np.array([int(c) | (t << 28) for c, t in zip(m.indices, cls)] or [0], np.uint32)
    dt, zw = u32_words([c * RI % p for c in m.coeffs]), u32_words(words)
    out = np.full(m.rows * 8, 0xa5a5a5a5, np.uint32)
    assert E.emul_spmv(m.fid, ip.ctypes.data, ix.ctypes.data, dt.ctypes.data, zw.ctypes.data, (1 << 28) - 1 if tagged else 0xffffffff, m.rows,
                       out.ctypes.data) == 0
    return C.ints(out.view(np.uint8))


@pytest.mark.parametrize("tagged", [True, False], ids=["tagged", "untagged"])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_grid_every_class_times_every_word(E, fid, tagged):
    m, z = X.grid_csr(fid), X.ZVALS(C.FIELDS[fid])
    got, want = emulate(E, m, z, tagged), m.times(z)
    bad = [X.grid_pair_name(fid, r) for r in range(m.rows) if got[r] != want[r]]
    assert not bad, bad[:8]
    assert all(g < m.p for g in got)


@pytest.mark.parametrize("tagged", [True, False], ids=["tagged", "untagged"])
@pytest.mark.parametrize("col", [X.P_MINUS_1_COL, X.ALL_ONES_COL], ids=["p-1", "2^256-1"])
@pytest.mark.parametrize("fid", FIDS)
def test_emulated_pileup_rows_either_side_of_the_six_term_reduction(E, fid, col, tagged):
    m, z = X.pileup_csr(fid, col), X.ZVALS(C.FIELDS[fid])
    got, want = emulate(E, m, z, tagged), m.times(z)
    bad = [X.pileup_row_name(r) for r in range(m.rows) if got[r] != want[r]]
    assert not bad, bad[:8]
    assert all(g < m.p for g in got)


@pytest.mark.parametrize("fid", [1, 2])
def test_emulated_shapes(E, fid):
    for m in X.shape_csrs(fid):
        w = X.shape_words(fid, m.cols, 41 + fid)
        for tagged in (True, False):
            assert emulate(E, m, w, tagged) == m.times(w), (m.name, tagged)


def test_index_mask_leaves_the_class_bits_only_when_the_indices_leave_room(E):
    assert E.emul_spmv_index_mask(1 << 28) == (1 << 28) - 1
    assert E.emul_spmv_index_mask((1 << 28) + 1) == 0xffffffff
    assert E.emul_spmv_index_mask(1) == (1 << 28) - 1 and E.emul_spmv_index_mask(0) == (1 << 28) - 1
