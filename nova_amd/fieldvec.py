"""Field-vector kernels either side of the MSM: thin marshalling over the C ABI.

Reference sites (relative to /root/reference):
  axpy        W = W1 + r*W2, E = E1 + r*T           src/r1cs/mod.rs:1058-1067   (RelaxedR1CSWitness::fold)
  axpy2       E = E1 + r*T + r^2*E2                 src/r1cs/mod.rs:1096-1101   (fold_relaxed)
  cross_term  T = AZ o BZ - u*CZ - E                src/r1cs/mod.rs:614-620     (commit_T)
  cross_term2 T = AZ o BZ - u*CZ - E1 - E2          src/r1cs/mod.rs:652-659     (commit_T_relaxed)
  vec_add     Z = Z1 + Z2                           src/r1cs/mod.rs:590-609
  bind_poly_var_top                                 src/spartan/polys/multilinear.rs:65-84
  fold_pairs  Pi[j] = P[2j] + x*(P[2j+1] - P[2j])   src/provider/hyperkzg.rs:1085-1095
Vectors: (n, 32) uint8 numpy arrays (host) or torch CUDA uint8 tensors (HBM-resident; the result is then a CUDA
tensor too and can be passed straight to DlogGroup.vartime_multiscalar_mul).  Field ids as include/nova_mi355x.h.
"""
import numpy as np

from . import _lib as L
from .provider import _check, _host_u8, _is_device_tensor

BN254_FQ, BN254_FR, PASTA_FP, PASTA_FQ = 0, 1, 2, 3
SCALAR_FIELD_OF_CURVE = {0: BN254_FR, 1: BN254_FQ, 2: PASTA_FQ, 3: PASTA_FP}


def _vec(x):
    if _is_device_tensor(x):
        assert x.is_contiguous() and x.numel() * x.element_size() % 32 == 0
        return x.data_ptr(), x.numel() * x.element_size() // 32, True, x
    a = _host_u8(x, 32)
    return a.ctypes.data, a.size // 32, False, a


def _out_like(dev, n, ref):
    if dev:
        import torch
        o = torch.empty((n, 32), dtype=torch.uint8, device=ref.device)
        return o.data_ptr(), o
    o = np.zeros((n, 32), dtype=np.uint8)
    return o.ctypes.data, o


def _chal(r):
    a = _host_u8(r, 32)
    assert a.size == 32
    return a


def _flags(dev, mont, async_=False):
    """async_ (NMX_ASYNC): device-resident operands only -- the call returns once its kernel is enqueued; the calling thread's
    next synchronous call (any MSM / commitment / reduction) or sync() completes it.  Keep the operand tensors alive until then:
    torch's allocator knows nothing about the library's stream."""
    return (L.SCALARS_DEVICE if dev else 0) | (L.SCALARS_MONT if mont else 0) | (L.ASYNC if (async_ and dev) else 0)


def sync():
    """nmx_sync: wait for this thread's asynchronous calls."""
    _check(L.lib().nmx_sync())


def axpy(field, a, b, r, mont=False, async_=False):
    pa, n, dev, _ka = _vec(a)
    pb, nb, devb, _kb = _vec(b)
    assert n == nb and dev == devb, "InvalidWitnessLength (r1cs/mod.rs:1054-1056)"
    po, out = _out_like(dev, n, a)
    rr = _chal(r)
    _check(L.lib().nmx_field_axpy(field, pa, pb, rr.ctypes.data, n, _flags(dev, mont, async_), po))
    return out


def axpy2(field, a, b, c, r, mont=False, async_=False):
    pa, n, dev, _ka = _vec(a)
    pb, nb, _d1, _kb = _vec(b)
    pc, nc, _d2, _kc = _vec(c)
    assert n == nb == nc
    po, out = _out_like(dev, n, a)
    rr = _chal(r)
    _check(L.lib().nmx_field_axpy2(field, pa, pb, pc, rr.ctypes.data, n, _flags(dev, mont, async_), po))
    return out


def cross_term(field, az, bz, cz, e, u, mont=False, async_=False):
    p1, n, dev, _k1 = _vec(az)
    p2, n2, _d2, _k2 = _vec(bz)
    p3, n3, _d3, _k3 = _vec(cz)
    p4, n4, _d4, _k4 = _vec(e)
    assert n == n2 == n3 == n4
    po, out = _out_like(dev, n, az)
    uu = _chal(u)
    _check(L.lib().nmx_field_cross_term(field, p1, p2, p3, p4, uu.ctypes.data, n, _flags(dev, mont, async_), po))
    return out


def cross_term2(field, az, bz, cz, e1, e2, u, mont=False, async_=False):
    """T = AZ o BZ - u*CZ - E1 - E2, u = U1.u + U2.u (commit_T_relaxed, src/r1cs/mod.rs:652-659)."""
    ps = [_vec(x) for x in (az, bz, cz, e1, e2)]
    n, dev = ps[0][1], ps[0][2]
    assert all(q[1] == n for q in ps)
    po, out = _out_like(dev, n, az)
    uu = _chal(u)
    _check(L.lib().nmx_field_cross_term2(field, *[q[0] for q in ps], uu.ctypes.data, n, _flags(dev, mont, async_), po))
    return out


def vec_add(field, a, b, mont=False, async_=False):
    pa, n, dev, _ka = _vec(a)
    pb, nb, _d, _kb = _vec(b)
    assert n == nb
    po, out = _out_like(dev, n, a)
    _check(L.lib().nmx_field_vec_add(field, pa, pb, n, _flags(dev, mont, async_), po))
    return out


def batch_invert(field, v, mont=False):
    """batch_invert (src/spartan/mod.rs:54-118): element-wise inverses; NmxError(E_ZERO) when an element is zero."""
    pv, n, dev, _kv = _vec(v)
    po, out = _out_like(dev, n, v)
    _check(L.lib().nmx_field_batch_invert(field, pv, n, _flags(dev, mont), po))
    return out


def concat(field, parts, n_out=None, async_=False):
    """nmx_field_concat: an HBM-resident vector = the parts (CUDA tensors or host arrays) one after the other, zero-padded to n_out.
    Spartan's z = [W, u, X] (src/spartan/snark.rs:133, 193-196); with one part, a clone ordered on the library's stream."""
    import ctypes
    import torch
    k = len(parts)
    ps = [_vec(p) for p in parts]
    total = sum(q[1] for q in ps)
    n = total if n_out is None else n_out
    mask = sum(1 << i for i, q in enumerate(ps) if q[2])
    ptrs = (ctypes.c_void_p * max(k, 1))(*[q[0] for q in ps])
    lens = (ctypes.c_size_t * max(k, 1))(*[q[1] for q in ps])
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    _check(L.lib().nmx_field_concat(field, ptrs, lens, mask, k, n, _flags(True, False, async_), out.data_ptr()))
    return out


def bind_poly_var_top(field, z, r, mont=False, in_place=False, async_=False):
    """Returns the bound polynomial (len/2 evaluations).  in_place (device tensors only) overwrites z[:len/2]."""
    pz, n, dev, _kz = _vec(z)
    assert n >= 2 and n % 2 == 0, "assert!(self.num_vars > 0)"
    rr = _chal(r)
    if in_place:
        assert dev
        _check(L.lib().nmx_mle_bind_top(field, pz, n, rr.ctypes.data, _flags(dev, mont, async_), pz))
        return z.view(-1)[: (n // 2) * 32].view(n // 2, 32)
    po, out = _out_like(dev, n // 2, z)
    _check(L.lib().nmx_mle_bind_top(field, pz, n, rr.ctypes.data, _flags(dev, mont, async_), po))
    return out


def fold_pairs(field, p, x, mont=False, async_=False):
    pp, n, dev, _kp = _vec(p)
    assert n >= 2 and n % 2 == 0
    xx = _chal(x)
    po, out = _out_like(dev, n // 2, p)
    _check(L.lib().nmx_poly_fold_pairs(field, pp, n, xx.ctypes.data, _flags(dev, mont, async_), po))
    return out


def fold_chain(field, p, xs, mont=False, async_=False):
    """nmx_poly_fold_chain: HyperKZG's fold loop (hyperkzg.rs:1085-1095) in one call -- [fold(p, xs[0]), fold(that, xs[1]), ...]."""
    import ctypes
    pp, n, dev, _kp = _vec(p)
    xx = _host_u8(xs, 32)
    k = xx.size // 32
    assert n >= 2 and n & (n - 1) == 0 and (n >> k) >= 1
    outs = [_out_like(dev, n >> (i + 1), p) for i in range(k)]
    ptrs = (ctypes.c_void_p * k)(*[o[0] for o in outs])
    _check(L.lib().nmx_poly_fold_chain(field, pp, n, xx.ctypes.data, k, _flags(dev, mont, async_), ptrs))
    return [o[1] for o in outs]


def sumcheck_eq_sums(field, mode, A, B, C, eq_right, eq_left=None, shift=0, mont=False):
    """(t_0, t_inf) of EqSumCheckInstance::evaluation_points_{quadratic_with_one_input (mode 1),
    cubic_with_two_inputs (2), cubic_with_three_inputs (3)} (src/spartan/sumcheck.rs:900-1075) as two 32-byte field
    elements.  eq_left given: first-half rounds, factor = eq_left[id >> shift] * eq_right[id & (2^shift - 1)]."""
    pa, n, dev, _ka = _vec(A)
    pb = pc = None
    keep = []
    if mode >= 2:
        pb, nb, _d, kb = _vec(B)
        assert nb == n
        keep.append(kb)
    if mode >= 3:
        pc, nc, _d, kc = _vec(C)
        assert nc == n
        keep.append(kc)
    pr, nr, _d, kr = _vec(eq_right)
    pl, nl = None, 0
    if eq_left is not None:
        pl, nl, _d, kl = _vec(eq_left)
        keep.append(kl)
    out = np.zeros(64, dtype=np.uint8)
    _check(L.lib().nmx_sumcheck_eq_sums(field, mode, pa, pb, pc, n, pl, nl, pr, nr, shift, _flags(dev, mont), out.ctypes.data))
    return out[:32].tobytes(), out[32:].tobytes()


def sumcheck_bind_eq_sums(field, mode, A, B, C, r, eq_right, eq_left=None, shift=0, mont=False):
    """One prover round fused (nmx_sumcheck_bind_eq_sums): binds the HBM-resident tables A, B, C IN PLACE with the
    challenge r and returns (A', B', C', (t_0, t_inf)) where the sums are the next round's, over the bound tables."""
    parts = [_vec(x) if x is not None else (None, 0, True, None) for x in (A, B, C)]
    n = parts[0][1]
    assert all(pt[2] for pt in parts), "HBM-resident tables only"
    assert n >= 4 and n % 4 == 0
    pr, nr, _d, _kr = _vec(eq_right)
    pl, nl = None, 0
    if eq_left is not None:
        pl, nl, _d, _kl = _vec(eq_left)
    rr = _chal(r)
    out = np.zeros(64, dtype=np.uint8)
    _check(L.lib().nmx_sumcheck_bind_eq_sums(field, mode, parts[0][0], parts[1][0], parts[2][0], n, rr.ctypes.data, pl, nl,
                                               pr, nr, shift, _flags(True, mont), parts[0][0], parts[1][0], parts[2][0],
                                               out.ctypes.data))
    half = lambda x: None if x is None else x.view(-1)[: (n // 2) * 32].view(n // 2, 32)
    return half(A), half(B), half(C), (out[:32].tobytes(), out[32:].tobytes())


def sumcheck_plain_sums(field, kind, A, B, C=None, mont=False):
    """Round sums of the sum-checks without an eq factor (src/spartan/sumcheck.rs): kind 1 compute_eval_points_quad_prod
    (:163-186), 2 ..._linear (:353-378), 3 ..._quadratic (:380-405), 4 ..._cubic (:407-443).  Returns a tuple of two
    (kinds 1-3) or three (kind 4) 32-byte field elements."""
    pa, n, dev, _ka = _vec(A)
    pb, nb, _d, _kb = _vec(B)
    assert nb == n
    pc = None
    if kind == 4:
        pc, nc, _d, _kc = _vec(C)
        assert nc == n
    out = np.zeros(96, dtype=np.uint8)
    _check(L.lib().nmx_sumcheck_plain_sums(field, kind, pa, pb, pc, n, _flags(dev, mont), out.ctypes.data))
    t = (out[:32].tobytes(), out[32:64].tobytes(), out[64:].tobytes())
    return t if kind == 4 else t[:2]


def lincomb_powers(field, vecs, s, n_out=None, mont=False):
    """PolyEvalWitness::batch / batch_diff_size (src/spartan/mod.rs:165-277): sum_j s^j * vecs[j], shorter vectors
    zero-padded to the longest (or to n_out)."""
    import ctypes
    k = len(vecs)
    parts = [_vec(v) for v in vecs]
    dev = bool(parts) and parts[0][2]
    assert all(pt[2] == dev for pt in parts)
    lens = [pt[1] for pt in parts]
    n = max(lens, default=0) if n_out is None else n_out
    ptrs = (ctypes.c_void_p * max(k, 1))(*[pt[0] for pt in parts])
    ln = (ctypes.c_size_t * max(k, 1))(*lens)
    po, out = _out_like(dev, n, vecs[0] if k else None)
    ss = _chal(s)
    _check(L.lib().nmx_field_lincomb_powers(field, ptrs, ln, k, ss.ctypes.data, n, _flags(dev, mont), po))
    return out


def eq_evals_from_points(field, r, mont=False, device=False):
    """EqPolynomial::evals_from_points (src/spartan/polys/eq.rs:54-73): (2^ell, 32) table, r[0] most significant.  device=True: the
    table is built and left in HBM (a CUDA tensor) -- compute_eval_table_sparse's operand, src/spartan/snark.rs:182-184."""
    rr = _host_u8(r, 32)
    ell = rr.size // 32
    if device:
        import torch
        out = torch.empty((1 << ell, 32), dtype=torch.uint8, device="cuda")
        _check(L.lib().nmx_eq_evals_from_points(field, rr.ctypes.data, ell, _flags(True, mont), out.data_ptr()))
        return out
    out = np.zeros((1 << ell, 32), dtype=np.uint8)
    _check(L.lib().nmx_eq_evals_from_points(field, rr.ctypes.data, ell, L.SCALARS_MONT if mont else 0, out.ctypes.data))
    return out


def mle_evaluate(field, z, r, mont=False):
    """MultilinearPolynomial::evaluate (src/spartan/polys/multilinear.rs:88-129)."""
    pz, n, dev, _kz = _vec(z)
    rr = _host_u8(r, 32)
    out = np.zeros(32, dtype=np.uint8)
    _check(L.lib().nmx_mle_evaluate(field, pz, n, rr.ctypes.data, rr.size // 32, _flags(dev, mont), out.ctypes.data))
    return out.tobytes()


def mle_multi_evaluate(field, zs, r, mont=False):
    """MultilinearPolynomial::multi_evaluate_with (src/spartan/polys/multilinear.rs:131-180): list of 32-byte values."""
    import ctypes
    k = len(zs)
    if k == 0:
        return []
    parts = [_vec(z) for z in zs]
    dev = parts[0][2]
    n = parts[0][1]
    assert all(pt[1] == n and pt[2] == dev for pt in parts), "assert!(Zs.iter().all(|z| z.len() == n))"
    rr = _host_u8(r, 32)
    ptrs = (ctypes.c_void_p * k)(*[pt[0] for pt in parts])
    out = np.zeros(32 * k, dtype=np.uint8)
    _check(L.lib().nmx_mle_multi_evaluate(field, ptrs, k, n, rr.ctypes.data, rr.size // 32, _flags(dev, mont), out.ctypes.data))
    return [out[32 * j: 32 * j + 32].tobytes() for j in range(k)]


def r1cs_cross_term(A, B, C, z1, z2, e, u, mont=False, async_=False):
    """commit_T's chain as one call (nmx_r1cs_cross_term; src/r1cs/mod.rs:590-620): T = (A Z)(B Z) - u (C Z) - E with Z = z1 + z2
    (z2 None: Z = z1).  A, B, C: SparseMatrix of one shape; CUDA tensors only."""
    p1, n, dev, _k1 = _vec(z1)
    p2 = _vec(z2)[0] if z2 is not None else None
    pe, ne, _de, _ke = _vec(e)
    assert dev and n == A.cols and ne == A.rows
    po, out = _out_like(dev, A.rows, z1)
    uu = _chal(u)
    _check(L.lib().nmx_r1cs_cross_term(A.handle, B.handle, C.handle, p1, p2, n, pe, uu.ctypes.data, _flags(dev, mont, async_), po))
    return out


def nifs_fold(field, w1, w2, e1, t, r, mont=False, async_=False):
    """R1CSWitness::fold as one launch (nmx_nifs_fold; src/r1cs/mod.rs:1044-1067): (w1 + r w2, e1 + r t).  CUDA tensors only."""
    pw1, nw, dev, _a = _vec(w1)
    pw2, nw2, _d, _b = _vec(w2)
    pe1, ne, _d2, _c = _vec(e1)
    pt, nt, _d3, _e = _vec(t)
    assert dev and nw == nw2 and ne == nt
    pw, w = _out_like(dev, nw, w1)
    pe, e = _out_like(dev, ne, e1)
    rr = _chal(r)
    _check(L.lib().nmx_nifs_fold(field, pw1, pw2, nw, pe1, pt, ne, rr.ctypes.data, _flags(dev, mont, async_), pw, pe))
    return w, e


class SparseMatrix:
    """CSR matrix resident in HBM (src/r1cs/sparse.rs:232-260); multiply_vec = sparse.rs:201-229."""

    def __init__(self, field, indptr, indices, data, cols, mont=False):
        import ctypes
        ip = np.ascontiguousarray(indptr, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint64)
        d = _host_u8(data, 32)
        self.rows, self.cols, self.field = len(ip) - 1, cols, field
        h = ctypes.c_uint64(0)
        _check(L.lib().nmx_spmv_register(field, ip.ctypes.data, ix.ctypes.data, d.ctypes.data, self.rows, cols,
                                         L.SCALARS_MONT if mont else 0, ctypes.byref(h)))
        self.handle = h.value

    def multiply_vec(self, z, mont=False, async_=False):
        pz, n, dev, _kz = _vec(z)
        assert n == self.cols, "invalid shape"
        po, out = _out_like(dev, self.rows, z)
        _check(L.lib().nmx_spmv_apply(self.handle, pz, n, _flags(dev, mont, async_), po))
        return out

    def multiply_vec_pair(self, z1, z2, mont=False, async_=False):
        """(M*z1, M*z2) in one pass (sparse.rs:215-229)."""
        p1, n1, dev, _k1 = _vec(z1)
        p2, n2, dev2, _k2 = _vec(z2)
        assert n1 == self.cols and n2 == self.cols and dev == dev2, "invalid shape"
        po1, out1 = _out_like(dev, self.rows, z1)
        po2, out2 = _out_like(dev, self.rows, z1)
        _check(L.lib().nmx_spmv_apply_pair(self.handle, p1, p2, n1, _flags(dev, mont, async_), po1, po2))
        return out1, out2

    def multiply_vec_transposed(self, x, mont=False, async_=False):
        """M^T x: compute_eval_table_sparse's product (src/spartan/mod.rs:497-533), x over the rows, result over the columns."""
        px, n, dev, _kx = _vec(x)
        assert n == self.rows, "assert_eq!(rx.len(), S.num_cons())"
        po, out = _out_like(dev, self.cols, x)
        _check(L.lib().nmx_spmv_apply_transposed(self.handle, px, n, _flags(dev, mont, async_), po))
        return out

    def close(self):
        if self.handle:
            _check(L.lib().nmx_spmv_unregister(self.handle))
            self.handle = 0


def multiply_vec_many(mats, x, transposed=False, mont=False, async_=False):
    """nmx_spmv_apply_many: [M x for M in mats] (R1CSShape::multiply_vec, src/r1cs/mod.rs:407-471) or, transposed, [M^T x ...]
    (compute_eval_table_sparse, src/spartan/mod.rs:497-533) in one call; HBM-resident x: the products run side by side."""
    import ctypes
    px, n, dev, _kx = _vec(x)
    k = len(mats)
    hs = (ctypes.c_uint64 * k)(*[m.handle for m in mats])
    outs = [_out_like(dev, m.cols if transposed else m.rows, x) for m in mats]
    ptrs = (ctypes.c_void_p * k)(*[o[0] for o in outs])
    _check(L.lib().nmx_spmv_apply_many(hs, k, 1 if transposed else 0, px, n, _flags(dev, mont, async_), ptrs))
    return [o[1] for o in outs]


def r1cs_evaluate(mats, r_x, r_y, mont=False):
    """nmx_r1cs_evaluate: RelaxedR1CSSNARK::verify's multi_evaluate (src/spartan/snark.rs:325-353) as one call --
    [sum over the entries (row, col, val) of M of eq(r_x, row) eq(r_y, col) val  for M in mats], 32 bytes each (Montgomery limbs with
    mont=True, like r_x and r_y then).  mats: 1..8 SparseMatrix over one field (what r1cs_is_sat takes for A, B, C); r_x, r_y: host
    points, most significant variable first, with rows <= 2^len(r_x) and cols <= 2^len(r_y) for every matrix.  The transposed form of
    a matrix is not built."""
    import ctypes
    k = len(mats)
    hs = (ctypes.c_uint64 * max(k, 1))(*[m.handle for m in mats])
    rx, ry = _host_u8(r_x, 32), _host_u8(r_y, 32)
    out = np.zeros((max(k, 1), 32), dtype=np.uint8)
    _check(L.lib().nmx_r1cs_evaluate(hs, k, rx.ctypes.data if rx.size else None, rx.size // 32, ry.ctypes.data if ry.size else None,
                                     ry.size // 32, L.SCALARS_MONT if mont else 0, out.ctypes.data))
    return [out[i].tobytes() for i in range(k)]


def suffix_horner(field, f, u, mont=False):
    """out[i] = sum_{k>=i} f[k] u^(k-i): out[0] = poly_eval(f, u) (hyperkzg.rs:1011-1020), out[1:] = the quotient of
    div_by_monomial(f, u) (hyperkzg.rs:961-999)."""
    pf, n, dev, _kf = _vec(f)
    uu = _chal(u)
    po, out = _out_like(dev, n, f)
    _check(L.lib().nmx_poly_suffix_horner(field, pf, n, uu.ctypes.data, _flags(dev, mont), po))
    return out


def lincomb_quotients(field, polys, q, points, mont=False, async_=False):
    """The three openings of kzg_open_batch (hyperkzg.rs:1007-1072) in one pass (nmx_poly_lincomb_quotients): with B = sum_i q^i polys[i]
    (ragged lengths, never stored), returns [out_j for the m <= 3 points u_j], out_j[t] = sum_{s >= t} B[s] u_j^(s - t) over
    max len(polys[i]) elements: out_j[0] = B(u_j), out_j[1:] = the quotient of div_by_monomial(B, u_j).  Byte-identical to
    lincomb_powers + suffix_horner per point.  Host arrays or CUDA tensors (all on the same side)."""
    import ctypes
    k = len(polys)
    pts = _host_u8(points, 32)
    m = pts.size // 32
    parts = [_vec(f) if len(f) else (None, 0, None, None) for f in polys]
    devs = {pt[2] for pt in parts if pt[2] is not None}
    assert len(devs) <= 1, "all vectors on the same side"
    dev = bool(devs) and devs.pop()
    n_out = max([pt[1] for pt in parts], default=0)
    like = next((f for f, pt in zip(polys, parts) if pt[2] is not None), None)
    ptrs = (ctypes.c_void_p * max(k, 1))(*[pt[0] for pt in parts])
    lens = (ctypes.c_size_t * max(k, 1))(*[pt[1] for pt in parts])
    outs = [_out_like(dev, n_out, like) for _ in range(m)]
    po = (ctypes.c_void_p * max(m, 1))(*[o[0] for o in outs])
    qq = _chal(q)
    _check(L.lib().nmx_poly_lincomb_quotients(field, ptrs, lens, k, qq.ctypes.data, pts.ctypes.data if m else None, m,
                                              _flags(dev, mont, async_), po))
    return [o[1] for o in outs]


def poly_eval_multi(field, polys, points, mont=False):
    """[[f_i(u_j) for j] for i] in one launch (nmx_poly_eval_multi): HyperKZG's v matrix, hyperkzg.rs:1049-1056."""
    import ctypes
    k = len(polys)
    pts = _host_u8(points, 32)
    m = pts.size // 32
    if k == 0 or m == 0:
        return [[] for _ in range(k)]
    parts = [_vec(f) if len(f) else (None, 0, None, None) for f in polys]
    devs = {pt[2] for pt in parts if pt[2] is not None}
    assert len(devs) <= 1
    dev = bool(devs) and devs.pop()
    ptrs = (ctypes.c_void_p * k)(*[pt[0] for pt in parts])
    lens = (ctypes.c_size_t * k)(*[pt[1] for pt in parts])
    out = np.zeros(32 * k * m, dtype=np.uint8)
    _check(L.lib().nmx_poly_eval_multi(field, ptrs, lens, k, pts.ctypes.data, m, _flags(dev, mont), out.ctypes.data))
    return [[out[32 * (i * m + j): 32 * (i * m + j) + 32].tobytes() for j in range(m)] for i in range(k)]


def poly_eval(field, f, u, mont=False):
    out = suffix_horner(field, f, u, mont)
    return (out[0].cpu().numpy() if _is_device_tensor(out) else out[0]).tobytes()


def div_by_monomial(field, f, u, mont=False):
    return suffix_horner(field, f, u, mont)[1:]


# ---- Mercury's prover passes (src/provider/mercury.rs): the N-sized steps between its commitments -------------------------------
FIELD_MODULUS = {BN254_FQ: 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
                 BN254_FR: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
                 PASTA_FP: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
                 PASTA_FQ: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001}


def mercury_h_poly(field, f, n_rows, n_cols, eq_col, mont=False, async_=False):
    """compute_h_poly (mercury.rs:369-386): h[row] = sum_col f[row * n_cols + col] * eq_col[col], f viewed as n_rows x n_cols."""
    pf, n, dev, _kf = _vec(f)
    pe, ne, deve, _ke = _vec(eq_col)
    assert n == n_rows * n_cols and ne == n_cols and dev == deve, "f is n_rows x n_cols, eq_col has n_cols entries, both host or both HBM"
    po, out = _out_like(dev, n_rows, f)
    _check(L.lib().nmx_mercury_h_poly(field, pf, n_rows, n_cols, pe, _flags(dev, mont, async_), po))
    return out


def mercury_divide_by_binomial(field, f, n_rows, n_cols, alpha, mont=False, async_=False):
    """divide_by_binomial (mercury.rs:319-356): f(X) = (X^n_cols - alpha) q(X) + g(X) -> (q, g); q has (n_rows - 1) * n_cols elements in the
    reference's layout after its transpose (its b * b vector before trim() without the all-zero tail), g has n_cols."""
    pf, n, dev, _kf = _vec(f)
    assert n == n_rows * n_cols, "f is n_rows x n_cols"
    aa = _chal(alpha)
    pq, q = _out_like(dev, (n_rows - 1) * n_cols, f)
    pg, g = _out_like(dev, n_cols, f)
    _check(L.lib().nmx_mercury_divide_by_binomial(field, pf, n_rows, n_cols, aa.ctypes.data, _flags(dev, mont, async_), pq if n_rows > 1 else None, pg))
    return q, g


def mercury_s_poly(field, a1, b1, a2, b2, gamma, mont=False, async_=False):
    """make_s_polynomial((a1, a2), (b1, b2), log_b, gamma) (mercury.rs:391-475) without its FFTs (nmx_mercury_s_poly): the b - 1
    coefficients of X^1 .. X^(b-1) of a1(X) b1(1/X) + a1(1/X) b1(X) + gamma (a2(X) b2(1/X) + a2(1/X) b2(X)), untrimmed, for four vectors
    of any equal length b >= 1 (all host arrays or all CUDA tensors); gamma a host scalar."""
    ps = [_vec(x) for x in (a1, b1, a2, b2)]
    b, dev = ps[0][1], ps[0][2]
    assert all(q[1] == b and q[2] == dev for q in ps), "four vectors of one length, all host or all HBM"
    gg = _chal(gamma)
    po, out = _out_like(dev, b - 1, a1)
    _check(L.lib().nmx_mercury_s_poly(field, ps[0][0], ps[1][0], ps[2][0], ps[3][0], b, gg.ctypes.data, _flags(dev, mont, async_), po if b > 1 else None))
    return out


def mercury_quot_f(field, f, q, zeta_b_minus_alpha, zeta, mont=False):
    """The quot_f block (mercury.rs:1163-1180) from calls that exist: f - (zeta^b - alpha) q through lincomb_powers over [f, q] with
    s = -(zeta^b - alpha), then suffix_horner at zeta -> (quot, rem).  quot = out[1:] is (f - (zeta^b - alpha) q - g(zeta)) / (X - zeta): it
    does not depend on coefficient 0, so the reference's `coeffs[0] -= g_zeta` never has to touch the vector; rem = out[0] (32 bytes) must
    equal g(zeta), which restates the reference's assert_eq!(rem, ZERO) -- the caller compares."""
    p = FIELD_MODULUS[field]
    z = int.from_bytes(_chal(zeta_b_minus_alpha).tobytes(), "little")
    assert z < p, "zeta^b - alpha >= field modulus"
    s = ((p - z) % p).to_bytes(32, "little")      # -x is p - x in the canonical and in the Montgomery form alike
    pq, nq, _dq, _kq = _vec(q)
    t = lincomb_powers(field, [f, q] if nq else [f], s, mont=mont)
    out = suffix_horner(field, t, zeta, mont)
    return out[1:], (out[0].cpu().numpy() if _is_device_tensor(out) else out[0]).tobytes()


# ---- NeutronNova's folding step (src/neutron/nifs.rs:200-289): pow tables, the zero-fold's sums, the witness fold ---------------------
def pow_split_evals(field, tau, left, right, mont=False, device=None, async_=False):
    """PowPolynomial::new(tau, ell).split_evals(left, right) (power.rs:62-86): [tau^j, j < left] ++ [(tau^left)^i, i < right].  device: a
    torch device for an HBM result (a CUDA tensor), None for a host array."""
    tt = _chal(tau)
    dev = device is not None
    if dev:
        import torch
        out = torch.empty((left + right, 32), dtype=torch.uint8, device=device)
        po = out.data_ptr()
    else:
        out = np.zeros((left + right, 32), dtype=np.uint8)
        po = out.ctypes.data
    _check(L.lib().nmx_pow_split_evals(field, tt.ctypes.data, left, right, _flags(dev, mont, async_), po))
    return out


def _neutron_vecs(left, right, vecs):
    ps = [_vec(x) for x in vecs]
    dev = ps[0][2]
    assert all(q[2] == dev for q in ps), "every vector host or every vector HBM"
    for k, q in enumerate(ps):
        assert q[1] == (left + right if k % 4 == 0 else left * right), "E has left + right elements, Az / Bz / Cz left * right"
    return ps, dev


def neutron_fold_sums(field, left, right, E1, Az1, Bz1, Cz1, E2, Az2, Bz2, Cz2, rho, mont=False):
    """NIFS::prove_helper (neutron/nifs.rs:29-186): the zero-fold's evaluations at t = 0, 2, 3, 4, 5 -> 160 bytes (five elements)."""
    ps, dev = _neutron_vecs(left, right, (E1, Az1, Bz1, Cz1, E2, Az2, Bz2, Cz2))
    rr = _chal(rho)
    out = np.zeros(160, dtype=np.uint8)
    _check(L.lib().nmx_neutron_fold_sums(field, left, right, *[q[0] for q in ps], rr.ctypes.data, _flags(dev, mont), out.ctypes.data))
    return out.tobytes()


def neutron_relation_sum(field, left, right, E, Az, Bz, Cz, mont=False):
    """The sum of Structure::is_sat (neutron/relation.rs:83-97): sum_i f[i] sum_j e[j] (Az Bz - Cz)[i * left + j] -> 32 bytes."""
    ps, dev = _neutron_vecs(left, right, (E, Az, Bz, Cz))
    out = np.zeros(32, dtype=np.uint8)
    _check(L.lib().nmx_neutron_relation_sum(field, left, right, *[q[0] for q in ps], _flags(dev, mont), out.ctypes.data))
    return out.tobytes()


def neutron_fold_witness(field, w1, w2, e1, e2, r_b, mont=False, async_=False, inplace=False):
    """FoldedWitness::fold (neutron/relation.rs:131-156): (w1 + r_b (w2 - w1), e1 + r_b (e2 - e1)) in one launch.  inplace: the results
    overwrite w1 and e1 (and are returned)."""
    pw1, n_w, dev, k1 = _vec(w1)
    pw2, n_w2, d2, _k2 = _vec(w2)
    pe1, n_e, d3, k3 = _vec(e1)
    pe2, n_e2, d4, _k4 = _vec(e2)
    assert n_w == n_w2 and n_e == n_e2 and dev == d2 == d3 == d4, "w1 / w2 and e1 / e2 of equal lengths, all host or all HBM"
    rr = _chal(r_b)
    if inplace:
        (pw, w), (pe, e) = (pw1, k1 if dev else k1.reshape(-1, 32)), (pe1, k3 if dev else k3.reshape(-1, 32))
    else:
        pw, w = _out_like(dev, n_w, w1)
        pe, e = _out_like(dev, n_e, e1)
    _check(L.lib().nmx_neutron_fold_witness(field, pw1, pw2, n_w, pe1, pe2, n_e, rr.ctypes.data, _flags(dev, mont, async_), pw, pe))
    return w, e


# ---- ppsnark's lookup gather and fused logUp oracles (src/spartan/ppsnark.rs:220-253, :371-489) ----------------------------------
def gather(field, mem, addr, mont=False):
    """evaluation_oracles' L_row = eq[row], L_col = z[col] (ppsnark.rs:220-253): out[i] = mem[addr[i]].  addr holds FIELD ELEMENTS whose
    integer values are the addresses (the form row / col are committed in).  NmxError(E_ARG) when an address is not below len(mem)."""
    pm, n_mem, dev, _km = _vec(mem)
    pa, n, deva, _ka = _vec(addr)
    assert dev == deva, "mem and addr both host or both HBM"
    po, out = _out_like(dev, n, mem)
    _check(L.lib().nmx_field_gather(field, pm, n_mem, pa, n, _flags(dev, mont), po))
    return out


def ppsnark_mem_oracles(field, mems, addrs, Ls, tss, gamma, r, mont=False):
    """MemorySumcheckInstance::compute_oracles (ppsnark.rs:371-489) without its commitments, every memory in one call.  Returns per memory
    (t_plus_r, w_plus_r, t_plus_r_inv, w_plus_r_inv): t_plus_r = mem gamma + i + r, w_plus_r = L gamma + addr + r, t_plus_r_inv =
    ts / t_plus_r, w_plus_r_inv = 1 / w_plus_r.  NmxError(E_ZERO) when some t_plus_r or w_plus_r is zero."""
    import ctypes
    k = len(mems)
    assert k == len(addrs) == len(Ls) == len(tss)
    ins = [[_vec(x) for x in group] for group in (mems, addrs, Ls, tss)]
    n, dev = (ins[0][0][1], ins[0][0][2]) if k else (0, False)
    assert all(q[1] == n and q[2] == dev for group in ins for q in group), "every vector has n elements, all host or all HBM"
    outs = [[_out_like(dev, n, mems[m]) for m in range(k)] for _ in range(4)]
    arr = lambda ptrs: (ctypes.c_void_p * max(k, 1))(*ptrs)  # noqa: E731
    g, rr = _chal(gamma), _chal(r)
    _check(L.lib().nmx_ppsnark_mem_oracles(field, k, n, *[arr([q[0] for q in group]) for group in ins], g.ctypes.data, rr.ctypes.data,
                                           _flags(dev, mont), *[arr([o[0] for o in group]) for group in outs]))
    return [tuple(outs[j][m][1] for j in range(4)) for m in range(k)]


# ---- ppsnark's key tables (src/spartan/ppsnark.rs:117-190, src/spartan/polys/masked_eq.rs:57-75) ----------------------------------
def ppsnark_spark_size(nnzs, num_vars, num_cons):
    """N of R1CSShapeSparkRepr::new (ppsnark.rs:118-121): max(total entries, 2 num_vars, num_cons).next_power_of_two()."""
    m = max(sum(nnzs), 2 * num_vars, num_cons, 1)
    return 1 << (m - 1).bit_length()


def ppsnark_spark_repr(mats, n, mont=False, device=True):
    """R1CSShapeSparkRepr::new (ppsnark.rs:117-190) over resident SparseMatrix objects (the reference: A, B, C): returns (row, col, vals,
    ts_row, ts_col), every vector n field elements and vals one vector per matrix -- CUDA tensors with device=True, numpy arrays otherwise.
    n: a power of two, at least the total entry count and every matrix's rows and columns (ppsnark_spark_size gives the reference's)."""
    import ctypes
    k = len(mats)
    hs = (ctypes.c_uint64 * max(k, 1))(*[m.handle for m in mats])
    if device:
        import torch
        ref = torch.empty(0, dtype=torch.uint8, device="cuda")
    else:
        ref = None
    outs = [_out_like(device, n, ref) for _ in range(4 + k)]
    vals = (ctypes.c_void_p * max(k, 1))(*[o[0] for o in outs[2:2 + k]])
    _check(L.lib().nmx_ppsnark_spark_repr(hs, k, n, _flags(device, mont), outs[0][0], outs[1][0], vals, outs[2 + k][0], outs[3 + k][0]))
    return outs[0][1], outs[1][1], [o[1] for o in outs[2:2 + k]], outs[2 + k][1], outs[3 + k][1]


def masked_eq_evals(field, r, num_masked_vars, mont=False, device=False):
    """MaskedEqPolynomial::evals (masked_eq.rs:57-75): eq_evals_from_points(field, r) with the first 2^num_masked_vars entries zero."""
    rr = _host_u8(r, 32)
    ell = rr.size // 32
    ref = None
    if device:
        import torch
        ref = torch.empty(0, dtype=torch.uint8, device="cuda")
    po, out = _out_like(device, 1 << ell, ref)
    _check(L.lib().nmx_masked_eq_evals(field, rr.ctypes.data if ell else None, ell, num_masked_vars, _flags(device, mont), po))
    return out


# ---- Spartan's sum-check provers, one call each (nmx_sumcheck_prove_*; src/spartan/sumcheck.rs:199-507) ---------------------
def as_transcript(fn):
    """fn(list of 32-byte coefficient strings) -> 32-byte challenge, wrapped as nmx_transcript_fn.  The transcript (Keccak on
    the reference's side, src/provider/keccak.rs) is the caller's: `absorb(b"p", &poly); squeeze(b"c")`."""
    import ctypes
    if isinstance(fn, L.TRANSCRIPT_FN):
        return fn

    def cb(_ctx, coeffs, n, out):
        try:
            ch = fn([bytes(coeffs[32 * i: 32 * i + 32]) for i in range(n)])
            ctypes.memmove(out, ch, 32)
            return 0
        except Exception:                   # an exception must not cross the C frame: the call fails with NMX_E_ARG
            import traceback
            traceback.print_exc()
            return 1
    return L.TRANSCRIPT_FN(cb)


def _rows(buf, n, w):
    b = buf.tobytes()
    return [[b[32 * (w * j + i): 32 * (w * j + i) + 32] for i in range(w)] for j in range(n)]


def sumcheck_prove_cubic_with_three_inputs(field, claim, taus, A, B, C, transcript, mont=False, ctx=None):
    """SumcheckProof::prove_cubic_with_three_inputs (src/spartan/sumcheck.rs:446-507) over HBM-resident tables, bound IN PLACE.
    Returns (round polynomials [rounds][4], challenges [rounds], [A(r), B(r), C(r)]) as 32-byte strings."""
    pa, n, dev, _a = _vec(A)
    pb, nb, _d1, _b = _vec(B)
    pc, nc, _d2, _c = _vec(C)
    t = _host_u8(taus, 32)
    nr = t.size // 32
    assert n == nb == nc == (1 << nr) and dev == _d1 == _d2
    cl = _chal(claim)
    polys, r, out = np.zeros(128 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(96, np.uint8)
    cb = as_transcript(transcript)
    _check(L.lib().nmx_sumcheck_prove_cubic_with_three_inputs(field, cl.ctypes.data, t.ctypes.data, nr, pa, pb, pc, _flags(dev, mont),
                                                             cb, ctx, polys.ctypes.data, r.ctypes.data, out.ctypes.data))
    return _rows(polys, nr, 4), [x[0] for x in _rows(r, nr, 1)], _rows(out, 1, 3)[0]


def sumcheck_prove_quad_prod(field, claim, num_rounds, A, B, transcript, mont=False, ctx=None):
    """SumcheckProof::prove_quad_prod (src/spartan/sumcheck.rs:199-249): (polys [rounds][3], challenges, [A(r), B(r)])."""
    pa, n, dev, _a = _vec(A)
    pb, nb, _d1, _b = _vec(B)
    nr = num_rounds
    assert n == nb == (1 << nr) and dev == _d1
    cl = _chal(claim)
    polys, r, out = np.zeros(96 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(64, np.uint8)
    cb = as_transcript(transcript)
    _check(L.lib().nmx_sumcheck_prove_quad_prod(field, cl.ctypes.data, nr, pa, pb, _flags(dev, mont), cb, ctx, polys.ctypes.data,
                                               r.ctypes.data, out.ctypes.data))
    return _rows(polys, nr, 3), [x[0] for x in _rows(r, nr, 1)], _rows(out, 1, 2)[0]


def sumcheck_prove_batch_eval(field, claims, num_rounds, polys, eq_points, coeffs, transcript, mont=False, ctx=None):
    """SumcheckProof::prove_batch_eval (src/spartan/sumcheck.rs:251-353).  polys: CUDA tensors, bound IN PLACE (the reference binds
    clones: pass copies to keep the originals).  Returns (polys [max rounds][3], challenges, [P_i final])."""
    import ctypes
    k = len(polys)
    parts = [_vec(p) for p in polys]
    dev = parts[0][2]
    assert all(pt[2] == dev for pt in parts) and all(pt[1] == (1 << nr) for pt, nr in zip(parts, num_rounds))
    nmax = max(num_rounds)
    pts = [_host_u8(x, 32) for x in eq_points]
    assert all(x.size // 32 == nr for x, nr in zip(pts, num_rounds))
    pp = (ctypes.c_void_p * k)(*[pt[0] for pt in parts])
    qp = (ctypes.c_void_p * k)(*[x.ctypes.data for x in pts])
    nrs = (ctypes.c_size_t * k)(*num_rounds)
    cl = _host_u8(b"".join(claims) if isinstance(claims, (list, tuple)) else claims, 32)
    co = _host_u8(b"".join(coeffs) if isinstance(coeffs, (list, tuple)) else coeffs, 32)
    out_p, r, fin = np.zeros(96 * nmax, np.uint8), np.zeros(32 * nmax, np.uint8), np.zeros(32 * k, np.uint8)
    cb = as_transcript(transcript)
    _check(L.lib().nmx_sumcheck_prove_batch_eval(field, cl.ctypes.data, nrs, pp, qp, co.ctypes.data, k, _flags(dev, mont), cb, ctx,
                                                out_p.ctypes.data, r.ctypes.data, fin.ctypes.data))
    return _rows(out_p, nmax, 3), [x[0] for x in _rows(r, nmax, 1)], [x[0] for x in _rows(fin, k, 1)]


def sumcheck_prove_batched_cubic(field, claim, taus, As, Bs, Cs, alphas, transcript, mont=False, ctx=None):
    """SumcheckProof::prove_batched_cubic (src/spartan/sumcheck.rs:509-577): sum_x eq(tau, x) sum_i alpha_i (A_i B_i - C_i)(x) = claim for
    k = len(As) <= 16 triples under one sum-check.  As, Bs, Cs: k tables each of 2^len(taus) elements -- CUDA tensors, bound IN PLACE
    (contents unspecified afterwards), or host arrays (uploaded for the call, left untouched); two tables must not share memory.  taus,
    alphas, claim: host.  Returns (round polynomials [rounds][4], challenges [rounds], [[A_i(r), B_i(r), C_i(r)] for i]) as 32-byte
    strings."""
    import ctypes
    k = len(As)
    assert k == len(Bs), "assert_eq!(k, polys_B.len())"
    assert k == len(Cs), "assert_eq!(k, polys_C.len())"
    al = _host_u8(alphas, 32)
    assert k == al.size // 32, "assert_eq!(k, alphas.len())"
    t = _host_u8(taus, 32)
    nr = t.size // 32
    parts = [_vec(x) for x in list(As) + list(Bs) + list(Cs)]
    dev = parts[0][2] if parts else False
    assert all(pt[2] == dev for pt in parts), "all tables in HBM or all on the host"
    assert all(pt[1] == (1 << nr) for pt in parts), "every table holds 2^len(taus) elements"
    ptrs = [(ctypes.c_void_p * max(k, 1))(*[pt[0] for pt in parts[w * k:(w + 1) * k]]) for w in range(3)]
    cl = _chal(claim)
    polys, r, out = np.zeros(128 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(96 * max(k, 1), np.uint8)
    cb = as_transcript(transcript)
    _check(L.lib().nmx_sumcheck_prove_batched_cubic(field, cl.ctypes.data, t.ctypes.data if nr else None, nr, ptrs[0], ptrs[1], ptrs[2],
                                                   al.ctypes.data if k else None, k, _flags(dev, mont), cb, ctx, polys.ctypes.data,
                                                   r.ctypes.data, out.ctypes.data))
    return _rows(polys, nr, 4), [x[0] for x in _rows(r, nr, 1)], _rows(out, k, 3)


PPS_TABLES = ("t_plus_r_row", "t_plus_r_inv_row", "w_plus_r_row", "w_plus_r_inv_row", "ts_row", "t_plus_r_col", "t_plus_r_inv_col", "w_plus_r_col",
              "w_plus_r_inv_col", "ts_col", "L_row", "L_col", "val", "E", "W", "masked_eq")    # include/nova_mi355x.h NMX_PPS_*


def sumcheck_prove_ppsnark(field, tables, rhos, r_outer, claims2, coeffs, transcript, mont=False, ctx=None):
    """RelaxedR1CSSNARK::prove_helper (src/spartan/ppsnark.rs:886-983): ppsnark's batched inner sum-check, nine claims over the sixteen
    tables of PPS_TABLES (that order), each of 2^len(rhos) elements -- CUDA tensors, bound IN PLACE (contents unspecified afterwards), or
    host arrays (uploaded for the call, left untouched); no two tables may share memory.  rhos, r_outer (len(rhos) elements each),
    claims2 (claim_ABC, claim_E) and coeffs (nine) are host.  Returns (round polynomials [rounds][4], challenges [rounds], the sixteen
    tables' values at r) as 32-byte strings."""
    import ctypes
    assert len(tables) == len(PPS_TABLES), "sixteen tables, in the order of PPS_TABLES"
    rh, ro = _host_u8(rhos, 32), _host_u8(r_outer, 32)
    nr = rh.size // 32
    assert ro.size // 32 == nr, "one r_outer per rho"
    parts = [_vec(x) for x in tables]
    dev = parts[0][2]
    assert all(pt[2] == dev for pt in parts), "all tables in HBM or all on the host"
    assert all(pt[1] == (1 << nr) for pt in parts), "every table holds 2^len(rhos) elements"
    ptrs = (ctypes.c_void_p * len(parts))(*[pt[0] for pt in parts])
    c2 = _host_u8(b"".join(claims2) if isinstance(claims2, (list, tuple)) else claims2, 32)
    co = _host_u8(b"".join(coeffs) if isinstance(coeffs, (list, tuple)) else coeffs, 32)
    assert c2.size == 64 and co.size == 9 * 32, "two claims, nine coefficients"
    polys, r, fin = np.zeros(128 * max(nr, 1), np.uint8), np.zeros(32 * max(nr, 1), np.uint8), np.zeros(32 * len(parts), np.uint8)
    cb = as_transcript(transcript)
    _check(L.lib().nmx_sumcheck_prove_ppsnark(field, nr, ptrs, rh.ctypes.data if nr else None, ro.ctypes.data if nr else None, c2.ctypes.data,
                                             co.ctypes.data, _flags(dev, mont), cb, ctx, polys.ctypes.data, r.ctypes.data, fin.ctypes.data))
    return _rows(polys, nr, 4), [x[0] for x in _rows(r, nr, 1)], [x[0] for x in _rows(fin, len(parts), 1)]


# ---- R1CSShape::is_sat / is_sat_relaxed as one call (nmx_r1cs_is_sat; src/r1cs/mod.rs:474-574) -----------------------------------
class SatResult:
    """Answer of r1cs_is_sat / r1cs_is_sat_relaxed.  `ok` is the reference's Ok(()); eq_ok false is its UnSat "... is unsatisfiable",
    eq_ok true with a comm_*_ok false its UnSat "Invalid commitment(s)" (the reference reports the equation first).  bad_rows = number of
    violated constraints, first_bad_row = the lowest one (None when there is none)."""

    def __init__(self, verdict, bad_rows, first_bad_row):
        self.verdict = verdict
        self.eq_ok = not (verdict & L.UNSAT_EQ)
        self.comm_W_ok = not (verdict & L.UNSAT_COMM_W)
        self.comm_E_ok = not (verdict & L.UNSAT_COMM_E)
        self.ok = verdict == 0
        self.bad_rows = bad_rows
        self.first_bad_row = None if first_bad_row == 2 ** 64 - 1 else first_bad_row

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return (f"SatResult(ok={self.ok}, eq_ok={self.eq_ok}, comm_W_ok={self.comm_W_ok}, comm_E_ok={self.comm_E_ok}, "
                f"bad_rows={self.bad_rows}, first_bad_row={self.first_bad_row})")


def _expected_point(c):
    """Commitment / (xy64, is_inf) / 64 bytes (all zero = the identity) -> (array, is_inf)"""
    if c is None:
        return None, 0
    if hasattr(c, "xy"):
        xy, inf = c.xy, c.is_inf
    elif isinstance(c, (tuple, list)) and len(c) == 2:
        xy, inf = c
    else:
        xy, inf = c, None
    a = _host_u8(xy, 64)
    assert a.size == 64
    return a, int(bool(inf) if inf is not None else not a.any())


def _is_sat(A, B, C, ck, W, E, u, X, comm_W, comm_E, r_W, r_E, h, mont):
    import ctypes
    pw, nw, dev, _kw = _vec(W)
    pe, ne = None, 0
    if E is not None:
        pe, ne, deve, _ke = _vec(E)
        assert deve == dev, "W and E: both in HBM or both on the host"
    xx = _host_u8(X, 32)
    uu = _chal(u) if u is not None else None
    rw = _host_u8(bytes(32) if r_W is None else r_W, 32)
    re_ = _host_u8(bytes(32) if r_E is None else r_E, 32)
    cw, cw_inf = _expected_point(comm_W)
    ce, ce_inf = _expected_point(comm_E)
    hh = _host_u8((ck.h if ck is not None else bytes(64)) if h is None else h, 64)
    flags = _flags(dev, mont) | (L.BASES_MONT if (ck is not None and ck.mont) else 0)
    verdict, bad, first = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(L.lib().nmx_r1cs_is_sat(A.handle, B.handle, C.handle, ck.handle if ck is not None else 0, pw, nw, pe, ne, ptr(uu),
                                   xx.ctypes.data if xx.size else None, xx.size // 32, rw.ctypes.data, re_.ctypes.data, hh.ctypes.data,
                                   ptr(cw), cw_inf, ptr(ce), ce_inf, flags, ctypes.byref(verdict), ctypes.byref(bad), ctypes.byref(first)))
    return SatResult(verdict.value, bad.value, first.value)


def r1cs_is_sat(A, B, C, ck, W, X, comm_W, r_W=None, h=None, mont=False):
    """R1CSShape::is_sat (src/r1cs/mod.rs:532-574): (A z)(B z) == C z on every row with z = [W, 1, X], and commit(ck, W, r_W) == comm_W.
    A, B, C: SparseMatrix of one shape over the scalar field of ck's curve; W: CUDA tensor (used in place) or host array (uploaded);
    X: host; comm_W: Commitment, (xy64, is_inf) or 64 bytes, in the key's form (Montgomery when ck.mont, like h); ck=None: the equation
    only.  Returns a SatResult."""
    return _is_sat(A, B, C, ck, W, None, None, X, comm_W, None, r_W, None, h, mont)


def r1cs_is_sat_relaxed(A, B, C, ck, W, E, u, X, comm_W, comm_E, r_W=None, r_E=None, h=None, mont=False):
    """R1CSShape::is_sat_relaxed (src/r1cs/mod.rs:474-529): (A z)(B z) == u (C z) + E with z = [W, u, X], commit(ck, W, r_W) == comm_W
    and commit(ck, E, r_E) == comm_E -- the two commitments run beside the equation pass.  Operands as r1cs_is_sat."""
    return _is_sat(A, B, C, ck, W, E, u, X, comm_W, comm_E, r_W, r_E, h, mont)
